// format_seq.hip — hit records to the lines of kaijux / kaijup (gfx950, wave64): the passes of kj_format_seq.h as kernels.  The
// size of the text is known on the device only, so every kernel behind the first sizes itself from counts in device memory
// (grid-stride over records / blocks of output) and nothing waits for the host.
//
//   k_fs_len            a team of 32 lanes per record, two records per wavefront: the decision, the sorted places of the
//                       sequence names by shuffles inside the team (registers only), for kaijup the fragment scan of the reads
//                       the decision left unclassified (a segmented scan over the team per 32 letters), the length of the
//                       line; counts of 'C' lines, inexact and truncated records
//   kjl::k_scan_sums / k_scan_top / k_scan_apply <FsCount>   line_off[] = prefix sum of the lengths (64 bit; kj_lines.h)
//   k_fs_mid            best and the ids column of every 'C' line that fits, by the record's team, into the shadow of the output
//   k_fs_write          per lane 16 aligned bytes of the output: kjl::write_blocks over format_schunk
//   k_fs_finish         kaiju_gpu_format_verbose_info, by one lane with ordinary stores
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/kaiju_gpu.h"
#include "kj_format_seq.h"
#include "kj_lines.h"

using namespace kjq;

namespace {

constexpr int kFsBlock = 256;
constexpr uint32_t kTeamsPerBlock = kFsBlock / kTeam;
static_assert(kFsBlock == (int)kBlockLanes && kFsBlock == (int)kScanBlock && kFsBlock == kjs::kScanLanes,
              "one lane per chunk of a block of output / element of a scan block");

// lane k of the caller's team (teams are 32 aligned lanes of a wavefront)
struct TeamShfl {
  __device__ uint64_t id(uint64_t mine, uint32_t k) const { return (uint64_t)__shfl((unsigned long long)mine, (int)k, (int)kTeam); }
  __device__ uint32_t piece(uint32_t mine, uint32_t k) const { return (uint32_t)__shfl((int)mine, (int)k, (int)kTeam); }
  __device__ Seg seg(const Seg &mine, uint32_t k) const {
    return Seg{(uint32_t)__shfl((int)mine.len, (int)k, (int)kTeam), (uint32_t)__shfl((int)mine.sum, (int)k, (int)kTeam),
               (uint32_t)__shfl((int)mine.brk, (int)k, (int)kTeam)};
  }
};

// does read 1 of record r hold a fragment (the kaijup rule)?  Every lane of the team calls it and gets the same answer
__device__ bool team_has_fragment(const Job &J, uint32_t r, uint32_t i, uint64_t l1) {
  const TeamShfl x;
  const uint64_t steps = frag_steps(l1);
  Seg carry{0, 0, 0};
  uint32_t hit = 0;
  for (uint64_t s = 0; s < steps; s++) {
    const uint32_t d = frag_letter(J, r, s * kTeam + i, l1);
    Seg me = frag_init(d);
#pragma unroll
    for (uint32_t delta = 1; delta < kTeam; delta <<= 1) me = frag_round(me, x.seg(me, i >= delta ? i - delta : i), i, delta);
    me = frag_close(me, carry);
    hit |= frag_hit(J, d, me) ? 1u : 0u;
    carry = x.seg(me, kTeam - 1);
  }
#pragma unroll
  for (int d = 1; d < (int)kTeam; d <<= 1) hit |= (uint32_t)__shfl_xor((int)hit, d, (int)kTeam);
  return hit != 0;
}

struct FsCount { const Hdr *hdr; __device__ uint64_t operator()() const { return hdr->n; } };   // elements of the scan

__global__ void k_fs_init(Hdr *h, uint32_t n) {
  if (blockIdx.x || threadIdx.x) return;
  *h = Hdr{0, n, 0, 0, 0};
}

__global__ __launch_bounds__(kFsBlock) void k_fs_len(Job J, uint32_t n) {
  const uint32_t i = threadIdx.x & (kTeam - 1);
  const uint32_t team = blockIdx.x * kTeamsPerBlock + threadIdx.x / kTeam, n_teams = gridDim.x * kTeamsPerBlock;
  const TeamShfl x;
  uint32_t nc = 0, ni = 0, nt = 0;
  for (uint32_t r = team; r < n; r += n_teams) {
    const Head h = record_head(J, r);
    uint64_t len, code;
    if (h.classified) {
      const Lane me = load_lane(J, r, i, h);
      uint32_t id_off, ids_len;
      round_ids(x, me, i, &id_off, &ids_len);
      len = line_len_c(h, ids_len);
      code = kCodeC;
    } else {
      bool scan;
      bool gated = u_gated(J, h, &scan);
      if (scan) gated = !team_has_fragment(J, r, i, h.l1);            // (the same branch for every lane of the team)
      len = line_len_u(h, gated);
      code = gated ? kCodeGated : kCodeU;
    }
    if (i == 0) {
      J.llen[r] = len;
      J.code[r] = code;
      nc += h.classified;
      ni += h.inexact;
      nt += h.truncated;
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { nc += __shfl_xor(nc, d, 64); ni += __shfl_xor(ni, d, 64); nt += __shfl_xor(nt, d, 64); }
  if ((threadIdx.x & 63) == 0) {
    if (nc) atomicAdd(&J.hdr->n_classified, nc);
    if (ni) atomicAdd(&J.hdr->n_inexact, ni);
    if (nt) atomicAdd(&J.hdr->n_truncated, nt);
  }
}

__global__ __launch_bounds__(kFsBlock) void k_fs_mid(Job J) {
  const uint32_t n = J.hdr->n;
  const uint32_t i = threadIdx.x & (kTeam - 1);
  const uint32_t team = blockIdx.x * kTeamsPerBlock + threadIdx.x / kTeam, n_teams = gridDim.x * kTeamsPerBlock;
  const TeamShfl x;
  for (uint32_t r = team; r < n; r += n_teams) {
    if (J.code[r] != kCodeC || J.line_off[r + 1] > J.out_cap) continue;   // (the same for every lane of the team)
    const Head h = record_head(J, r);
    const Lane me = load_lane(J, r, i, h);
    uint32_t id_off, ids_len;
    round_ids(x, me, i, &id_off, &ids_len);
    mid_lane(J, h, me, i, id_off, ids_len, J.shadow + J.line_off[r] + 3 + h.name.len);
  }
}

__global__ __launch_bounds__(kFsBlock) void k_fs_write(Job J) {
  kjl::write_blocks(J.line_off, J.hdr->n, J.out, J.out_cap,
                    [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) { return format_schunk(J, c, lo, hi, total, v); });
}

__global__ void k_fs_finish(Job J) {
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t n = J.hdr->n;
  J.hdr->written = kjv::written_bytes(J.line_off, n, J.out_cap);
  *J.info = kjv::make_info(J.line_off[n], *J.hdr, J.out_cap);
}

// ---- host side: scratch and the queue of passes ----------------------------------------------------------------------
void carve(kjl::Carver &c, Job &J, uint32_t n) {
  const size_t nblk = (size_t)n / kScanBlock + 2;
  J.llen = c.take<uint64_t>((size_t)n + 1);
  J.line_off = c.take<uint64_t>((size_t)n + 1);
  J.code = c.take<uint64_t>((size_t)n + 1);
  J.oblk = c.take<uint64_t>(nblk);
  J.oblk_base = c.take<uint64_t>(nblk + 1);
  J.hdr = c.take<Hdr>(1);
}
}  // namespace

int kj_fs_lengths(kjl::Lines &st, hipStream_t s, Job &J, uint32_t n, const char **err) {
  *err = "";
  if (!J.pw || (n && (!J.hits || !J.off || !J.names)) || (!J.names_text && J.names_bytes) ||
      (n && J.pep && (!J.text_pos || !J.text_len)) || (n && J.u_rule == KAIJU_GPU_U_RULE_PROTEIN && !J.seqs)) {
    *err = "NULL argument";
    return KAIJU_GPU_ERR_ARG;
  }
  if (J.u_rule != KAIJU_GPU_U_RULE_NUCLEOTIDE && J.u_rule != KAIJU_GPU_U_RULE_PROTEIN) { *err = "u_rule must be KAIJU_GPU_U_RULE_NUCLEOTIDE or _PROTEIN"; return KAIJU_GPU_ERR_ARG; }
  if (J.names_bytes > kjf::kMaxBytes || n > kjf::kMaxRecords) { *err = "the names must be below 2^32 - 32 bytes, a batch below 2^31 records"; return KAIJU_GPU_ERR_ARG; }
  if (!J.sn_blob || !J.sn_len || !J.sn_off) { *err = "no sequence-name table"; return KAIJU_GPU_ERR_ARG; }
  J.out = nullptr; J.out_cap = 0; J.info = nullptr; J.shadow = nullptr;
  kjl::Carver measure{nullptr};
  carve(measure, J, n);
  if (int rc = st.mem.reserve(measure.at, 256, "hipMalloc of the sequence format scratch", err)) return rc;
  kjl::Carver c{static_cast<uint8_t *>(st.mem.p)};
  carve(c, J, n);
  st.total = J.line_off + n;
  st.written = &J.hdr->written;

  const dim3 blk(kFsBlock);
  const dim3 tgrid((unsigned)std::min<uint64_t>(8192, (uint64_t)n / kTeamsPerBlock + 1));
  const dim3 ogrid((unsigned)std::min<uint64_t>(2048, (uint64_t)n / kScanBlock + 1));
  hipLaunchKernelGGL(k_fs_init, dim3(1), dim3(64), 0, s, J.hdr, n);
  hipLaunchKernelGGL(k_fs_len, tgrid, blk, 0, s, J, n);
  kjl::launch_offsets(s, ogrid, FsCount{J.hdr}, J.llen, J.oblk, J.oblk_base, J.line_off);
  if (hipGetLastError() != hipSuccess) { *err = "a kernel of the sequence format passes could not be launched"; return KAIJU_GPU_ERR_HIP; }
  return KAIJU_GPU_OK;
}

int kj_fs_write(kjl::Lines &st, hipStream_t s, Job &J, uint32_t n, void *d_out, uint64_t out_cap, kaiju_gpu_format_verbose_info *d_info, const char **err) {
  *err = "";
  if (!J.hdr || !d_info || (!d_out && out_cap)) { *err = "NULL argument"; return KAIJU_GPU_ERR_ARG; }
  if ((uintptr_t)d_out & (kChunk - 1)) { *err = "the output pointer must be 16-byte aligned"; return KAIJU_GPU_ERR_ARG; }
  if (int rc = st.shadow.reserve(out_cap, 64, "hipMalloc of the shadow of the output (out_cap bytes)", err)) return rc;
  J.out = static_cast<uint8_t *>(d_out); J.out_cap = out_cap; J.info = d_info; J.shadow = static_cast<uint8_t *>(st.shadow.p);
  const dim3 blk(kFsBlock);
  const dim3 tgrid((unsigned)std::min<uint64_t>(8192, (uint64_t)n / kTeamsPerBlock + 1));
  const dim3 wgrid((unsigned)std::min<uint64_t>(8192, out_cap / kBlockBytes + 1));
  hipLaunchKernelGGL(k_fs_mid, tgrid, blk, 0, s, J);
  hipLaunchKernelGGL(k_fs_write, wgrid, blk, 0, s, J);
  hipLaunchKernelGGL(k_fs_finish, dim3(1), dim3(64), 0, s, J);
  if (hipGetLastError() != hipSuccess) { *err = "a kernel of the sequence format passes could not be launched"; return KAIJU_GPU_ERR_HIP; }
  return KAIJU_GPU_OK;
}
