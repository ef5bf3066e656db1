// format.hip — 16-byte records to the lines of the output file (gfx950, wave64): the passes of kj_format.h as kernels.  The
// size of the text is known on the device only, so every kernel behind the first sizes itself from counts in device memory
// (grid-stride over records / blocks of output) and nothing waits for the host.
//
//   k_fmt_len           per record: the decision (the taxon to print), the length of the line; counts of 'C' lines and of
//                       records flagged inexact; the header of the call
//   kjl::k_scan_sums / k_scan_top / k_scan_apply <FmtCount>   line_off[] = prefix sum of the lengths (64 bit; kj_lines.h)
//   k_fmt_write         per lane 16 aligned bytes of the output, whole lines of memory per wavefront: kjl::write_blocks over
//                       format_chunk
//   k_fmt_finish        kaiju_gpu_format_info, by one lane with ordinary stores
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/kaiju_gpu.h"
#include "kj_format.h"
#include "kj_lines.h"

using namespace kjf;

namespace {

constexpr int kFmtBlock = 256;
static_assert(kFmtBlock == (int)kBlockLanes && kFmtBlock == (int)kScanBlock && kFmtBlock == kjs::kScanLanes,
              "one lane per chunk of a block of output / element of a scan block");

struct FmtHdr { uint64_t written; uint32_t n, n_classified, n_inexact, pad; };

struct FmtJob {
  Params P;
  const double *pw;
  const kaiju_gpu_compact *recs;
  const uint64_t *off;
  const uint8_t *text;
  uint64_t bytes1;
  const kaiju_gpu_name_span *names;
  uint8_t *out;
  uint64_t out_cap;
  kaiju_gpu_format_info *info;
  uint32_t *llen;                      // n
  uint64_t *line_off, *tax;            // n + 1, n
  uint64_t *oblk, *oblk_base;          // per block of kScanBlock records (+ 1)
  FmtHdr *hdr;
};

struct FmtCount { const FmtHdr *hdr; __device__ uint64_t operator()() const { return hdr->n; } };   // elements of the scan

__global__ void k_fmt_init(FmtHdr *h, uint32_t n) {
  if (blockIdx.x || threadIdx.x) return;
  *h = FmtHdr{0, n, 0, 0, 0};
}

__global__ __launch_bounds__(kFmtBlock) void k_fmt_len(FmtJob J, uint32_t n) {
  uint32_t nc = 0, ni = 0;
  for (uint32_t r = blockIdx.x * kFmtBlock + threadIdx.x; r < n; r += gridDim.x * kFmtBlock) {
    uint64_t t;
    J.llen[r] = record_line(J.recs, J.off, J.names, r, J.bytes1, J.P, J.pw, &t);
    J.tax[r] = t;
    nc += t ? 1u : 0u;
    ni += (J.recs[r].info & KAIJU_HIT_INEXACT) ? 1u : 0u;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { nc += __shfl_xor(nc, d, 64); ni += __shfl_xor(ni, d, 64); }
  if ((threadIdx.x & 63) == 0) {
    if (nc) atomicAdd(&J.hdr->n_classified, nc);
    if (ni) atomicAdd(&J.hdr->n_inexact, ni);
  }
}

__global__ __launch_bounds__(kFmtBlock) void k_fmt_write(FmtJob J) {
  kjl::write_blocks(J.line_off, J.hdr->n, J.out, J.out_cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) {
    return format_chunk(c, J.text, J.bytes1, J.names, J.line_off, J.tax, lo, hi, total, J.out_cap, v);
  });
}

__global__ void k_fmt_finish(FmtJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t n = J.hdr->n;
  const uint64_t total = J.line_off[n];
  // the lines that fit: line_off[0 .. k] with line_off[k] <= out_cap
  J.hdr->written = total <= J.out_cap ? total : J.line_off[find_record(J.line_off, 0, n + 1, J.out_cap)];
  *J.info = make_info(total, n, J.hdr->n_classified, J.hdr->n_inexact, J.out_cap);
}

// ---- host side: scratch and the queue of passes ----------------------------------------------------------------------
void carve(kjl::Carver &c, FmtJob &J, uint32_t n) {
  const size_t nblk = (size_t)n / kScanBlock + 2;
  J.llen = c.take<uint32_t>((size_t)n + 1);
  J.line_off = c.take<uint64_t>((size_t)n + 1);
  J.tax = c.take<uint64_t>((size_t)n + 1);
  J.oblk = c.take<uint64_t>(nblk);
  J.oblk_base = c.take<uint64_t>(nblk + 1);
  J.hdr = c.take<FmtHdr>(1);
}
}  // namespace

int kj_format_launch(kjl::Lines &st, hipStream_t s, const Params &P, const double *d_pw, const kaiju_gpu_compact *d_recs,
                     const uint64_t *d_off, uint32_t n, const void *d_text1, uint64_t bytes1, const kaiju_gpu_name_span *d_names,
                     void *d_out, uint64_t out_cap, kaiju_gpu_format_info *d_info, const char **err) {
  *err = "";
  if (!d_info || !d_pw || (n && (!d_recs || !d_off || !d_names)) || (!d_text1 && bytes1) || (!d_out && out_cap)) {
    *err = "NULL argument";
    return KAIJU_GPU_ERR_ARG;
  }
  if (bytes1 > kMaxBytes || n > kMaxRecords) { *err = "a block of text must be below 2^32 - 32 bytes, a batch below 2^31 records"; return KAIJU_GPU_ERR_ARG; }
  if ((uintptr_t)d_out & (kChunk - 1)) { *err = "the output pointer must be 16-byte aligned"; return KAIJU_GPU_ERR_ARG; }
  FmtJob J{};
  kjl::Carver measure{nullptr};
  carve(measure, J, n);
  if (int rc = st.mem.reserve(measure.at, 256, "hipMalloc of the format scratch", err)) return rc;
  kjl::Carver c{static_cast<uint8_t *>(st.mem.p)};
  carve(c, J, n);
  st.total = J.line_off + n;
  st.written = &J.hdr->written;
  J.P = P; J.pw = d_pw; J.recs = d_recs; J.off = d_off; J.text = static_cast<const uint8_t *>(d_text1); J.bytes1 = bytes1;
  J.names = d_names; J.out = static_cast<uint8_t *>(d_out); J.out_cap = out_cap; J.info = d_info;

  const dim3 blk(kFmtBlock);
  const dim3 rgrid((unsigned)std::min<uint64_t>(4096, (uint64_t)n / kFmtBlock + 1));
  const dim3 ogrid((unsigned)std::min<uint64_t>(2048, (uint64_t)n / kScanBlock + 1));
  // blocks of the write pass: how many bytes there are is known on the device only (at most name bytes + 24 per record)
  const uint64_t most = std::min<uint64_t>(out_cap, bytes1 + (uint64_t)kLineExtra * n);
  const dim3 wgrid((unsigned)std::min<uint64_t>(8192, most / kBlockBytes + 1));
  hipLaunchKernelGGL(k_fmt_init, dim3(1), dim3(64), 0, s, J.hdr, n);
  hipLaunchKernelGGL(k_fmt_len, rgrid, blk, 0, s, J, n);
  kjl::launch_offsets(s, ogrid, FmtCount{J.hdr}, J.llen, J.oblk, J.oblk_base, J.line_off);
  hipLaunchKernelGGL(k_fmt_write, wgrid, blk, 0, s, J);
  hipLaunchKernelGGL(k_fmt_finish, dim3(1), dim3(64), 0, s, J);
  if (hipGetLastError() != hipSuccess) { *err = "a kernel of the format passes could not be launched"; return KAIJU_GPU_ERR_HIP; }
  return KAIJU_GPU_OK;
}
