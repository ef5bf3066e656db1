// sufsort.hip - the suffix sort of the index builder on the device (gfx950): prefix doubling over ranks, kj_sufsort.h has the
// definition, the rank invariant and the per-lane logic.  Here: the kernels and the driver loop.  The stable radix sort of
// (64-bit key, 32-bit position) and the prefix scans are rocPRIM's; everything else is below.
//
// Passes.  Round 1: k_ss_count (letters per tile of 4096 text bytes) -> exclusive scan of the tile counts -> k_ss_keys (keys
// of 12 symbols and positions in position order, sequence numbers as ranks of the terminators) -> radix sort, 60 bits.
// Round h: k_ss_round_keys (rank[p] << 32 | rank[p + h] of the active list) -> radix sort.  Every round then: k_ss_heads ->
// inclusive max-scan of (last old head, last new head) -> k_ss_ranks (new ranks, flags of what stays active) -> inclusive scan
// of the flags -> k_ss_compact (the next active list) -> ONE read-back: the active count.  At the end k_ss_scatter writes
// SA[rank[p] - nseq] = p.  All memory is allocated in front of round 1 (ss_scratch_bytes + rocPRIM's temporary storage,
// compared with the free HBM first).
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <string>

#include "kj_sufsort.h"
#include "mkfmi.h"

static_assert((int)KJ_SS_STATS_ROUNDS == (int)KAIJU_SUFSORT_STATS_ROUNDS, "kaiju_sufsort_stats");

namespace {

// ---- kernels -------------------------------------------------------------------------------------------------------------
// text is allocated to ss_text_alloc(tlen) bytes, zero behind tlen: lane g reads bytes [16 g, 16 g + 32)
__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_count(const uint4 *__restrict__ text, uint64_t nlanes, uint32_t *__restrict__ tile_count) {
  const uint64_t g = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x;
  uint32_t c = 0;
  if (g < nlanes) {
    const uint4 v = text[g];
    c = ss_lane_letters((uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32));
  }
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  __shared__ uint32_t part[KJ_SS_BLOCK / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < KJ_SS_BLOCK / 64; w++) s += part[w];
    tile_count[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_keys(const uint4 *__restrict__ text, uint64_t nlanes, uint64_t tlen, uint64_t nsuf,
                                                        const uint32_t *__restrict__ tile_base, uint64_t *__restrict__ keys,
                                                        uint32_t *__restrict__ vals, uint32_t *__restrict__ rank) {
  const uint64_t g = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x;
  uint64_t k[KJ_SS_LANE_BYTES];
  uint32_t letters = 0;
  if (g < nlanes) {
    const uint4 a = text[g], b = text[g + 1];
    const uint64_t w[4] = {(uint64_t)a.x | ((uint64_t)a.y << 32), (uint64_t)a.z | ((uint64_t)a.w << 32),
                           (uint64_t)b.x | ((uint64_t)b.y << 32), (uint64_t)b.z | ((uint64_t)b.w << 32)};
    letters = ss_lane_keys(w, k);
  }
  // exclusive prefix of the letter counts inside the block
  const uint32_t cnt = __popc(letters);
  uint32_t inc = cnt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
  __shared__ uint32_t part[KJ_SS_BLOCK / 64];
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; w++) before += part[w];
  if (g >= nlanes) return;
  uint64_t o = (uint64_t)tile_base[blockIdx.x] + before + inc - cnt;     // letters in front of the lane's first byte
  const uint64_t p0 = g * KJ_SS_LANE_BYTES;
#pragma unroll
  for (int j = 0; j < KJ_SS_LANE_BYTES; j++) {
    const uint64_t p = p0 + j;
    if ((letters >> j) & 1u) {
      if (o < nsuf) { keys[o] = k[j]; vals[o] = (uint32_t)p; }
      o++;
    } else if (p < tlen) {
      rank[p] = (uint32_t)(p - o);          // a terminator: its sequence number = the terminators in front of it
    }
  }
}

__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_round_keys(const uint32_t *__restrict__ act, uint64_t m, const uint32_t *__restrict__ rank,
                                                              uint64_t h, uint64_t tlen, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  for (uint64_t i = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const uint32_t p = act[i];
    keys[i] = p < tlen ? ss_round_key(rank, p, h, tlen) : 0ull;
    vals[i] = p;
  }
}

__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_heads(const uint64_t *__restrict__ keys, uint64_t m, int first, uint64_t *__restrict__ items) {
  for (uint64_t i = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const uint64_t k = keys[i], kp = i ? keys[i - 1] : 0ull;
    items[i] = first ? ss_scan_item((uint32_t)i, false, ss_head_first(i, kp, k))
                     : ss_scan_item((uint32_t)i, ss_head_old(i, kp, k), ss_head_new(i, kp, k));
  }
}

__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_ranks(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                         const uint64_t *__restrict__ scanned, uint64_t m, int first, uint32_t nseq, uint64_t tlen,
                                                         uint32_t *__restrict__ rank, uint32_t *__restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const uint64_t s = scanned[i], sn = i + 1 < m ? scanned[i + 1] : 0ull;
    const uint32_t p = vals[i];
    if (p < tlen) rank[p] = first ? ss_rank_first(nseq, s) : ss_rank_round(keys[i], s);
    flags[i] = ss_is_final(i, m, s, sn) ? 0u : 1u;
  }
}

__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_compact(const uint32_t *__restrict__ vals, const uint32_t *__restrict__ incl, uint64_t m,
                                                           uint32_t *__restrict__ act) {
  for (uint64_t i = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const uint32_t c = incl[i], b = i ? incl[i - 1] : 0u;
    if (c != b && c <= m) act[c - 1] = vals[i];        // (c <= i + 1 by construction)
  }
}

// rank is allocated to 16 nlanes entries: lane g reads its 16
__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_scatter(const uint4 *__restrict__ text, const uint4 *__restrict__ rank, uint64_t nlanes,
                                                           uint32_t nseq, uint64_t nsuf, uint32_t *__restrict__ sa) {
  for (uint64_t g = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; g < nlanes; g += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const uint4 t = text[g];
    const uint32_t tw[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (!tw[q]) continue;
      const uint4 r = rank[g * 4 + q];
      const uint32_t rw[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (!((tw[q] >> (8 * j)) & 0xffu)) continue;
        const uint64_t row = (uint64_t)rw[j] - nseq;       // (wraps to a huge value if the rank were below nseq)
        if (row < nsuf) sa[row] = (uint32_t)(g * KJ_SS_LANE_BYTES + q * 4 + j);
      }
    }
  }
}

// ---- driver ---------------------------------------------------------------------------------------------------------------
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
  template <class T> T *as() { return static_cast<T *>(p); }
};
struct Events {
  hipEvent_t a = nullptr, b = nullptr;
  ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};
struct DeviceGuard {
  int prev = -1;
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

unsigned grid_for(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + KJ_SS_BLOCK - 1) / KJ_SS_BLOCK, 2048)); }
int bits_of(uint64_t v) { int b = 0; while (v >> b) ++b; return b; }

#define SS_HIP(call)                                                                                          \
  do {                                                                                                        \
    const hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) { err = std::string("suffix sort on the device: ") + #call + ": " + hipGetErrorString(e_); return KAIJU_GPU_ERR_HIP; } \
  } while (0)

size_t sort_temp(uint64_t n, unsigned end_bit) {
  rocprim::double_buffer<uint64_t> k(nullptr, nullptr);
  rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
  size_t s = 0;
  (void)rocprim::radix_sort_pairs(nullptr, s, k, v, (size_t)n, 0u, end_bit);
  return s;
}
size_t scan64_temp(uint64_t n) { size_t s = 0; (void)rocprim::inclusive_scan(nullptr, s, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, SsScanMax()); return s; }
size_t scan32_temp(uint64_t n) { size_t s = 0; (void)rocprim::inclusive_scan(nullptr, s, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, rocprim::plus<uint32_t>()); return s; }
size_t tile_temp(uint64_t n) { size_t s = 0; (void)rocprim::exclusive_scan(nullptr, s, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>()); return s; }

}  // namespace

int kj_sufsort_check_device(int device_id, std::string &err) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { err = "suffix sort on the device: no HIP device (kaiju_build_fmi is the host builder)"; return KAIJU_GPU_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= n) { err = "suffix sort on the device: device_id " + std::to_string(device_id) + " of " + std::to_string(n) + " devices"; return KAIJU_GPU_ERR_ARG; }
  return KAIJU_GPU_OK;
}

int kj_sufsort_device(const uint8_t *text, uint64_t tlen, int device_id, uint32_t *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats,
                      std::string &err) {
  return kj_sufsort_device_keep(text, tlen, device_id, sa_out, n_out, stats, nullptr, err);
}

// what one sort allocates (the caller has selected the device: rocPRIM sizes its temporary storage for it)
uint64_t kj_sufsort_need_bytes(uint64_t tlen, uint64_t nsuf, uint64_t *temp_bytes_out) {
  const uint64_t n = std::max<uint64_t>(nsuf, 1);
  const uint64_t nlanes = (tlen + KJ_SS_LANE_BYTES - 1) / KJ_SS_LANE_BYTES, ntiles = (nlanes + KJ_SS_BLOCK - 1) / KJ_SS_BLOCK;
  const uint64_t rank_entries = nlanes * KJ_SS_LANE_BYTES;
  const unsigned round_bits = 32u + (unsigned)bits_of(tlen);
  const size_t temp_bytes = std::max({sort_temp(n, KJ_SS_KEY_BITS), sort_temp(n, round_bits), scan64_temp(n), scan32_temp(n), tile_temp(ntiles)});
  if (temp_bytes_out) *temp_bytes_out = temp_bytes;
  return ss_scratch_bytes(tlen, nsuf) + 4 * (rank_entries - tlen) + temp_bytes + 4 * ntiles;
}

// keep != nullptr: SA is not downloaded (sa_out may be nullptr); text, rank[], SA, the first key buffer and the temporary
// storage stay allocated and are handed to the caller, who frees them (hipFree) - also for a text without a suffix, whose
// terminators still get their ranks
int kj_sufsort_device_keep(const uint8_t *text, uint64_t tlen, int device_id, uint32_t *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats,
                           SsKeep *keep, std::string &err) {
  if (stats) memset(stats, 0, sizeof *stats);
  if (n_out) *n_out = 0;
  if (!ss_tlen_ok(tlen)) {
    err = "suffix sort on the device: 32-bit positions only (text of " + std::to_string(tlen) + " symbols); kaiju_build_fmi, the host builder, sorts with 64-bit positions";
    return KAIJU_GPU_ERR_ARG;
  }
  if (!text || tlen == 0 || (!sa_out && !keep)) { err = "suffix sort on the device: no text"; return KAIJU_GPU_ERR_ARG; }
  if (text[tlen - 1] != 0) { err = "suffix sort on the device: the text does not end with a terminator"; return KAIJU_GPU_ERR_ARG; }
  int rc = kj_sufsort_check_device(device_id, err);
  if (rc != KAIJU_GPU_OK) return rc;
  // sequences and the longest of them: the bound of the round loop
  uint64_t nseq = 0, maxlen = 0;
  for (uint64_t p = 0; p < tlen;) {
    const uint8_t *z = static_cast<const uint8_t *>(memchr(text + p, 0, (size_t)(tlen - p)));
    const uint64_t e = (uint64_t)(z - text);                 // (found: the last byte is a terminator)
    maxlen = std::max(maxlen, e - p);
    nseq++;
    p = e + 1;
  }
  const uint64_t nsuf = tlen - nseq;
  if (n_out) *n_out = nsuf;
  if (nsuf == 0 && !keep) return KAIJU_GPU_OK;

  DeviceGuard dg;
  SS_HIP(hipGetDevice(&dg.prev));
  SS_HIP(hipSetDevice(device_id));

  const uint64_t nlanes = (tlen + KJ_SS_LANE_BYTES - 1) / KJ_SS_LANE_BYTES, ntiles = (nlanes + KJ_SS_BLOCK - 1) / KJ_SS_BLOCK;
  const uint64_t text_bytes = ss_text_alloc(tlen), rank_entries = nlanes * KJ_SS_LANE_BYTES;
  const unsigned round_bits = 32u + (unsigned)bits_of(tlen);
  uint64_t temp_bytes64 = 0;
  const uint64_t need = kj_sufsort_need_bytes(tlen, nsuf, &temp_bytes64);
  const size_t temp_bytes = (size_t)temp_bytes64;
  size_t free_b = 0, total_b = 0;
  SS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b) {
    err = "suffix sort on the device: needs " + std::to_string(need >> 20) + " MiB of device memory, " + std::to_string(free_b >> 20) +
          " MiB are free; kaiju_build_fmi sorts on the host";
    return KAIJU_GPU_ERR_NOMEM;
  }
  DevBuf d_text, d_rank, d_k0, d_k1, d_v0, d_v1, d_act, d_tcnt, d_tbase, d_temp;
  SS_HIP(d_text.alloc(text_bytes));
  SS_HIP(d_rank.alloc(4 * rank_entries));
  SS_HIP(d_k0.alloc(8 * nsuf));
  SS_HIP(d_k1.alloc(8 * nsuf));
  SS_HIP(d_v0.alloc(4 * nsuf));
  SS_HIP(d_v1.alloc(4 * nsuf));
  SS_HIP(d_act.alloc(4 * nsuf));
  SS_HIP(d_tcnt.alloc(4 * ntiles));
  SS_HIP(d_tbase.alloc(4 * ntiles));
  SS_HIP(d_temp.alloc(temp_bytes));
  Events ev;
  SS_HIP(hipEventCreate(&ev.a));
  SS_HIP(hipEventCreate(&ev.b));
  const hipStream_t st = nullptr;
  SS_HIP(hipEventRecord(ev.a, st));
  SS_HIP(hipMemsetAsync(d_text.as<uint8_t>() + (text_bytes - KJ_SS_TEXT_PAD - KJ_SS_LANE_BYTES), 0, KJ_SS_TEXT_PAD + KJ_SS_LANE_BYTES, st));
  SS_HIP(hipMemcpyAsync(d_text.p, text, tlen, hipMemcpyHostToDevice, st));
  SS_HIP(hipMemsetAsync(d_rank.p, 0, 4 * rank_entries, st));

  // ---- round 1 ----
  size_t tb = temp_bytes;
  k_ss_count<<<(unsigned)ntiles, KJ_SS_BLOCK, 0, st>>>(d_text.as<uint4>(), nlanes, d_tcnt.as<uint32_t>());
  SS_HIP(hipGetLastError());
  SS_HIP(rocprim::exclusive_scan(d_temp.p, tb, d_tcnt.as<uint32_t>(), d_tbase.as<uint32_t>(), 0u, (size_t)ntiles, rocprim::plus<uint32_t>(), st));
  k_ss_keys<<<(unsigned)ntiles, KJ_SS_BLOCK, 0, st>>>(d_text.as<uint4>(), nlanes, tlen, nsuf, d_tbase.as<uint32_t>(), d_k0.as<uint64_t>(),
                                                     d_v0.as<uint32_t>(), d_rank.as<uint32_t>());
  SS_HIP(hipGetLastError());

  rocprim::double_buffer<uint64_t> kb(d_k0.as<uint64_t>(), d_k1.as<uint64_t>());
  rocprim::double_buffer<uint32_t> vb(d_v0.as<uint32_t>(), d_v1.as<uint32_t>());
  uint64_t m = nsuf, h = 0;
  uint32_t rounds = 0;
  while (m != 0) {                                          // (a text without a suffix, kept: no round)
    const int first = rounds == 0;
    if (stats && rounds < KJ_SS_STATS_ROUNDS) stats->active[rounds] = m;
    if (!first) {
      if (!ss_round_allowed(h, maxlen)) {
        err = "internal: suffix sort on the device: " + std::to_string(m) + " suffixes still active at h = " + std::to_string(h) + " beyond the longest sequence (" +
              std::to_string(maxlen) + ")";
        return KAIJU_GPU_ERR_ARG;
      }
      k_ss_round_keys<<<grid_for(m), KJ_SS_BLOCK, 0, st>>>(d_act.as<uint32_t>(), m, d_rank.as<uint32_t>(), h, tlen, kb.current(), vb.current());
      SS_HIP(hipGetLastError());
    }
    const unsigned end_bit = first ? (unsigned)KJ_SS_KEY_BITS : round_bits;
    if (sort_temp(m, end_bit) > temp_bytes || scan64_temp(m) > temp_bytes || scan32_temp(m) > temp_bytes) { err = "internal: suffix sort on the device: temporary storage"; return KAIJU_GPU_ERR_ARG; }
    tb = temp_bytes;
    SS_HIP(rocprim::radix_sort_pairs(d_temp.p, tb, kb, vb, (size_t)m, 0u, end_bit, st));
    uint64_t *items = kb.alternate();
    uint32_t *flags = vb.alternate();
    k_ss_heads<<<grid_for(m), KJ_SS_BLOCK, 0, st>>>(kb.current(), m, first, items);
    SS_HIP(hipGetLastError());
    tb = temp_bytes;
    SS_HIP(rocprim::inclusive_scan(d_temp.p, tb, items, items, (size_t)m, SsScanMax(), st));
    k_ss_ranks<<<grid_for(m), KJ_SS_BLOCK, 0, st>>>(kb.current(), vb.current(), items, m, first, (uint32_t)nseq, tlen, d_rank.as<uint32_t>(), flags);
    SS_HIP(hipGetLastError());
    tb = temp_bytes;
    SS_HIP(rocprim::inclusive_scan(d_temp.p, tb, flags, flags, (size_t)m, rocprim::plus<uint32_t>(), st));
    k_ss_compact<<<grid_for(m), KJ_SS_BLOCK, 0, st>>>(vb.current(), flags, m, d_act.as<uint32_t>());
    SS_HIP(hipGetLastError());
    uint32_t left = 0;
    SS_HIP(hipMemcpyAsync(&left, flags + (m - 1), 4, hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));                       // the one synchronisation of a round: is there another one?
    rounds++;
    h = first ? (uint64_t)KJ_SS_K : 2 * h;
    if (left > m) { err = "internal: suffix sort on the device: active count"; return KAIJU_GPU_ERR_ARG; }
    m = left;
    if (m == 0) break;
  }
  k_ss_scatter<<<grid_for(nlanes), KJ_SS_BLOCK, 0, st>>>(d_text.as<uint4>(), d_rank.as<uint4>(), nlanes, (uint32_t)nseq, nsuf, d_v0.as<uint32_t>());
  SS_HIP(hipGetLastError());
  if (!keep) SS_HIP(hipMemcpyAsync(sa_out, d_v0.p, 4 * nsuf, hipMemcpyDeviceToHost, st));
  SS_HIP(hipEventRecord(ev.b, st));
  SS_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  SS_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
  if (stats) { stats->rounds = rounds; stats->ms_sort = ms; }
  if (keep) {
    keep->text = d_text.p; keep->rank = d_rank.p; keep->sa = d_v0.p; keep->k0 = d_k0.p; keep->temp = d_temp.p;
    d_text.p = d_rank.p = d_v0.p = d_k0.p = d_temp.p = nullptr;
    keep->temp_bytes = temp_bytes; keep->nseq = nseq; keep->nsuf = nsuf; keep->maxlen = maxlen; keep->bytes = need;
  }
  return KAIJU_GPU_OK;
}
