// fmibuild.hip - the stages of the index builder behind the suffix sort on the device (gfx950, wave64): kj_fmibuild.h has the
// definitions and the per-lane logic.  Here: the kernels and the driver.  When the sort (sufsort.hip) ends, the text, rank[]
// and SA are in device memory; five passes make the arrays of the file from them, and only what the file is written from comes
// down.  Rows are indexed in 64 bits throughout (tlen * copies passes 2^32 on the wide-index builds); positions of the text
// are 32-bit, as the sorter's.
//
// Passes.  BWT: k_fb_bwt_rows (B[nseq + k] = T[SA[k] - 1], coalesced stores) and k_fb_terminators (the nseq terminator rows and
// the sequence starts, scattered).  Ranks: k_fb_flags -> inclusive scan (rocPRIM, in the sort's first key buffer) ->
// k_fb_seq_ranks -> ONE read-back, the number of whole sequences, checked against nseq.  Replication + samples: k_fb_replicate
// (8 rows per lane, one division per lane), k_fb_samples.  Checkpoints: k_fb_checkpoints, one workgroup per piece of 65 536
// rows.  Then index2's rows and the piece counts come down, the host makes startLcode (double arithmetic over 21 numbers: its
// expression stays the host's), 22 ints go up.  Coding: k_fb_recode, one wavefront per block of 256 rows, in place.  No kernel
// waits for another workgroup; every loop is bounded by its input.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <string>

#include "kj_fmibuild.h"
#include "kj_sufsort.h"
#include "mkfmi.h"

static_assert((int)KJ_FB_STAGE_BWT == (int)KAIJU_FMI_STAGE_BWT && (int)KJ_FB_STAGE_RANKS == (int)KAIJU_FMI_STAGE_RANKS &&
              (int)KJ_FB_STAGE_SAMPLES == (int)KAIJU_FMI_STAGE_SAMPLES && (int)KJ_FB_STAGE_CHECKPOINTS == (int)KAIJU_FMI_STAGE_CHECKPOINTS &&
              (int)KJ_FB_STAGE_RECODE == (int)KAIJU_FMI_STAGE_RECODE, "kaiju_fmi_build_stats");

namespace {

// ---- kernels -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KJ_FB_THREADS) void k_fb_bwt_rows(const uint8_t *__restrict__ text, const uint32_t *__restrict__ sa, uint64_t nsuf, uint64_t nseq,
                                                              uint8_t *__restrict__ B) {
  for (uint64_t k = (uint64_t)blockIdx.x * KJ_FB_THREADS + threadIdx.x; k < nsuf; k += (uint64_t)gridDim.x * KJ_FB_THREADS)
    B[nseq + k] = fb_bwt_of(text, sa[k]);
}

// text is allocated to ss_text_alloc(tlen) bytes: lane g reads bytes [4 g, 4 g + 4)
__global__ __launch_bounds__(KJ_FB_THREADS) void k_fb_terminators(const uint8_t *__restrict__ text, const uint32_t *__restrict__ rank, uint64_t tlen, uint64_t nseq,
                                                                 uint8_t *__restrict__ B, uint32_t *__restrict__ starts) {
  const uint64_t nwords = (tlen + 3) / 4;
  for (uint64_t g = (uint64_t)blockIdx.x * KJ_FB_THREADS + threadIdx.x; g < nwords; g += (uint64_t)gridDim.x * KJ_FB_THREADS) {
    const uint32_t w = reinterpret_cast<const uint32_t *>(text)[g];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint64_t p = g * 4 + j;
      if (p < tlen && ((w >> (8 * j)) & 0xffu) == 0) fb_terminator(text, rank, p, nseq, B, starts);
    }
  }
}

__global__ __launch_bounds__(KJ_FB_THREADS) void k_fb_flags(const uint8_t *__restrict__ B, uint64_t nseq, uint64_t nsuf, uint32_t *__restrict__ flags) {
  for (uint64_t k = (uint64_t)blockIdx.x * KJ_FB_THREADS + threadIdx.x; k < nsuf; k += (uint64_t)gridDim.x * KJ_FB_THREADS)
    flags[k] = B[nseq + k] == 0 ? 1u : 0u;
}

__global__ __launch_bounds__(KJ_FB_THREADS) void k_fb_seq_ranks(const uint8_t *__restrict__ B, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ rank,
                                                               const uint32_t *__restrict__ incl, uint64_t nsuf, uint64_t nseq, uint64_t r0,
                                                               uint32_t *__restrict__ read_of_rank, uint32_t *__restrict__ rank_of) {
  for (uint64_t k = (uint64_t)blockIdx.x * KJ_FB_THREADS + threadIdx.x; k < nsuf; k += (uint64_t)gridDim.x * KJ_FB_THREADS)
    if (B[nseq + k] == 0) fb_seq_rank(sa, rank, k, incl[k], r0, nseq, read_of_rank, rank_of);
}

// bwt is allocated to a multiple of KJ_FB_PAD bytes: lane g writes bytes [8 g, 8 g + 8)
__global__ __launch_bounds__(KJ_FB_THREADS) void k_fb_replicate(const uint8_t *__restrict__ B, uint64_t otlen, uint64_t copies, uint64_t *__restrict__ bwt) {
  const uint64_t nwords = (otlen + KJ_FB_REP_BYTES - 1) / KJ_FB_REP_BYTES;
  for (uint64_t g = (uint64_t)blockIdx.x * KJ_FB_THREADS + threadIdx.x; g < nwords; g += (uint64_t)gridDim.x * KJ_FB_THREADS)
    bwt[g] = fb_replicate(B, g * KJ_FB_REP_BYTES, otlen, copies);
}

__global__ __launch_bounds__(KJ_FB_THREADS) void k_fb_samples(FbPlan P, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ starts,
                                                             const uint32_t *__restrict__ rank_of, uint8_t *__restrict__ out) {
  for (uint64_t q = (uint64_t)blockIdx.x * KJ_FB_THREADS + threadIdx.x; q < P.nfill; q += (uint64_t)gridDim.x * KJ_FB_THREADS)
    fb_sample(P, q, sa, starts, rank_of, out);
}

// one workgroup per piece of 65 536 rows; lane t counts block t of the piece; index2 has nblk rows, piece_counts npieces rows
__global__ __launch_bounds__(KJ_FB_THREADS) void k_fb_checkpoints(const uint8_t *__restrict__ bwt, uint64_t otlen, uint16_t *__restrict__ index2,
                                                                 uint32_t *__restrict__ piece_counts) {
  static_assert(KJ_FB_THREADS * KJ_FB_BLOCK == KJ_FB_PIECE, "a lane per block of the piece");
  __shared__ uint32_t cnt[KJ_FB_ALEN * KJ_FB_THREADS];
  __shared__ uint32_t part[KJ_FB_ALEN][KJ_FB_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint64_t R = blockIdx.x;
  const uint64_t lo = R * KJ_FB_PIECE + (uint64_t)t * KJ_FB_BLOCK, hi = lo + KJ_FB_BLOCK < otlen ? lo + KJ_FB_BLOCK : otlen;
#pragma unroll
  for (int a = 0; a < KJ_FB_ALEN; a++) cnt[a * KJ_FB_THREADS + t] = 0;
  if (lo < otlen) fb_count_block(bwt, lo, hi, cnt + t, KJ_FB_THREADS);
  uint32_t own[KJ_FB_ALEN], inc[KJ_FB_ALEN];
#pragma unroll
  for (int a = 0; a < KJ_FB_ALEN; a++) {
    const uint32_t v = cnt[a * KJ_FB_THREADS + t];         // (the lane's own slots: no other lane wrote them)
    uint32_t s = v;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(s, d, 64); if (lane >= d) s += o; }
    own[a] = v; inc[a] = s;
    if (lane == 63) part[a][wave] = s;
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < KJ_FB_ALEN; a++) {
    uint32_t before = 0;
    for (int w = 0; w < wave; w++) before += part[a][w];
    const uint32_t excl = before + inc[a] - own[a];        // at most 65 280: 255 blocks of 256 rows
    if (lo < otlen) index2[(R * KJ_FB_THREADS + t) * KJ_FB_ALEN + a] = (uint16_t)excl;
    if (t == KJ_FB_THREADS - 1) piece_counts[R * KJ_FB_ALEN + a] = excl + own[a];
  }
}

// one wavefront per block of 256 rows, lane l holds rows 4 l .. 4 l + 3; bwt is allocated to a multiple of KJ_FB_PAD bytes
__global__ __launch_bounds__(KJ_FB_THREADS) void k_fb_recode(uint32_t *__restrict__ bwt, uint64_t otlen, uint64_t nblk, const int *__restrict__ startLcode) {
  const int lane = threadIdx.x & 63;
  const uint64_t blk = (uint64_t)blockIdx.x * (KJ_FB_THREADS / 64) + (threadIdx.x >> 6);
  if (blk >= nblk) return;                                  // (the whole wavefront)
  const uint64_t left = otlen - blk * KJ_FB_BLOCK;
  const int nvalid = left < KJ_FB_BLOCK ? (int)left : (int)KJ_FB_BLOCK;
  const uint32_t word = bwt[blk * 64 + lane];
  FbBallots bal;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    bal.valid[i] = __ballot(4 * lane + i < nvalid);
#pragma unroll
    for (int b = 0; b < KJ_FB_SYM_BITS; b++) bal.bit[i][b] = __ballot((word >> (8 * i + b)) & 1u);
  }
  bwt[blk * 64 + lane] = fb_recode_lane(bal, lane, word, nvalid, startLcode);
}

// ---- driver ---------------------------------------------------------------------------------------------------------------
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
  template <class T> T *as() { return static_cast<T *>(p); }
};
enum { FB_EVENTS = 9 };
struct Events {
  hipEvent_t e[FB_EVENTS] = {};
  ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
struct DeviceGuard {
  int prev = -1;
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

unsigned grid_for(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + KJ_FB_THREADS - 1) / KJ_FB_THREADS, 4096)); }

#define FB_HIP(call)                                                                                          \
  do {                                                                                                        \
    const hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) { err = std::string("index stages on the device: ") + #call + ": " + hipGetErrorString(e_); return KAIJU_GPU_ERR_HIP; } \
  } while (0)

}  // namespace

int kj_fmibuild_device(const uint8_t *text, const FbPlan &P, uint64_t r0, int device_id, int recode,
                       const std::function<void(FbHostOut &)> &prepare,
                       const std::function<void(const uint32_t *piece_counts, int *startLcode)> &finish,
                       const std::function<void(const char *)> &mark, kaiju_fmi_build_stats *stats, std::string &err) {
  if (stats) memset(stats, 0, sizeof *stats);
  if (!text || P.tlen == 0 || !prepare || !finish || r0 > P.nseq) { err = "index stages on the device: bad argument"; return KAIJU_GPU_ERR_ARG; }
  if (!ss_tlen_ok(P.tlen)) {
    err = "index stages on the device: 32-bit positions only (text of " + std::to_string(P.tlen) + " symbols); kaiju_build_fmi, the host builder, has 64-bit positions";
    return KAIJU_GPU_ERR_ARG;
  }
  int rc = kj_sufsort_check_device(device_id, err);
  if (rc != KAIJU_GPU_OK) return rc;
  DeviceGuard dg;
  FB_HIP(hipGetDevice(&dg.prev));
  FB_HIP(hipSetDevice(device_id));

  // ---- the size check, before anything is allocated: the sort's peak, or what is kept of it plus the stages' own --------------
  const uint64_t tlen = P.tlen, nseq = P.nseq, nsuf = P.nsuf, otlen = P.otlen;
  const uint64_t sort_need = kj_sufsort_need_bytes(tlen, nsuf, nullptr);
  const uint64_t own = fb_scratch_bytes(tlen, nseq, P.copies, P.chpt_exp), freed = std::min(sort_need, fb_sort_bytes_freed(nsuf));
  const uint64_t need = std::max(sort_need, sort_need - freed + own);
  size_t free_b = 0, total_b = 0;
  FB_HIP(hipMemGetInfo(&free_b, &total_b));
  if (stats) stats->device_bytes = need;
  if (need > free_b) {
    err = "index stages on the device: need " + std::to_string(need >> 20) + " MiB of device memory (" + std::to_string(otlen) + " rows), " +
          std::to_string(free_b >> 20) + " MiB are free; stages = host (KAIJU_FMI_STAGES_HOST) makes these arrays on the host";
    return KAIJU_GPU_ERR_NOMEM;
  }
  FbHostOut out = {nullptr, nullptr, nullptr, nullptr, nullptr};
  prepare(out);
  const uint64_t samples_bytes = fb_samples_bytes(P);
  if (!out.read_of_rank || !out.bwt || !out.piece_counts || !out.index2 || (samples_bytes && !out.samples)) {
    err = "index stages on the device: no host buffers";
    return KAIJU_GPU_ERR_ARG;
  }

  // ---- the sort; text, rank[], SA, its first key buffer and the temporary storage stay --------------------------------------
  SsKeep keep;
  DevBuf d_text, d_rank, d_sa, d_k0, d_temp;
  uint64_t n = 0;
  rc = kj_sufsort_device_keep(text, tlen, device_id, nullptr, &n, stats ? &stats->sort : nullptr, &keep, err);
  d_text.p = keep.text; d_rank.p = keep.rank; d_sa.p = keep.sa; d_k0.p = keep.k0; d_temp.p = keep.temp;
  if (rc != KAIJU_GPU_OK) return rc;
  if (n != nsuf || keep.nseq != nseq || !keep.text || !keep.rank || !keep.sa || !keep.k0 || !keep.temp) { err = "internal: index stages on the device: suffix count"; return KAIJU_GPU_ERR_ARG; }
  if (mark) mark("suffix sort");

  DevBuf d_B, d_bwt, d_samples, d_index2, d_pieces, d_starts, d_rank_of, d_ror, d_sl;
  const uint64_t nblk = P.nblk, npieces = P.npieces;
  FB_HIP(d_B.alloc(fb_round_up(tlen, KJ_FB_PAD)));
  if (P.copies > 1) FB_HIP(d_bwt.alloc(fb_round_up(otlen, KJ_FB_PAD)));
  FB_HIP(d_samples.alloc(samples_bytes));
  FB_HIP(d_index2.alloc(2 * (uint64_t)KJ_FB_ALEN * nblk));
  FB_HIP(d_pieces.alloc(4 * (uint64_t)KJ_FB_ALEN * npieces));
  FB_HIP(d_starts.alloc(4 * nseq));
  FB_HIP(d_rank_of.alloc(4 * nseq));
  FB_HIP(d_ror.alloc(4 * nseq));
  FB_HIP(d_sl.alloc(4 * (KJ_FB_ALEN + 1)));
  uint8_t *bwt = P.copies > 1 ? d_bwt.as<uint8_t>() : d_B.as<uint8_t>();
  Events ev;
  for (hipEvent_t &x : ev.e) FB_HIP(hipEventCreate(&x));
  const hipStream_t st = nullptr;
  const uint8_t *T = d_text.as<uint8_t>();
  const uint32_t *SA = d_sa.as<uint32_t>(), *rank = d_rank.as<uint32_t>();

  // ---- BWT of the file ----
  FB_HIP(hipEventRecord(ev.e[0], st));
  FB_HIP(hipMemsetAsync(d_rank_of.p, 0, 4 * nseq, st));
  FB_HIP(hipMemsetAsync(d_ror.p, 0, 4 * nseq, st));
  FB_HIP(hipMemsetAsync(d_starts.p, 0, 4 * nseq, st));
  k_fb_bwt_rows<<<grid_for(nsuf), KJ_FB_THREADS, 0, st>>>(T, SA, nsuf, nseq, d_B.as<uint8_t>());
  FB_HIP(hipGetLastError());
  k_fb_terminators<<<grid_for((tlen + 3) / 4), KJ_FB_THREADS, 0, st>>>(T, rank, tlen, nseq, d_B.as<uint8_t>(), d_starts.as<uint32_t>());
  FB_HIP(hipGetLastError());
  FB_HIP(hipEventRecord(ev.e[1], st));

  // ---- sequence ranks ----
  uint32_t whole = 0;
  if (nsuf) {
    uint32_t *flags = d_k0.as<uint32_t>();                   // 8 nsuf bytes: the flags and, in place, their scan
    k_fb_flags<<<grid_for(nsuf), KJ_FB_THREADS, 0, st>>>(d_B.as<uint8_t>(), nseq, nsuf, flags);
    FB_HIP(hipGetLastError());
    size_t tb = 0;
    FB_HIP(rocprim::inclusive_scan(nullptr, tb, flags, flags, (size_t)nsuf, rocprim::plus<uint32_t>(), st));
    if (tb > keep.temp_bytes) { err = "internal: index stages on the device: temporary storage"; return KAIJU_GPU_ERR_ARG; }
    tb = keep.temp_bytes;
    FB_HIP(rocprim::inclusive_scan(d_temp.p, tb, flags, flags, (size_t)nsuf, rocprim::plus<uint32_t>(), st));
    k_fb_seq_ranks<<<grid_for(nsuf), KJ_FB_THREADS, 0, st>>>(d_B.as<uint8_t>(), SA, rank, flags, nsuf, nseq, r0, d_ror.as<uint32_t>(), d_rank_of.as<uint32_t>());
    FB_HIP(hipGetLastError());
    FB_HIP(hipMemcpyAsync(&whole, flags + (nsuf - 1), 4, hipMemcpyDeviceToHost, st));
  }
  FB_HIP(hipEventRecord(ev.e[2], st));
  FB_HIP(hipStreamSynchronize(st));
  if (r0 + whole != nseq) { err = "internal: sequence ranks"; return KAIJU_GPU_ERR_ARG; }

  // ---- replication and samples ----
  if (P.copies > 1) {
    k_fb_replicate<<<grid_for((otlen + KJ_FB_REP_BYTES - 1) / KJ_FB_REP_BYTES), KJ_FB_THREADS, 0, st>>>(d_B.as<uint8_t>(), otlen, P.copies, d_bwt.as<uint64_t>());
    FB_HIP(hipGetLastError());
  }
  FB_HIP(hipMemsetAsync(d_samples.p, 0, samples_bytes ? samples_bytes : 1, st));
  if (P.nfill) {
    k_fb_samples<<<grid_for(P.nfill), KJ_FB_THREADS, 0, st>>>(P, SA, d_starts.as<uint32_t>(), d_rank_of.as<uint32_t>(), d_samples.as<uint8_t>());
    FB_HIP(hipGetLastError());
  }
  FB_HIP(hipEventRecord(ev.e[3], st));

  // ---- checkpoints; index2's rows and the piece counts down; the host's sums and code table; 22 ints up ----
  if (npieces > 0x7fffffffull) { err = "internal: index stages on the device: pieces"; return KAIJU_GPU_ERR_ARG; }
  k_fb_checkpoints<<<(unsigned)npieces, KJ_FB_THREADS, 0, st>>>(bwt, otlen, d_index2.as<uint16_t>(), d_pieces.as<uint32_t>());
  FB_HIP(hipGetLastError());
  FB_HIP(hipEventRecord(ev.e[4], st));
  FB_HIP(hipMemcpyAsync(out.index2, d_index2.p, 2 * (uint64_t)KJ_FB_ALEN * nblk, hipMemcpyDeviceToHost, st));
  FB_HIP(hipMemcpyAsync(out.piece_counts, d_pieces.p, 4 * (uint64_t)KJ_FB_ALEN * npieces, hipMemcpyDeviceToHost, st));
  FB_HIP(hipEventRecord(ev.e[5], st));
  FB_HIP(hipStreamSynchronize(st));
  int sl[KJ_FB_ALEN + 1] = {0};
  finish(out.piece_counts, sl);
  for (int a = 0; a < KJ_FB_ALEN; a++)
    if (sl[a] < 0 || sl[a + 1] <= sl[a] || sl[a + 1] > 256) { err = "internal: index stages on the device: code table"; return KAIJU_GPU_ERR_ARG; }

  // ---- byte coding ----
  FB_HIP(hipMemcpyAsync(d_sl.p, sl, sizeof sl, hipMemcpyHostToDevice, st));
  FB_HIP(hipEventRecord(ev.e[6], st));
  if (recode) {
    const uint64_t groups = (nblk + KJ_FB_THREADS / 64 - 1) / (KJ_FB_THREADS / 64);
    if (groups > 0x7fffffffull) { err = "internal: index stages on the device: blocks"; return KAIJU_GPU_ERR_ARG; }
    k_fb_recode<<<(unsigned)groups, KJ_FB_THREADS, 0, st>>>(reinterpret_cast<uint32_t *>(bwt), otlen, nblk, d_sl.as<int>());
    FB_HIP(hipGetLastError());
  }
  FB_HIP(hipEventRecord(ev.e[7], st));

  // ---- what the file is written from comes down; SA does not ----
  if (nseq > r0) FB_HIP(hipMemcpyAsync(out.read_of_rank + r0, d_ror.as<uint32_t>() + r0, 4 * (nseq - r0), hipMemcpyDeviceToHost, st));
  if (samples_bytes) FB_HIP(hipMemcpyAsync(out.samples, d_samples.p, samples_bytes, hipMemcpyDeviceToHost, st));
  FB_HIP(hipMemcpyAsync(out.bwt, bwt, otlen, hipMemcpyDeviceToHost, st));
  FB_HIP(hipEventRecord(ev.e[8], st));
  FB_HIP(hipStreamSynchronize(st));
  if (stats) {
    float d1 = 0.f, d2 = 0.f;
    FB_HIP(hipEventElapsedTime(&stats->ms_bwt, ev.e[0], ev.e[1]));
    FB_HIP(hipEventElapsedTime(&stats->ms_ranks, ev.e[1], ev.e[2]));
    FB_HIP(hipEventElapsedTime(&stats->ms_samples, ev.e[2], ev.e[3]));
    FB_HIP(hipEventElapsedTime(&stats->ms_checkpoints, ev.e[3], ev.e[4]));
    FB_HIP(hipEventElapsedTime(&d1, ev.e[4], ev.e[5]));
    FB_HIP(hipEventElapsedTime(&stats->ms_recode, ev.e[6], ev.e[7]));
    FB_HIP(hipEventElapsedTime(&d2, ev.e[7], ev.e[8]));
    stats->ms_download = d1 + d2;
    stats->device_stages = KJ_FB_STAGE_BWT | KJ_FB_STAGE_RANKS | KJ_FB_STAGE_SAMPLES | KJ_FB_STAGE_CHECKPOINTS | (recode ? KJ_FB_STAGE_RECODE : 0);
  }
  return KAIJU_GPU_OK;
}
