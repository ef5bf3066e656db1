// format.hip — 16-byte records to the lines of the output file (gfx950, wave64): the passes of kj_format.h as kernels.  The
// size of the text is known on the device only, so every kernel behind the first sizes itself from counts in device memory
// (grid-stride over records / blocks of output) and nothing waits for the host.
//
//   k_fmt_len           per record: the decision (the taxon to print), the length of the line; counts of 'C' lines and of
//                       records flagged inexact; the header of the call
//   k_fmt_off_sums / k_fmt_off_top / k_fmt_off_apply   line_off[] = prefix sum of the lengths (64 bit)
//   k_fmt_write         per lane 16 aligned bytes of the output, whole lines of memory per wavefront
//   k_fmt_finish        kaiju_gpu_format_info, by one lane with ordinary stores
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "../../include/kaiju_gpu.h"
#include "kj_format.h"
#include "kj_scan.h"

using namespace kjf;
using kjs::OpAdd64;
using kjs::block_scan_excl;

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

__global__ __launch_bounds__(kFmtBlock) void k_fmt_off_sums(FmtJob J) {
  const uint64_t M = J.hdr->n, nb = (M + kScanBlock - 1) / kScanBlock;
  for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t i = b * kScanBlock + threadIdx.x;
    uint64_t tot;
    block_scan_excl<uint64_t>(i < M ? J.llen[i] : 0ull, 0ull, &tot, OpAdd64());
    if (threadIdx.x == 0) J.oblk[b] = tot;
  }
}

__global__ __launch_bounds__(kFmtBlock) void k_fmt_off_top(FmtJob J) {
  const uint64_t M = J.hdr->n, nb = (M + kScanBlock - 1) / kScanBlock;
  uint64_t carry = 0;
  for (uint64_t i0 = 0; i0 < nb; i0 += kFmtBlock) {
    const uint64_t i = i0 + threadIdx.x;
    uint64_t tot;
    const uint64_t ex = block_scan_excl<uint64_t>(i < nb ? J.oblk[i] : 0ull, 0ull, &tot, OpAdd64());
    if (i < nb) J.oblk_base[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) J.line_off[M] = carry;
}

__global__ __launch_bounds__(kFmtBlock) void k_fmt_off_apply(FmtJob J) {
  const uint64_t M = J.hdr->n, nb = (M + kScanBlock - 1) / kScanBlock;
  for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t i = b * kScanBlock + threadIdx.x;
    uint64_t tot;
    const uint64_t ex = block_scan_excl<uint64_t>(i < M ? J.llen[i] : 0ull, 0ull, &tot, OpAdd64());
    if (i < M) J.line_off[i] = J.oblk_base[b] + ex;
  }
}

__global__ __launch_bounds__(kFmtBlock) void k_fmt_write(FmtJob J) {
  __shared__ uint32_t s_lo, s_hi;
  const uint32_t n = J.hdr->n;
  const uint64_t total = J.line_off[n];
  const uint64_t lim = total < J.out_cap ? total : J.out_cap;          // no line reaches beyond it
  const uint64_t nb = (lim + kBlockBytes - 1) / kBlockBytes;
  for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    if (threadIdx.x == 0) {
      uint32_t lo, hi;
      block_records(J.line_off, n, b, lim, &lo, &hi);
      s_lo = lo; s_hi = hi;
    }
    __syncthreads();
    const uint32_t lo = s_lo, hi = s_hi;
    const uint64_t c = b * kBlockLanes + threadIdx.x;
    if (c * kChunk < lim) {
      Chunk v;
      const uint32_t m = format_chunk(c, J.text, J.bytes1, J.names, J.line_off, J.tax, lo, hi, total, J.out_cap, &v);
      if (m) store_chunk(J.out, c, v, m);
    }
    __syncthreads();
  }
}

__global__ void k_fmt_finish(FmtJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t n = J.hdr->n;
  const uint64_t total = J.line_off[n];
  // the lines that fit: line_off[0 .. k] with line_off[k] <= out_cap
  J.hdr->written = total <= J.out_cap ? total : J.line_off[find_record(J.line_off, 0, n + 1, J.out_cap)];
  *J.info = make_info(total, n, J.hdr->n_classified, J.hdr->n_inexact, J.out_cap);
}

}  // namespace

// ---- host side: scratch and the queue of passes ----------------------------------------------------------------------
struct kj_format_scratch {
  void *p = nullptr;
  size_t cap = 0;
  const uint64_t *written = nullptr;
};

void kj_format_free(kj_format_scratch *s) {
  if (!s) return;
  if (s->p) (void)hipFree(s->p);
  delete s;
}
const uint64_t *kj_format_written(const kj_format_scratch *s) { return s ? s->written : nullptr; }

namespace {
struct Carver {
  uint8_t *base;
  size_t at = 0;
  template <class T> T *take(size_t n) {
    at = (at + 255) & ~(size_t)255;
    T *q = base ? reinterpret_cast<T *>(base + at) : nullptr;
    at += n * sizeof(T);
    return q;
  }
};
void carve(Carver &c, FmtJob &J, uint32_t n) {
  const size_t nblk = (size_t)n / kScanBlock + 2;
  J.llen = c.take<uint32_t>((size_t)n + 1);
  J.line_off = c.take<uint64_t>((size_t)n + 1);
  J.tax = c.take<uint64_t>((size_t)n + 1);
  J.oblk = c.take<uint64_t>(nblk);
  J.oblk_base = c.take<uint64_t>(nblk + 1);
  J.hdr = c.take<FmtHdr>(1);
}
}  // namespace

int kj_format_launch(kj_format_scratch **scratch, hipStream_t s, const Params &P, const double *d_pw, const kaiju_gpu_compact *d_recs,
                     const uint64_t *d_off, uint32_t n, const void *d_text1, uint64_t bytes1, const kaiju_gpu_name_span *d_names,
                     void *d_out, uint64_t out_cap, kaiju_gpu_format_info *d_info, const char **err) {
  *err = "";
  if (!scratch || !d_info || !d_pw || (n && (!d_recs || !d_off || !d_names)) || (!d_text1 && bytes1) || (!d_out && out_cap)) {
    *err = "NULL argument";
    return KAIJU_GPU_ERR_ARG;
  }
  if (bytes1 > kMaxBytes || n > kMaxRecords) { *err = "a block of text must be below 2^32 - 32 bytes, a batch below 2^31 records"; return KAIJU_GPU_ERR_ARG; }
  if ((uintptr_t)d_out & (kChunk - 1)) { *err = "the output pointer must be 16-byte aligned"; return KAIJU_GPU_ERR_ARG; }
  FmtJob J{};
  Carver measure{nullptr};
  carve(measure, J, n);
  if (!*scratch) { *scratch = new (std::nothrow) kj_format_scratch(); if (!*scratch) { *err = "out of host memory"; return KAIJU_GPU_ERR_NOMEM; } }
  kj_format_scratch *sc = *scratch;
  if (measure.at + 256 > sc->cap) {
    // (the passes of an earlier call on another stream may still use the old scratch)
    if (sc->p) { if (hipDeviceSynchronize() != hipSuccess || hipFree(sc->p) != hipSuccess) { *err = "hipFree"; return KAIJU_GPU_ERR_HIP; } sc->p = nullptr; sc->cap = 0; }
    const size_t want = measure.at + measure.at / 8 + 256;
    if (hipMalloc(&sc->p, want) != hipSuccess) { (void)hipGetLastError(); *err = "hipMalloc of the format scratch"; return KAIJU_GPU_ERR_NOMEM; }
    sc->cap = want;
  }
  Carver c{static_cast<uint8_t *>(sc->p)};
  carve(c, J, n);
  sc->written = &J.hdr->written;
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
  hipLaunchKernelGGL(k_fmt_off_sums, ogrid, blk, 0, s, J);
  hipLaunchKernelGGL(k_fmt_off_top, dim3(1), blk, 0, s, J);
  hipLaunchKernelGGL(k_fmt_off_apply, ogrid, blk, 0, s, J);
  hipLaunchKernelGGL(k_fmt_write, wgrid, blk, 0, s, J);
  hipLaunchKernelGGL(k_fmt_finish, dim3(1), dim3(64), 0, s, J);
  if (hipGetLastError() != hipSuccess) { *err = "a kernel of the format passes could not be launched"; return KAIJU_GPU_ERR_HIP; }
  return KAIJU_GPU_OK;
}
