// kj_lines.h — the skeleton the pipelines "lengths per record in, bytes out" share (ingest.hip, format.hip, format_names.hip,
// format_verbose.hip, format_seq.hip; device and its host side only):
//   k_scan_sums / k_scan_top / k_scan_apply   the exclusive prefix sum over more elements than one block, on the block scan of
//                       kj_scan.h: 64-bit offsets of 32- or 64-bit lengths, the total at off[M].  M is known on the device
//                       only and comes from a functor of the caller
//   write_blocks        the output-centric write loop: per lane 16 aligned bytes of the output, whole lines of memory per
//                       wavefront; what the 16 bytes are is the caller's
//   Carver / Scratch / Lines   device scratch that grows on demand and is carved into arrays
// Every kernel here is a template over a type of the including file's anonymous namespace (its count functor), so every code
// object of the library holds instantiations of its own, under names of its own.
#ifndef KJ_LINES_H
#define KJ_LINES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kaiju_gpu.h"
#include "kj_format.h"
#include "kj_scan.h"

namespace kjl {

using kjs::kScanLanes;

// ---- off[i] = len[0] + .. + len[i - 1] for i <= M = count() ------------------------------------------------------------
// the sum of every block of kScanLanes elements
template <class Count, class Len>
__global__ __launch_bounds__(kScanLanes) void k_scan_sums(Count count, const Len *len, uint64_t *blk) {
  const uint64_t M = count(), nb = (M + kScanLanes - 1) / kScanLanes;
  for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t i = b * kScanLanes + threadIdx.x;
    uint64_t tot;
    kjs::block_scan_excl<uint64_t>(i < M ? len[i] : 0ull, 0ull, &tot, kjs::OpAdd64());
    if (threadIdx.x == 0) blk[b] = tot;
  }
}

// one block walks those sums kScanLanes at a time: the base of every block, and the total
template <class Count>
__global__ __launch_bounds__(kScanLanes) void k_scan_top(Count count, const uint64_t *blk, uint64_t *blk_base, uint64_t *off) {
  const uint64_t M = count(), nb = (M + kScanLanes - 1) / kScanLanes;
  uint64_t carry = 0;
  for (uint64_t i0 = 0; i0 < nb; i0 += kScanLanes) {
    const uint64_t i = i0 + threadIdx.x;
    uint64_t tot;
    const uint64_t ex = kjs::block_scan_excl<uint64_t>(i < nb ? blk[i] : 0ull, 0ull, &tot, kjs::OpAdd64());
    if (i < nb) blk_base[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) off[M] = carry;
}

// the base of its block added to the scan inside the block
template <class Count, class Len>
__global__ __launch_bounds__(kScanLanes) void k_scan_apply(Count count, const Len *len, const uint64_t *blk_base, uint64_t *off) {
  const uint64_t M = count(), nb = (M + kScanLanes - 1) / kScanLanes;
  for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t i = b * kScanLanes + threadIdx.x;
    uint64_t tot;
    const uint64_t ex = kjs::block_scan_excl<uint64_t>(i < M ? len[i] : 0ull, 0ull, &tot, kjs::OpAdd64());
    if (i < M) off[i] = blk_base[b] + ex;
  }
}

// the three of them behind each other on stream s.  grid: blocks of sums and apply (both grid-stride over the blocks of len[])
template <class Count, class Len>
void launch_offsets(hipStream_t s, dim3 grid, Count count, const Len *len, uint64_t *blk, uint64_t *blk_base, uint64_t *off) {
  hipLaunchKernelGGL((k_scan_sums<Count, Len>), grid, dim3(kScanLanes), 0, s, count, len, blk);
  hipLaunchKernelGGL((k_scan_top<Count>), dim3(1), dim3(kScanLanes), 0, s, count, static_cast<const uint64_t *>(blk), blk_base, off);
  hipLaunchKernelGGL((k_scan_apply<Count, Len>), grid, dim3(kScanLanes), 0, s, count, len, static_cast<const uint64_t *>(blk_base), off);
}

// ---- the write pass ----------------------------------------------------------------------------------------------------
// Blocks of kBlockLanes lanes, grid-stride over the blocks of kBlockBytes bytes of the output: lane 0 narrows the search to
// the records the block's bytes touch, then every lane makes and stores its chunk.  chunk(c, lo, hi, total, &v): the bytes of
// chunk c of a text of `total` bytes into v, the mask of those to write as the result.
template <class F>
__device__ __forceinline__ void write_blocks(const uint64_t *line_off, uint32_t n, uint8_t *out, uint64_t out_cap, F chunk) {
  __shared__ uint32_t s_lo, s_hi;
  const uint64_t total = line_off[n];
  const uint64_t lim = total < out_cap ? total : out_cap;              // no line reaches beyond it
  const uint64_t nb = (lim + kjf::kBlockBytes - 1) / kjf::kBlockBytes;
  for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    if (threadIdx.x == 0) {
      uint32_t lo, hi;
      kjf::block_records(line_off, n, b, lim, &lo, &hi);
      s_lo = lo; s_hi = hi;
    }
    __syncthreads();
    const uint32_t lo = s_lo, hi = s_hi;
    const uint64_t c = b * kjf::kBlockLanes + threadIdx.x;
    if (c * kjf::kChunk < lim) {
      kjf::Chunk v;
      const uint32_t m = chunk(c, lo, hi, total, &v);
      if (m) kjf::store_chunk(out, c, v, m);
    }
    __syncthreads();
  }
}

// ---- host side: scratch ------------------------------------------------------------------------------------------------
// arrays behind each other in one allocation, 256-byte aligned.  base == nullptr: only measures
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

struct Scratch {
  void *p = nullptr;
  size_t cap = 0;
  // room for bytes + margin: grows only when too small, then with an eighth of headroom.  what: the message of a failed
  // hipMalloc.  Returns 0, or a kaiju_gpu_status with *err set
  int reserve(size_t bytes, size_t margin, const char *what, const char **err) {
    if (bytes + margin <= cap) return KAIJU_GPU_OK;
    // (the passes of an earlier call on another stream may still use the old memory)
    if (p) { if (hipDeviceSynchronize() != hipSuccess || hipFree(p) != hipSuccess) { *err = "hipFree"; return KAIJU_GPU_ERR_HIP; } p = nullptr; cap = 0; }
    const size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); *err = what; return KAIJU_GPU_ERR_NOMEM; }
    cap = want;
    return KAIJU_GPU_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// what a formatter keeps between calls
struct Lines {
  Scratch mem;                         // the carved arrays
  Scratch shadow;                      // the shadow of the output (verbose and sequence lines)
  const uint64_t *total = nullptr;     // device addresses of the last call: the size of the whole text (line_off[n]) ...
  const uint64_t *written = nullptr;   // ... and the bytes written (= the size unless it overflowed)
  void release() { mem.release(); shadow.release(); total = written = nullptr; }
};

}  // namespace kjl

#endif  // KJ_LINES_H
