// kj_scan.h — the block scan the passes of ingest.hip and of the formatters are built on (device only): an exclusive scan over
// the 256 lanes of a block in lane order, for any associative operator (ingest.hip scans the transition functions of its FASTQ
// state machine with it).  The prefix sum over more elements than one block - three kernels on top of it - is in kj_lines.h.
#ifndef KJ_SCAN_H
#define KJ_SCAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kjs {

constexpr int kScanLanes = 256;

struct OpAdd32 { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct OpAdd64 { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; } };

// exclusive scan over the 256 lanes of a block in lane order (op need not commute); *total = all of them
template <class T, class Op>
__device__ T block_scan_excl(T v, T ident, T *total, Op op) {
  __shared__ T wtot[kScanLanes / 64];
  const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
  T x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d, 64);
    if (lane >= d) x = op(y, x);
  }
  const T up = __shfl_up(x, 1, 64);
  if (lane == 63) wtot[w] = x;
  __syncthreads();
  T pre = ident, tot = ident;
#pragma unroll
  for (int k = 0; k < kScanLanes / 64; k++) { if (k < w) pre = op(pre, wtot[k]); tot = op(tot, wtot[k]); }
  __syncthreads();
  *total = tot;
  return lane ? op(pre, up) : pre;
}

}  // namespace kjs

#endif  // KJ_SCAN_H
