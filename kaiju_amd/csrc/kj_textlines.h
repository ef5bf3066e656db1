// kj_textlines.h — the line pass of kj_ingest.h as kernels, for the files that need nothing else of a text (accmap.hip,
// convert.hip; device side only).  The kernels live in the including file's anonymous namespace: every code object holds its own.
//   k_tl_count   '\n' per tile            k_tl_top    prefix sum over the tiles, one block
//   k_tl_fill    line_start[]             k_tl_plan   by one lane: the number of lines, line_start[0] and the sentinel
// Line i is text[line_start[i], line_start[i + 1] - 1).
#ifndef KJ_TEXTLINES_H
#define KJ_TEXTLINES_H

#include <hip/hip_runtime.h>

#include "kj_ingest.h"
#include "kj_lines.h"
#include "kj_scan.h"

namespace {

constexpr int kTlBlock = 256;
static_assert(kTlBlock == (int)kji::kTileLanes && kTlBlock == kjs::kScanLanes, "one lane per chunk of a tile / element of a scan block");

struct TlText {
  const uint8_t *text;
  uint64_t bytes;
  uint32_t n_tiles;
  uint32_t *tile_cnt, *tile_base;      // n_tiles + 1
  uint32_t *line_start;                // bytes + 2
  uint32_t *n_lines;                   // one
};

inline void tl_carve(kjl::Carver &c, TlText &X) {
  X.n_tiles = (uint32_t)((X.bytes + kji::kTileBytes - 1) / kji::kTileBytes);
  X.tile_cnt = c.take<uint32_t>((size_t)X.n_tiles + 1);
  X.tile_base = c.take<uint32_t>((size_t)X.n_tiles + 1);
  X.line_start = c.take<uint32_t>(X.bytes + 2);
  X.n_lines = c.take<uint32_t>(1);
}

__global__ __launch_bounds__(kTlBlock) void k_tl_count(TlText X) {
  const uint64_t c = (uint64_t)blockIdx.x * kji::kTileLanes + threadIdx.x;
  uint32_t tot;
  kjs::block_scan_excl<uint32_t>(kji::popc16(kji::nl_mask(X.text, X.bytes, c)), 0u, &tot, kjs::OpAdd32());
  if (threadIdx.x == 0) X.tile_cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kTlBlock) void k_tl_top(const uint32_t *in, uint32_t *out, uint32_t n) {
  uint32_t carry = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kTlBlock) {
    const uint32_t i = i0 + threadIdx.x;
    uint32_t tot;
    const uint32_t ex = kjs::block_scan_excl<uint32_t>(i < n ? in[i] : 0u, 0u, &tot, kjs::OpAdd32());
    if (i < n) out[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) out[n] = carry;
}

__global__ __launch_bounds__(kTlBlock) void k_tl_fill(TlText X) {
  const uint64_t c = (uint64_t)blockIdx.x * kji::kTileLanes + threadIdx.x;
  const uint32_t m = kji::nl_mask(X.text, X.bytes, c);
  uint32_t tot;
  const uint32_t ex = kjs::block_scan_excl<uint32_t>(kji::popc16(m), 0u, &tot, kjs::OpAdd32());
  uint32_t j = X.tile_base[blockIdx.x] + ex;                       // the line that ends at the next '\n'
  for (uint32_t mm = m; mm; mm &= mm - 1, j++) X.line_start[j + 1] = (uint32_t)(c * kji::kChunk + kji::ctz16(mm) + 1);
}

__global__ void k_tl_plan(TlText X) {
  if (blockIdx.x || threadIdx.x) return;
  X.line_start[0] = 0;
  uint32_t sentinel;
  const uint32_t n = kji::line_count(X.text, X.bytes, X.tile_base[X.n_tiles], &sentinel);
  X.line_start[n] = sentinel;
  *X.n_lines = n;
}

inline void tl_launch(hipStream_t s, const TlText &X) {
  const dim3 blk(kTlBlock);
  if (X.n_tiles) hipLaunchKernelGGL(k_tl_count, dim3(X.n_tiles), blk, 0, s, X);
  hipLaunchKernelGGL(k_tl_top, dim3(1), blk, 0, s, static_cast<const uint32_t *>(X.tile_cnt), X.tile_base, X.n_tiles);
  if (X.n_tiles) hipLaunchKernelGGL(k_tl_fill, dim3(X.n_tiles), blk, 0, s, X);
  hipLaunchKernelGGL(k_tl_plan, dim3(1), dim3(64), 0, s, X);
}

}  // namespace

#endif  // KJ_TEXTLINES_H
