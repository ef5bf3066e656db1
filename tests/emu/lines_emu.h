// lines_emu.h — what the emulations of ingest.hip and of the four formatters share: the order in which the units of a pass run,
// and the skeleton of kaiju_amd/csrc/kj_lines.h restated in plain C++ (nothing of that header is called here): the prefix
// sum in its three steps, and the blocks and lanes of the write pass.  What a block of the device does with a wavefront scan
// is a loop here.  The units of every step run in the order the caller asks for: no step may depend on it.
#ifndef LINES_EMU_H
#define LINES_EMU_H

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <random>
#include <vector>

namespace emu {

// mode: 0 forward, 1 reversed, 2 shuffled (rng)
struct Order {
  int mode; std::mt19937 rng;
  std::vector<uint64_t> units(uint64_t n) {
    std::vector<uint64_t> v(n);
    std::iota(v.begin(), v.end(), 0);
    if (mode == 1) std::reverse(v.begin(), v.end());
    if (mode == 2) std::shuffle(v.begin(), v.end(), rng);
    return v;
  }
};

// off[i] = len[0] + .. + len[i - 1] for i <= M, in blocks of `block` elements
template <class Len>
void scan_offsets(Order &o, const Len *len, uint64_t M, uint64_t block, uint64_t *off) {
  const uint64_t nb = (M + block - 1) / block;
  std::vector<uint64_t> blk(nb + 1, 0), base(nb + 1, 0);
  for (uint64_t b : o.units(nb)) {                                            // kjl::k_scan_sums
    uint64_t t = 0;
    for (uint64_t i = b * block; i < std::min(M, (b + 1) * block); i++) t += len[i];
    blk[b] = t;
  }
  uint64_t carry = 0;                                                         // kjl::k_scan_top
  for (uint64_t b = 0; b < nb; b++) { base[b] = carry; carry += blk[b]; }
  off[M] = carry;
  for (uint64_t b : o.units(nb)) {                                            // kjl::k_scan_apply
    uint64_t t = base[b];
    for (uint64_t i = b * block; i < std::min(M, (b + 1) * block); i++) { off[i] = t; t += len[i]; }
  }
}

#ifdef KJ_FORMAT_H
// kjl::write_blocks: the blocks of the output and the lanes of a block.  out: 16-byte aligned, out_cap bytes;
// chunk(c, lo, hi, total, &v) as on the device
template <class F>
void write_blocks(Order &o, const uint64_t *line_off, uint32_t n, uint8_t *out, uint64_t out_cap, F chunk) {
  const uint64_t total = line_off[n], lim = std::min(total, out_cap), nb = (lim + kjf::kBlockBytes - 1) / kjf::kBlockBytes;
  for (uint64_t b : o.units(nb)) {
    uint32_t lo, hi;
    kjf::block_records(line_off, n, b, lim, &lo, &hi);
    for (uint64_t l : o.units(kjf::kBlockLanes)) {
      const uint64_t c = b * kjf::kBlockLanes + l;
      if (c * kjf::kChunk >= lim) continue;
      kjf::Chunk v;
      const uint32_t m = chunk(c, lo, hi, total, &v);
      if (m) kjf::store_chunk(out, c, v, m);
    }
  }
}
#endif

}  // namespace emu

#endif  // LINES_EMU_H
