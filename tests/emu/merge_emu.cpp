// merge_emu.cpp — the passes of kaiju_amd/csrc/merge.hip on the host: the per-lane functions of kj_merge.h (and the line pass
// of kj_ingest.h), driven work unit by work unit as tests/emu/annotate_emu.cpp does for kj_annotate.h.  The units of a pass
// run in the order the caller asks for (forward, reversed, shuffled): no pass may depend on it.  It is compiled together with
// kaiju_amd/csrc/taxonomy.cpp, whose loader and table (kj_taxonomy_table: the arrays the library uploads) it uses.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_merge.h"
#include "../../kaiju_amd/csrc/taxonomy.h"
#include "lines_emu.h"

using namespace kjm;
using emu::Order;

namespace {

// the text as the device sees it: 16-byte aligned, readable to the next multiple of 16 and not one byte further
uint8_t *device_text(const uint8_t *in, uint64_t bytes) {
  const uint64_t padded = std::max<uint64_t>((bytes + kChunk - 1) / kChunk * kChunk, kChunk);
  void *mem = nullptr;
  if (posix_memalign(&mem, kChunk, padded) != 0) return nullptr;
  memset(mem, 0x5a, padded);
  if (bytes) memcpy(mem, in, bytes);
  return static_cast<uint8_t *>(mem);
}

// k_mg_lines_count / k_mg_top / k_mg_lines_fill; returns the number of '\n'
uint32_t lines(Order &o, const uint8_t *text, uint64_t bytes, std::vector<uint32_t> &line_start) {
  const uint32_t n_tiles = (uint32_t)((bytes + kji::kTileBytes - 1) / kji::kTileBytes);
  std::vector<uint32_t> tile_cnt((size_t)n_tiles + 1, 0xdeadbeefu), tile_base((size_t)n_tiles + 1, 0xdeadbeefu);
  line_start.assign(bytes + 2, 0xdeadbeefu);
  for (uint64_t t : o.units(n_tiles)) {
    uint32_t cnt = 0;
    for (uint64_t l : o.units(kji::kTileLanes)) cnt += kji::popc16(kji::nl_mask(text, bytes, t * kji::kTileLanes + l));
    tile_cnt[t] = cnt;
  }
  uint32_t carry = 0;
  for (uint32_t t = 0; t < n_tiles; t++) { tile_base[t] = carry; carry += tile_cnt[t]; }
  tile_base[n_tiles] = carry;
  for (uint64_t t : o.units(n_tiles)) {
    std::vector<uint32_t> ex(kji::kTileLanes);
    uint32_t run = 0;
    for (uint32_t l = 0; l < kji::kTileLanes; l++) { ex[l] = run; run += kji::popc16(kji::nl_mask(text, bytes, t * kji::kTileLanes + l)); }
    for (uint64_t l : o.units(kji::kTileLanes)) {
      const uint64_t c = t * kji::kTileLanes + l;
      uint32_t j = tile_base[t] + ex[l];
      for (uint32_t mm = kji::nl_mask(text, bytes, c); mm; mm &= mm - 1, j++) line_start[j + 1] = (uint32_t)(c * kChunk + kji::ctz16(mm) + 1);
    }
  }
  return tile_base[n_tiles];
}

}  // namespace

extern "C" void merge_emu_constants(uint32_t *out) { out[0] = kjf::kBlockBytes; out[1] = kjf::kScanBlock; out[2] = kChunk; out[3] = kji::kTileBytes; out[4] = sizeof(Rec); }
extern "C" uint64_t merge_emu_bound(uint64_t bytes1, uint64_t bytes2) { return bound(bytes1, bytes2); }

// score text -> kind, exponent, mantissa (for the test of the decimal comparison)
extern "C" int merge_emu_score(const uint8_t *s, uint32_t n, int32_t *exp, uint64_t *mant) {
  const Score v = score_value(s, 0, n);
  *exp = v.exp; *mant = v.mant;
  return (int)v.kind;
}
extern "C" int merge_emu_score_cmp(const uint8_t *a, uint32_t na, const uint8_t *b, uint32_t nb) { return score_cmp(score_value(a, 0, na), score_value(b, 0, nb)); }

// tax: kaiju_taxonomy_load's tree or NULL.  info: kaiju_gpu_merge_info.  out: out_cap bytes, changed only where lines are written.
// order: 0 forward, 1 reversed, 2 shuffled (seed)
extern "C" int merge_emu(const uint8_t *in1, uint64_t bytes1, const uint8_t *in2, uint64_t bytes2, const kaiju_taxonomy *tax, int mode, int use_score, int final,
                         uint8_t *out, uint64_t out_cap, kaiju_gpu_merge_info *info, int order, uint32_t seed) {
  if (bytes1 > kji::kMaxBytes || bytes2 > kji::kMaxBytes || (mode == kModeLca && !tax)) return -1;
  Order o{order, std::mt19937(seed)};
  std::vector<uint64_t> key, parent_id;
  std::vector<uint32_t> parent_slot, depth;
  Tree T{};
  if (tax) {
    kj_taxonomy_table(tax, key, parent_id, parent_slot, depth);
    T = Tree{key.data(), parent_slot.data(), depth.data(), (uint32_t)(key.size() - 1)};
  }
  uint8_t *text[2] = {device_text(in1, bytes1), device_text(in2, bytes2)};
  const uint64_t bytes[2] = {bytes1, bytes2};
  if (!text[0] || !text[1]) return -6;

  // ---- lines, plan (k_mg_plan) ----
  std::vector<uint32_t> ls[2];
  uint32_t n[2];
  for (int k = 0; k < 2; k++) {
    const uint32_t n_nl = lines(o, text[k], bytes[k], ls[k]);
    ls[k][0] = 0;
    uint32_t sentinel;
    n[k] = merge_line_count(text[k], bytes[k], n_nl, ls[k][n_nl], final, &sentinel);
    ls[k][n[k]] = sentinel;
  }
  const uint32_t n_pairs = std::min(n[0], n[1]), n_look = pairs_looked_at(n[0], n[1], final, bytes1, bytes2);
  const uint64_t used1 = final ? bytes1 : ls[0][n_pairs], used2 = final ? bytes2 : ls[1][n_pairs];
  const uint32_t more_in_2 = final && n[1] > n[0] && kji::line_len(ls[1].data(), n[0]) != 0 ? 1u : 0u;

  // ---- pair (k_mg_pair) ----
  const size_t cap = pair_cap(bytes1, bytes2);
  if (n_look > cap) return -9;
  std::vector<Rec> rec(cap);
  memset(rec.data(), 0xa7, cap * sizeof(Rec));
  uint32_t stop = kNoStop;
  for (uint64_t r64 : o.units(n_look)) {
    const uint32_t r = (uint32_t)r64;
    const bool have2 = r < n[1];
    rec[r] = resolve_pair(text[0], ls[0][r], (uint64_t)ls[0][r + 1] - 1, text[1], have2 ? ls[1][r] : 0, have2 ? (uint64_t)ls[1][r + 1] - 1 : 0, have2, T, mode, use_score);
    if (rec_why(rec[r])) stop = std::min(stop, r);
  }

  // ---- count (k_mg_count), offsets ----
  const uint32_t n_out = std::min(n_look, stop);
  std::vector<uint64_t> olen(cap, 0xdeadbeefdeadbeefull), out_off(cap + 1, 0xdeadbeefdeadbeefull);
  uint32_t count[kKindCount] = {0, 0, 0, 0};
  for (uint64_t r : o.units(n_out)) { olen[r] = rec_olen(rec[r]); count[rec_kind(rec[r])]++; }
  emu::scan_offsets(o, olen.data(), n_out, kjf::kScanBlock, out_off.data());
  const uint64_t total = out_off[n_out];

  // ---- write (k_mg_write) ----
  void *mem = nullptr;
  if (posix_memalign(&mem, kChunk, std::max<uint64_t>(out_cap, 1)) != 0) return -6;
  uint8_t *dev_out = static_cast<uint8_t *>(mem);
  if (out_cap) memcpy(dev_out, out, out_cap);
  emu::write_blocks(o, out_off.data(), n_out, dev_out, out_cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t tot, Chunk *v) {
    return merge_chunk(c, text[0], text[1], rec.data(), out_off.data(), lo, hi, tot, out_cap, v);
  });
  if (out_cap) memcpy(out, dev_out, out_cap);
  free(mem);
  *info = make_info(total, used1, used2, n[0], n[1], n_out, stop, stop != kNoStop ? rec_why(rec[stop]) : 0u, count, more_in_2, out_cap);   // k_mg_finish
  free(text[0]);
  free(text[1]);
  return 0;
}
