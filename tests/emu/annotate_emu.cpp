// annotate_emu.cpp — the passes of kaiju_amd/csrc/annotate.hip on the host: the per-lane functions of kj_annotate.h (and the
// line pass of kj_ingest.h), driven work unit by work unit as tests/emu/format_names_emu.cpp does for kj_format_names.h.  The
// units of a pass run in the order the caller asks for (forward, reversed, shuffled): no pass may depend on it.  It is
// compiled together with kaiju_amd/csrc/taxon_names.cpp, whose tables it reads; the tables of the upload are built here by
// the same functions, one slot at a time.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_annotate.h"
#include "../../kaiju_amd/csrc/taxon_names.h"
#include "lines_emu.h"

using namespace kja;
using emu::Order;

namespace {

struct Built {
  Tab T{};
  std::vector<uint32_t> path_len, rank_src, rank_len;
  uint64_t max_annotation = 0;
};

// k_fn_tables
void build(const kaiju_taxon_names &N, Built &B) {
  Tab &T = B.T;
  const uint32_t cap = (uint32_t)N.key.size();
  T.key = N.key.data(); T.parent = N.parent.data(); T.name_pos = N.name_pos.data(); T.name_len = N.name_len.data();
  T.rank = N.rank.data(); T.blob = N.blob.data();
  T.cap_mask = cap - 1; T.mode = (uint32_t)N.mode; T.n_ranks = (uint32_t)N.ranks.size(); T.n_list = (uint32_t)N.list.size();
  for (uint32_t j = 0; j < T.n_list; j++) T.list[j] = N.list[j];
  B.path_len.assign(cap, 0xdeadbeefu); B.rank_len.assign(cap, 0xdeadbeefu); B.rank_src.assign((size_t)cap * std::max(1u, T.n_ranks), 0xdeadbeefu);
  for (uint32_t s = 0; s < cap; s++) {
    uint64_t len = 0;
    if (T.mode == KAIJU_NAMES_PATH) { len = kjn::build_path_len(T, s); B.path_len[s] = kjn::clamp32(len); }
    else if (T.mode == KAIJU_NAMES_RANKS) { len = kjn::build_ranks(T, s, B.rank_src.data() + (size_t)s * T.n_ranks); B.rank_len[s] = kjn::clamp32(len); }
    else if (T.key[s] != ~0ull && !(T.name_len[s] & kjn::kGenerated)) len = T.name_len[s];
    B.max_annotation = std::max(B.max_annotation, len);
  }
  T.path_len = B.path_len.data(); T.rank_src = B.rank_src.data(); T.rank_len = B.rank_len.data();
}

}  // namespace

extern "C" void annotate_emu_constants(uint32_t *out) { out[0] = kjf::kBlockBytes; out[1] = kjf::kScanBlock; out[2] = kChunk; out[3] = kji::kTileBytes; }

extern "C" uint64_t annotate_emu_bound(uint64_t bytes, uint64_t n_lines, const kaiju_taxon_names *tnames) {
  Built B;
  build(*tnames, B);
  return bound(bytes, n_lines, B.max_annotation);
}

// text_in: `bytes` bytes.  info: the twelve 32-bit words of kaiju_gpu_annotate_info.  out: out_cap bytes, changed only where
// lines are written.  order: 0 forward, 1 reversed, 2 shuffled (seed)
extern "C" int annotate_emu(const uint8_t *text_in, uint64_t bytes, const kaiju_taxon_names *tnames, int drop, uint8_t *out, uint64_t out_cap, uint32_t *info,
                            int order, uint32_t seed) {
  if (!tnames || bytes > kji::kMaxBytes) return -1;
  Order o{order, std::mt19937(seed)};
  Built B;
  build(*tnames, B);
  if (B.max_annotation >= kjn::kMaxAnnotation) return -8;
  const Tab &T = B.T;
  // the text as the device sees it: 16-byte aligned, readable to the next multiple of 16 and not one byte further
  const uint64_t padded = (bytes + kChunk - 1) / kChunk * kChunk;
  void *tmem = nullptr;
  if (posix_memalign(&tmem, kChunk, std::max<uint64_t>(padded, kChunk)) != 0) return -6;
  uint8_t *text = static_cast<uint8_t *>(tmem);
  memset(text, 0x5a, std::max<uint64_t>(padded, kChunk));
  if (bytes) memcpy(text, text_in, bytes);

  // ---- lines (k_an_lines_count / k_an_top / k_an_lines_fill) ----
  const uint32_t n_tiles = (uint32_t)((bytes + kji::kTileBytes - 1) / kji::kTileBytes);
  std::vector<uint32_t> tile_cnt((size_t)n_tiles + 1, 0xdeadbeefu), tile_base((size_t)n_tiles + 1, 0xdeadbeefu), line_start(bytes + 2, 0xdeadbeefu);
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
  uint32_t sentinel;
  const uint32_t n = kji::line_count(text, bytes, tile_base[n_tiles], &sentinel);
  line_start[0] = 0;
  line_start[n] = sentinel;

  // ---- len (k_an_len) ----
  std::vector<uint32_t> aslot((size_t)n + 1, 0xdeadbeefu);
  std::vector<uint64_t> olen((size_t)n + 1, 0xdeadbeefdeadbeefull), out_off((size_t)n + 2, 0xdeadbeefdeadbeefull);
  uint32_t count[kWhyCount] = {0, 0, 0, 0, 0, 0, 0};
  for (uint64_t r64 : o.units(n)) {
    const uint32_t r = (uint32_t)r64;
    uint32_t slot, why;
    olen[r] = line_out(text, line_start[r], kji::line_len(line_start.data(), r), T, drop, &slot, &why);
    aslot[r] = slot;
    count[why]++;
  }
  emu::scan_offsets(o, olen.data(), n, kjf::kScanBlock, out_off.data());       // kjl::k_scan_sums / _top / _apply
  const uint64_t total = out_off[n];

  // ---- write (k_an_write) ----
  void *mem = nullptr;
  if (posix_memalign(&mem, kChunk, std::max<uint64_t>(out_cap, 1)) != 0) { free(tmem); return -6; }
  uint8_t *dev_out = static_cast<uint8_t *>(mem);
  if (out_cap) memcpy(dev_out, out, out_cap);
  emu::write_blocks(o, out_off.data(), n, dev_out, out_cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t tot, Chunk *v) {
    return annotate_chunk(c, text, line_start.data(), out_off.data(), aslot.data(), T, lo, hi, tot, out_cap, v);
  });
  if (out_cap) memcpy(out, dev_out, out_cap);
  free(mem);
  free(tmem);
  const kaiju_gpu_annotate_info ai = make_info(total, n, count, out_cap);     // k_an_finish
  memcpy(info, &ai, sizeof ai);
  return 0;
}
