// tally_emu.cpp — the passes of kaiju_amd/csrc/tally.hip on the host: the per-lane functions of kj_tally.h (and the line pass
// of kj_ingest.h), driven work unit by work unit as tests/emu/merge_emu.cpp does for kj_merge.h.  The units of a pass run in
// the order the caller asks for (forward, reversed, shuffled): no pass may depend on it.  The count pass has the device's
// blocks (kjt::count_blocks), each with the lines of its sweeps and a table of its own (kjt::table_place with a plain
// compare-and-swap), added to direct[] at the block's end; how often a lane found no room and added for itself is counted
// for the tests.  It is compiled together with kaiju_amd/csrc/taxon_names.cpp, whose loader and tables it uses.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_tally.h"
#include "../../kaiju_amd/csrc/taxon_names.h"
#include "lines_emu.h"

using namespace kjt;
using emu::Order;

namespace {

constexpr uint32_t kChunk = kji::kChunk;
constexpr uint32_t kBlockLanes = 256;  // tally.hip's kTlBlock

struct Tally {
  const kaiju_taxon_names *names;
  std::vector<uint64_t> direct, totals;
  std::vector<uint8_t> virus;
  uint64_t spilled = 0;                // lines that found no room in a block's table
};

// the text as the device sees it: 16-byte aligned, readable to the next multiple of 16 and not one byte further
uint8_t *device_text(const uint8_t *in, uint64_t bytes) {
  const uint64_t padded = std::max<uint64_t>((bytes + kChunk - 1) / kChunk * kChunk, kChunk);
  void *mem = nullptr;
  if (posix_memalign(&mem, kChunk, padded) != 0) return nullptr;
  memset(mem, 0x5a, padded);
  if (bytes) memcpy(mem, in, bytes);
  return static_cast<uint8_t *>(mem);
}

// k_tl_lines_count / k_tl_top / k_tl_lines_fill; returns the number of '\n'
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

extern "C" void tally_emu_constants(uint32_t *out) { out[0] = kji::kTileBytes; out[1] = kChunk; out[2] = sizeof(kaiju_gpu_tally_entry); out[3] = sizeof(kaiju_gpu_tally_info); out[4] = kTableSlots; out[5] = (uint32_t)kCountShare; }

extern "C" void *tally_emu_create(const kaiju_taxon_names *names, int order, uint32_t seed) {
  Order o{order, std::mt19937(seed)};
  Tally *t = new Tally{names, {}, {}, {}};
  const uint32_t cap = (uint32_t)names->key.size();
  t->direct.assign(cap, 0);
  t->totals.assign(2 + kCounts, 0);
  t->virus.assign(cap, 0xa7);
  const uint32_t vslot = kjn::find_slot(names->key.data(), cap - 1, kVirusTaxon);                // k_tl_virus
  for (uint64_t s : o.units(cap)) t->virus[s] = names->key[s] != ~0ull && is_virus(names->parent.data(), vslot, (uint32_t)s) ? 1 : 0;
  return t;
}
extern "C" uint64_t tally_emu_spilled(void *h) { return static_cast<Tally *>(h)->spilled; }
extern "C" void tally_emu_free(void *h) { delete static_cast<Tally *>(h); }
extern "C" void tally_emu_reset(void *h) {
  Tally *t = static_cast<Tally *>(h);
  std::fill(t->direct.begin(), t->direct.end(), 0);
  std::fill(t->totals.begin(), t->totals.end(), 0);
}

// order: 0 forward, 1 reversed, 2 shuffled (seed)
extern "C" int tally_emu_add(void *h, const uint8_t *in, uint64_t bytes, int final, kaiju_gpu_tally_info *info, int order, uint32_t seed) {
  Tally *t = static_cast<Tally *>(h);
  if (bytes > kji::kMaxBytes) return -1;
  Order o{order, std::mt19937(seed)};
  uint8_t *text = device_text(in, bytes);
  if (!text) return -6;
  const uint64_t *key = t->names->key.data();
  const uint32_t cap_mask = (uint32_t)t->names->key.size() - 1;

  // ---- lines, plan (k_tl_plan) ----
  std::vector<uint32_t> ls;
  const uint32_t n_nl = lines(o, text, bytes, ls);
  ls[0] = 0;
  uint32_t sentinel;
  uint64_t used;
  const uint32_t n = lines_counted(text, bytes, n_nl, ls[n_nl], final, &sentinel, &used);
  ls[n] = sentinel;

  // ---- count (k_tl_count_table): blocks, their sweeps, their tables ----
  uint64_t count[kCounts] = {0, 0, 0, 0, 0};
  const uint32_t blocks = count_blocks(bytes);
  for (uint64_t b : o.units(blocks)) {
    std::vector<uint32_t> t_key(kTableSlots, kNone), t_cnt(kTableSlots, 0);
    for (uint64_t r0 = b * kBlockLanes; r0 < n; r0 += (uint64_t)blocks * kBlockLanes) {
      for (uint64_t l : o.units(kBlockLanes)) {
        const uint64_t r = r0 + l;
        if (r >= n) continue;
        uint32_t slot;
        const uint32_t kind = line_kind(text, ls[r], kji::line_len(ls.data(), (uint32_t)r), key, cap_mask, &slot);
        count[kCntTotal] += kind != kLineEmpty;
        count[kCntUnclassified] += kind == kLineUnclassified;
        count[kCntBadId] += kind == kLineBadId;
        count[kCntUnknown] += kind == kLineUnknown;
        if (slot == kNone) continue;
        count[kCntVirus] += t->virus[slot];
        const uint32_t i = table_place(slot, [&](uint32_t at, uint32_t v) { const uint32_t old = t_key[at]; if (old == kNone) t_key[at] = v; return old; });
        if (i != kNone) t_cnt[i]++;
        else { t->direct[slot] += 1; t->spilled++; }
      }
    }
    for (uint64_t i : o.units(kTableSlots)) if (t_cnt[i]) t->direct[t_key[i]] += t_cnt[i];
  }

  // ---- finish (k_tl_finish) ----
  *info = make_info(used, n, count);
  t->totals[0] += used;
  t->totals[1] += n;
  for (int w = 0; w < kCounts; w++) t->totals[2 + w] += count[w];
  free(text);
  return 0;
}

// entries: room for cap; *n_entries: how many there are (more than cap: -2, none written)
extern "C" int tally_emu_result(void *h, kaiju_gpu_tally_entry *entries, uint64_t cap, uint64_t *n_entries, kaiju_gpu_tally_info *totals, int order, uint32_t seed) {
  Tally *t = static_cast<Tally *>(h);
  Order o{order, std::mt19937(seed)};
  const kaiju_taxon_names &N = *t->names;
  const uint32_t slots = (uint32_t)N.key.size();
  std::vector<uint64_t> summed(slots, 0), pos((size_t)slots + 1, 0xdeadbeefdeadbeefull);
  std::vector<uint32_t> flag(slots, 0xdeadbeefu);
  for (uint64_t s : o.units(slots))                                                               // k_tl_sum
    if (t->direct[s]) sum_walk(N.parent.data(), t->virus.data(), (uint32_t)s, t->direct[s], [&](uint32_t a, uint64_t v) { summed[a] += v; });
  for (uint64_t s : o.units(slots)) flag[s] = summed[s] ? 1u : 0u;                                // k_tl_flag
  emu::scan_offsets(o, flag.data(), slots, 256, pos.data());
  *totals = make_info(t->totals[0], t->totals[1], t->totals.data() + 2);
  *n_entries = pos[slots];
  if (pos[slots] > cap) return -2;
  for (uint64_t s : o.units(slots))                                                               // k_tl_compact
    if (flag[s]) entries[pos[s]] = make_entry(N.key[s], t->direct[s], summed[s], t->virus[s]);
  return 0;
}
