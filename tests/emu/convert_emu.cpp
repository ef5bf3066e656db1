// convert_emu.cpp — kaiju_amd/csrc/kj_convert.h on the host: the per-lane functions of accmap.hip and convert.hip driven pass by
// pass, the units of every pass in the order the caller asks for (lines_emu.h).  What a kernel does with an atomic is a plain
// read-modify-write here; the order of the lanes stands in for the races.  tests/test_convert_emu.py compares with
// tests/convert_expect.py.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kaiju_amd/csrc/kj_convert.h"
#include "../../kaiju_amd/csrc/taxonomy.h"
#include "lines_emu.h"

using namespace kjc;

namespace {

struct EmuTree {
  kaiju_taxonomy *t = nullptr;
  std::vector<uint64_t> key, parent_id;
  std::vector<uint32_t> parent_slot, depth;
  Tree T{};
};

// a text as the device sees it: 16-byte aligned, 16 readable bytes behind it
struct Text {
  std::vector<uint8_t> store;
  uint8_t *p = nullptr;
  uint64_t bytes = 0;
  std::vector<uint32_t> line_start;
  uint32_t n_lines = 0;
  Text(const uint8_t *src, uint64_t n) : store(n + 48, 0x5a), bytes(n) {
    p = store.data() + ((16 - ((uintptr_t)store.data() & 15)) & 15);
    if (n) memcpy(p, src, n);
    line_start.assign(n + 2, 0);
    uint32_t nl = 0;
    for (uint64_t c = 0; c * kChunk < n; c++)
      for (uint32_t m = kji::nl_mask(p, n, c); m; m &= m - 1) line_start[++nl] = (uint32_t)(c * kChunk + kji::ctz16(m) + 1);
    uint32_t sentinel;
    n_lines = kji::line_count(p, n, nl, &sentinel);
    line_start[n_lines] = sentinel;
  }
};

struct EmuMap {
  const EmuTree *tree = nullptr;
  std::vector<uint64_t> from, to;
  std::vector<uint64_t> slots;
  std::vector<uint8_t> arena;
  uint64_t arena_used = 0, entries = 0, lines = 0, no_insert = 0, duplicates = 0, ord_base = 0, rehashes = 0;
  bool full = false;
  Map view() const { return Map{slots.data(), slots.size() - 1, arena.data()}; }
};

void place(std::vector<uint64_t> &slots, const uint8_t *arena, uint64_t v, bool *full) {
  const uint8_t *e = arena + ((v & kEntryMask) - 1) * 8;
  const uint64_t mask = slots.size() - 1;
  uint64_t s = slot_home(key_hash(e + kEntryHead, entry_len(e)), mask);
  for (uint64_t k = 0; k <= mask; k++, s = (s + 1) & mask)
    if (!slots[s]) { slots[s] = v; return; }
  *full = true;
}

struct EmuConv {
  const EmuTree *tree;
  const EmuMap *map, *excl;
  int add_acc;
  std::vector<uint8_t> listed, keep;
};

}  // namespace

extern "C" {

void *cvemu_tree(const char *nodes_path) {
  EmuTree *t = new EmuTree();
  if (kaiju_taxonomy_load(nodes_path, &t->t) != 0) { delete t; return nullptr; }
  kj_taxonomy_table(t->t, t->key, t->parent_id, t->parent_slot, t->depth);
  t->T = Tree{t->key.data(), t->parent_slot.data(), t->depth.data(), (uint32_t)(t->key.size() - 1)};
  return t;
}
void cvemu_tree_free(void *h) { EmuTree *t = static_cast<EmuTree *>(h); if (t) { kaiju_taxonomy_free(t->t); delete t; } }

void *cvemu_map_create(const void *tree, const uint64_t *pairs, uint64_t n_pairs, uint64_t initial_slots) {
  EmuMap *m = new EmuMap();
  m->tree = static_cast<const EmuTree *>(tree);
  std::vector<std::pair<uint64_t, uint64_t>> v;
  for (uint64_t i = 0; i < n_pairs; i++) v.emplace_back(pairs[2 * i], pairs[2 * i + 1]);
  std::stable_sort(v.begin(), v.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
  v.erase(std::unique(v.begin(), v.end(), [](const auto &x, const auto &y) { return x.first == y.first; }), v.end());
  for (auto &p : v) { m->from.push_back(p.first); m->to.push_back(p.second); }
  uint64_t n = 8;
  while (n < initial_slots) n *= 2;
  m->slots.assign(n, 0);
  return m;
}
void cvemu_map_free(void *h) { delete static_cast<EmuMap *>(h); }

// the passes of accmap.hip over a block; returns 1 when the table is full
int cvemu_map_add(void *h, const uint8_t *text, uint64_t n, int first_block, int keys_only, uint64_t value, int order, uint32_t seed) {
  EmuMap *m = static_cast<EmuMap *>(h);
  emu::Order o{order, std::mt19937(seed)};
  const Text X(text, n);
  const Tree T = m->tree ? m->tree->T : Tree{nullptr, nullptr, nullptr, 0};
  const Merged G{m->from.data(), m->to.data(), (uint32_t)m->from.size()};
  std::vector<uint32_t> key_pos(X.n_lines), key_len(X.n_lines, kNone);
  std::vector<uint64_t> taxon(X.n_lines), ent(X.n_lines);
  uint64_t need = 0, valid = 0;
  for (uint64_t i : o.units(X.n_lines)) {                                     // k_am_parse
    const uint64_t a = X.line_start[i], e = (uint64_t)X.line_start[i + 1] - 1;
    if (a >= e || (first_block && i == 0)) continue;
    m->lines++;
    MapLine L = parse_map_line(X.p, a, e, keys_only != 0, value);
    uint32_t slot;
    if (!L.valid || (!keys_only && !resolve_taxon(T, G, &L.taxon, &slot))) { m->no_insert++; continue; }
    key_pos[i] = (uint32_t)L.key; key_len[i] = (uint32_t)(L.key_end - L.key); taxon[i] = L.taxon;
    need += entry_bytes(key_len[i]); valid++;
  }
  m->arena.resize(m->arena_used + need + 8);                                  // grow
  if (m->entries + valid > m->slots.size() / 4 * 3) {
    uint64_t want = m->slots.size();
    while (m->entries + valid > want / 2) want *= 2;
    std::vector<uint64_t> next(want, 0);
    for (uint64_t s : o.units(m->slots.size()))                               // k_am_rehash
      if (m->slots[s]) place(next, m->arena.data(), m->slots[s], &m->full);
    m->slots.swap(next);
    m->rehashes++;
  }
  const uint64_t mask = m->slots.size() - 1;
  for (uint64_t i : o.units(X.n_lines)) {                                     // k_am_insert
    const uint32_t len = key_len[i];
    if (len == kNone) continue;
    const uint8_t *key = X.p + key_pos[i];
    const uint64_t ord = m->ord_base + i, hh = key_hash(key, len), tag = slot_tag(hh);
    uint64_t s = slot_home(hh, mask);
    bool done = false;
    for (uint64_t k = 0; k <= mask && !done; k++, s = (s + 1) & mask) {
      const uint64_t v = m->slots[s];
      if (v == 0) {
        const uint64_t off = m->arena_used;
        m->arena_used += entry_bytes(len);
        uint64_t w[3] = {ord, taxon[i], len};
        memcpy(m->arena.data() + off, w, 24);
        memset(m->arena.data() + off + 24, 0, entry_bytes(len) - 24);
        memcpy(m->arena.data() + off + 24, key, len);
        m->slots[s] = tag << 40 | (off / 8 + 1);
        ent[i] = off / 8; m->entries++; done = true;
        continue;
      }
      if ((v >> 40) != tag) continue;
      uint8_t *e = m->arena.data() + ((v & kEntryMask) - 1) * 8;
      if (entry_len(e) != len || !key_equal(e + kEntryHead, key, len)) continue;
      uint64_t cur = entry_ord(e);
      if (ord < cur) memcpy(e, &ord, 8);
      ent[i] = (v & kEntryMask) - 1; m->duplicates++; done = true;
    }
    if (!done) { key_len[i] = kNone; m->full = true; }
  }
  for (uint64_t i : o.units(X.n_lines)) {                                     // k_am_resolve
    if (key_len[i] == kNone) continue;
    uint8_t *e = m->arena.data() + ent[i] * 8;
    if (entry_ord(e) == m->ord_base + i) memcpy(e + 8, &taxon[i], 8);
  }
  m->ord_base += n + 1;
  return m->full ? 1 : 0;
}

uint64_t cvemu_map_lookup(const void *h, const uint8_t *key, uint32_t n, uint32_t *probes) {
  const EmuMap *m = static_cast<const EmuMap *>(h);
  std::vector<uint8_t> k(key, key + n);                                       // (not aligned, nothing readable behind it)
  const uint8_t *e = map_find(m->view(), k.data(), n, probes);
  return e ? entry_taxon(e) : ~0ull;
}
// entries, slots, arena bytes, lines, lines that inserted nothing, duplicates, rehashes
void cvemu_map_stats(const void *h, uint64_t *out) {
  const EmuMap *m = static_cast<const EmuMap *>(h);
  const uint64_t v[7] = {m->entries, m->slots.size(), m->arena_used, m->lines, m->no_insert, m->duplicates, m->rehashes};
  memcpy(out, v, sizeof v);
}

uint64_t cvemu_strtoul(const uint8_t *text, uint64_t n) {
  uint64_t e = 0;
  while (e < n && text[e]) e++;
  return field_strtoul(text, 0, e);
}
uint64_t cvemu_hash(const uint8_t *key, uint32_t n) { std::vector<uint8_t> k(key, key + n); return key_hash(k.data(), n); }

// the entries of a header line by the local rule: every mark on its own
uint32_t cvemu_entries(const uint8_t *line, uint64_t n, uint32_t *start, uint32_t *end, uint32_t cap, int order, uint32_t seed) {
  emu::Order o{order, std::mt19937(seed)};
  const Text X(line, n);
  std::vector<std::pair<uint32_t, uint32_t>> found;
  for (uint64_t p : o.units(n)) {
    if (!(p == 0 || X.p[p] == 1)) continue;
    uint64_t acc_end;
    if (entry_at(X.p, 0, n, p, &acc_end)) found.emplace_back((uint32_t)p + 1, (uint32_t)acc_end);
  }
  std::sort(found.begin(), found.end());
  for (uint32_t k = 0; k < found.size() && k < cap; k++) { start[k] = found[k].first; end[k] = found[k].second; }
  return (uint32_t)found.size();
}

// the fold of lca_pair over ids in the order given: the id, 0 for an empty set, ~0 where two paths do not meet
uint64_t cvemu_lca_fold(const void *tree, const uint64_t *ids, uint32_t n) {
  const Tree &T = static_cast<const EmuTree *>(tree)->T;
  uint32_t cur = kNone;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t s = kjm::find_slot(T, ids[k]);
    if (s == kNoSlot) continue;
    cur = cur == kNone ? s : lca_pair(T, cur, s);
    if (cur == kNoSlot) return ~0ull;
  }
  return cur == kNone ? 0 : T.key[cur];
}

void *cvemu_conv_create(const void *tree, const uint64_t *ids, uint32_t n, const void *map, const void *excl, int add_acc) {
  EmuConv *c = new EmuConv{static_cast<const EmuTree *>(tree), static_cast<const EmuMap *>(map), static_cast<const EmuMap *>(excl), add_acc ? 1 : 0, {}, {}};
  const Tree &T = c->tree->T;
  c->listed.assign((size_t)T.cap_mask + 1, 0);
  c->keep.assign((size_t)T.cap_mask + 1, 0);
  for (uint32_t i = 0; i < n; i++) { const uint32_t s = kjm::find_slot(T, ids[i]); if (s != kNoSlot) c->listed[s] = 1; }
  for (uint32_t s = 0; s <= T.cap_mask; s++) c->keep[s] = T.key[s] == ~0ull ? 0 : include_walk(T, c->listed.data(), s);
  return c;
}
void cvemu_conv_free(void *h) { delete static_cast<EmuConv *>(h); }

// the passes of convert.hip; out: out_cap bytes, 16-byte aligned
int cvemu_convert(const void *h, const uint8_t *text, uint64_t n, uint8_t *out, uint64_t out_cap, kaiju_gpu_convert_info *info, int order, uint32_t seed) {
  const EmuConv *C = static_cast<const EmuConv *>(h);
  emu::Order o{order, std::mt19937(seed)};
  const Text X(text, n);
  const Tree &T = C->tree->T;
  const Map M = C->map->view(), E = C->excl ? C->excl->view() : Map{nullptr, 0, nullptr};
  const uint32_t nl = X.n_lines;
  std::vector<uint8_t> is_header(nl + 1, 0);
  for (uint64_t i : o.units(nl)) is_header[i] = kji::line_len(X.line_start.data(), (uint32_t)i) > 0 && X.p[X.line_start[i]] == '>';   // k_cv_kinds
  std::vector<uint64_t> hdr_pos(nl + 1), line_off(nl + 1);
  emu::scan_offsets(o, is_header.data(), nl, 256, hdr_pos.data());
  const uint32_t n_rec = (uint32_t)hdr_pos[nl];
  std::vector<uint32_t> rec_line(n_rec + 1), rec_lca(n_rec, kNone), rec_flags(n_rec, 0), rec_first(n_rec, kNone), olen(nl);
  std::vector<uint64_t> rec_taxon(n_rec, 0);
  for (uint64_t i : o.units(nl)) if (is_header[i]) rec_line[hdr_pos[i]] = (uint32_t)i;   // k_cv_records
  rec_line[n_rec] = nl;
  kaiju_gpu_convert_info I{};
  for (uint64_t c : o.units((n + kChunk - 1) / kChunk)) {                                 // k_cv_entries
    const kji::Chunk v = kji::load_chunk(X.p, c);
    uint32_t m = (kji::eq_mask(v, 1) | kji::eq_mask(v, '>')) & kji::range_mask(c * kChunk, 0, n);
    if (!m) continue;
    uint32_t lo = 0, hi = nl;
    const uint64_t p0 = c * kChunk + kji::ctz16(m);
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (X.line_start[mid] <= p0) lo = mid; else hi = mid; }
    uint32_t i = lo;
    for (; m; m &= m - 1) {
      const uint64_t p = c * kChunk + kji::ctz16(m);
      while (i + 1 < nl && X.line_start[i + 1] <= p) i++;
      const uint64_t a = X.line_start[i], e = (uint64_t)X.line_start[i + 1] - 1;
      if (!is_header[i] || p >= e) continue;
      if (X.p[p] == '>' && p != a) continue;
      uint64_t acc_end;
      if (!entry_at(X.p, a, e, p, &acc_end)) continue;
      I.n_entries++;
      const uint32_t r = (uint32_t)hdr_pos[i], len = (uint32_t)(acc_end - p - 1);
      uint32_t probes;
      if (map_find(E, X.p + p + 1, len, &probes)) rec_flags[r] |= kFlagExcluded;
      const uint8_t *ent = map_find(M, X.p + p + 1, len, &probes);
      if (!ent || entry_taxon(ent) == 0) continue;
      const uint32_t slot = kjm::find_slot(T, entry_taxon(ent));
      if (slot == kNoSlot) continue;
      I.n_hits++;
      if ((uint32_t)(p + 1) < rec_first[r]) rec_first[r] = (uint32_t)(p + 1);
      const uint32_t next = rec_lca[r] == kNone ? slot : lca_pair(T, rec_lca[r], slot);   // join_lca
      if (next == kNoSlot) rec_flags[r] |= kFlagNoLca; else rec_lca[r] = next;
    }
  }
  for (uint64_t r : o.units(n_rec)) {                                                     // k_cv_decide
    const uint32_t s = rec_lca[r];
    if (rec_flags[r] & kFlagExcluded) I.dropped_excluded++;
    else if (s == kNone) I.dropped_no_taxon++;
    else if (rec_flags[r] & kFlagNoLca) I.dropped_no_lca++;
    else if (!C->keep[s]) I.dropped_not_included++;
    else { rec_taxon[r] = T.key[s]; I.n_kept++; }
  }
  const View V{X.p, X.line_start.data(), is_header.data(), hdr_pos.data(), rec_line.data(), rec_taxon.data(), rec_first.data(), nl, n_rec, C->add_acc};
  for (uint64_t i : o.units(nl)) olen[i] = line_out_len(V, (uint32_t)i);                  // k_cv_len
  emu::scan_offsets(o, olen.data(), nl, 256, line_off.data());
  emu::write_blocks(o, line_off.data(), nl, out, out_cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) {
    return convert_chunk(c, V, line_off.data(), lo, hi, total, out_cap, v);
  });
  I.text_bytes = line_off[nl];                                                            // k_cv_finish
  I.written_bytes = written_bytes(V, line_off.data(), out_cap);
  I.n_records = n_rec; I.n_lines = nl;
  I.overflow = I.text_bytes > out_cap ? 1u : 0u;
  *info = I;
  return 0;
}

}  // extern "C"
