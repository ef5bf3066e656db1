// refseq_emu.cpp — the rule set of kaiju-convertRefSeq (kaiju_amd/csrc/kj_convert.h) on the host: refseq_map_line as k_am_parse
// calls it and first_entry as k_cv_first calls it, driven pass by pass with the units of every pass in the order the caller
// asks for.  The tree, the text, the map and every pass the two rule sets share are those of convert_emu.cpp, which this file
// includes: its cvemu_* entry points (the rules of kaiju-convertNR) are in the same library, so that one test can put a text
// through both.  tests/test_refseq_emu.py compares with tests/refseq_expect.py.
#include "convert_emu.cpp"

extern "C" {

// the passes of accmap.hip over a block of a map made with the RefSeq rules; returns 1 when the table is full
int rsemu_map_add(void *h, const uint8_t *text, uint64_t n, int first_block, int order, uint32_t seed) {
  EmuMap *m = static_cast<EmuMap *>(h);
  emu::Order o{order, std::mt19937(seed)};
  const Text X(text, n);
  const Tree T = m->tree->T;
  const Merged G{m->from.data(), m->to.data(), (uint32_t)m->from.size()};
  std::vector<uint32_t> key_pos(X.n_lines), key_len(X.n_lines, kNone);
  std::vector<uint64_t> taxon(X.n_lines), ent(X.n_lines);
  uint64_t need = 0, valid = 0;
  for (uint64_t i : o.units(X.n_lines)) {                                     // k_am_parse
    const uint64_t a = X.line_start[i], e = (uint64_t)X.line_start[i + 1] - 1;
    if (a >= e || (first_block && i == 0)) continue;
    m->lines++;
    const MapLine L = refseq_map_line(X.p, a, e, T, G);
    if (!L.valid) { m->no_insert++; continue; }
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
      if (ord < entry_ord(e)) memcpy(e, &ord, 8);
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

// where first_space finds the first space of the header line text[a, e), e where there is none; the text is laid out as the
// device sees it, with byte 0 16-byte aligned
uint64_t rsemu_first_space(const uint8_t *text, uint64_t n, uint64_t a, uint64_t e) {
  const Text X(text, n);
  return first_space(X.p, a, e);
}

// the passes of convert.hip under the RefSeq rules (h: a cvemu_conv_create over a map of rsemu_map_add, without an excluded map)
int rsemu_convert(const void *h, const uint8_t *text, uint64_t n, uint8_t *out, uint64_t out_cap, kaiju_gpu_convert_info *info, int order, uint32_t seed) {
  const EmuConv *C = static_cast<const EmuConv *>(h);
  emu::Order o{order, std::mt19937(seed)};
  const Text X(text, n);
  const Tree &T = C->tree->T;
  const Map M = C->map->view();
  const uint32_t nl = X.n_lines;
  std::vector<uint8_t> is_header(nl + 1, 0);
  for (uint64_t i : o.units(nl)) is_header[i] = kji::line_len(X.line_start.data(), (uint32_t)i) > 0 && X.p[X.line_start[i]] == '>';   // k_cv_kinds
  std::vector<uint64_t> hdr_pos(nl + 1), line_off(nl + 1);
  emu::scan_offsets(o, is_header.data(), nl, 256, hdr_pos.data());
  const uint32_t n_rec = (uint32_t)hdr_pos[nl];
  // (k_cv_records sets the three to kNone, 0, kNone; other values here show that k_cv_first stores all of them)
  std::vector<uint32_t> rec_line(n_rec + 1), rec_lca(n_rec, 7), rec_flags(n_rec, kFlagExcluded | kFlagNoLca), rec_first(n_rec, 7), olen(nl);
  std::vector<uint64_t> rec_taxon(n_rec, 0);
  for (uint64_t i : o.units(nl)) if (is_header[i]) rec_line[hdr_pos[i]] = (uint32_t)i;   // k_cv_records
  rec_line[n_rec] = nl;
  kaiju_gpu_convert_info I{};
  for (uint64_t r : o.units(n_rec)) {                                                     // k_cv_first
    const uint32_t i = rec_line[r];
    const First F = first_entry(X.p, X.line_start[i], (uint64_t)X.line_start[i + 1] - 1, M, T);
    rec_lca[r] = F.slot; rec_first[r] = F.first; rec_flags[r] = 0;
    I.n_entries += F.entry; I.n_hits += F.hit;
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
