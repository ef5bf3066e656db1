// kj_convert.h — kaiju-convertNR on blocks of text: the per-lane logic, for the device (accmap.hip, convert.hip) and for the
// host (tests/emu/convert_emu.cpp drives the same functions pass by pass).  kaiju-convertRefSeq is a second rule set over the
// same map and the same passes: its rules stand with its code below ("kaiju-convertRefSeq"; tests/emu/refseq_emu.cpp).
//
// The rules are those of kaiju-convertNR.cpp:145-306 and util.cpp:79-121, :194-263 of the reference (getline, find, substr,
// strtoul, unordered_map::emplace, lca_from_ids), observed on the unmodified tool (tests/golden/convert/):
//   map       the first line is skipped, empty lines are skipped.  t1 = find('\t'), t2 = find('\t', t1 + 1).  The key is
//             substr(t1 + 1, t2 - t1 - 1), the taxon strtoul(c_str() + t2 + 1).  With npos + 1 == 0 a line without a tab has the
//             whole line as its key and the number at its front as its taxon; a line with one tab has what follows the tab as its
//             key and the number at the front of the line as its taxon.  Observed: "561" maps "561" to 561, "1386\tK1" maps "K1"
//             to 1386.  strtoul: leading " \t\n\v\f\r", one sign, decimal digits; no digit: 0; a magnitude above 2^64 - 1:
//             ULONG_MAX; '-' negates modulo 2^64 (observed: "-18446744073709551054" is 562).  ULONG_MAX skips the line.  A taxon
//             that is no node goes through `merged` once; still no node: the line inserts nothing.  emplace: the first line that
//             inserts a key wins, a line that inserted nothing does not count.  A key may have zero bytes ("Q0\t\t1423")
//   excluded  every non-empty line, whole, is a key
//   text      a line ends at '\n', the last one may lack it; '\r' is a byte of the line.  Lines of length 0 are nothing.  A line
//             whose byte 0 is '>' is a header; every other line is a sequence line of the record of the last header in front of
//             it; sequence lines in front of the first header are dropped
//   header    start = 1; loop: end = find(' ', start), none: stop; the accession is [start, end); excluded: the record is
//             dropped; in the map with a taxon > 0: the taxon joins the set, with -a the first such accession is kept;
//             start = find('\x01', end + 1) + 1, none: stop
//   local     the same without the loop.  Call byte 0 of the line and every '\x01' a mark.  A '\x01' at p separates entries iff
//             a space lies between the mark in front of it and p.  Proof, by induction over the entries of the loop: let an
//             entry start at s, where s - 1 is a mark (byte 0, or the separator found last), and let e be the first space at or
//             behind s.  Every '\x01' in [s, e) has only bytes of [s, e) between the mark in front of it and itself, none of them
//             a space: no separator, and the loop, too, takes them as bytes of the accession.  The first '\x01' behind e, at p,
//             has its previous mark at s - 1 or inside [s, e), so e lies between: a separator, and the loop's next start is
//             p + 1.  Without a space behind s the loop stops, and no later '\x01' has a space in front of it either.  So the
//             entries are: the byte behind a mark that is byte 0 or a separator, up to the first space behind it; without such a
//             space it is no entry.  (Observed: ">V\x011.1 x\x01\x01A1.1 z" looks up "V\x011.1" and "\x01A1.1".)
//   decision  an empty set drops the record.  The taxon is the single id or lca_from_ids of the set: every member is a node,
//             so that is the lowest common ancestor.  Here it is a fold of the pairwise LCA by depths: on a tree the LCA of a
//             set is the LCA of (the LCA of a subset) and (the LCA of the rest) - the ancestors of a node form a chain, and
//             the common ancestors of a set are the intersection of chains ending at the root, a chain again - so the fold is
//             exact in any order and any grouping.  The record is kept iff the walk `while (node(id) && id != 1)` from the taxon
//             meets an id of the include list.  Id 1 itself never keeps a record
//   output    '>' [first accession '_'] taxon '\n', the bytes of the record's sequence lines that are in ARNDCQEGHILKMFPSTWYV,
//             '\n'.  The tool writes "\n" in front of every record but the first and endl at the end of the file: per record that is
//             the '\n' behind it, and a file of which nothing is kept is the one byte "\n" - that byte is the caller's, who knows
//             when the file ends (host/convert_main.cpp, api.Converter.convert_file)
// Deliberately different: where the tree is no tree (two roots, a parent that is no node) lca_from_ids never returns or
// throws; here every walk counts down the depth stored with the slot, two paths that do not meet drop the record and it is
// counted (dropped_no_lca).  The include walk is bounded the same way.
//
// The map: open addressing over 64-bit slots, slot = tag << 40 | entry, 0 = empty.  entry - 1 is the offset / 8 of an entry in
// the arena: { ord, taxon, len, pad, key bytes padded to 8 }.  ord is the number of the line (over every block added) that
// gave the entry its taxon: lines of an equal key take the minimum of their numbers, the line whose number that is writes the
// taxon in a pass of its own - which lane came first does not matter.
//
// Passes of a conversion (independent units each; the units of a pass may run in any order):
//   lines    that of kj_ingest.h
//   kinds    one lane per line: header or not; a prefix sum numbers the records
//   entries  one lane per 16 bytes of text: the marks of its chunk that start an entry, both lookups, and the record's
//            reduction with atomics: LCA (compare-and-swap over the slot of the tree), "any excluded", the smallest position of
//            an accession with a taxon.  A header of thousands of entries is thousands of lanes
//   decide   one lane per record
//   lengths  one lane per line: bytes it gives to the output (a header, the letters counted in 16-byte chunks, the '\n')
//   offsets  kjl::launch_offsets;  write: kjl::write_blocks over convert_chunk;  finish: kaiju_gpu_convert_info
#ifndef KJ_CONVERT_H
#define KJ_CONVERT_H

#include "kj_format.h"
#include "kj_ingest.h"
#include "kj_merge.h"

namespace kjc {

using kjf::Chunk;
using kjf::kChunk;
using kjm::Tree;
using kjm::kNoSlot;

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint64_t kSkip = ~0ull;                    // ULONG_MAX
constexpr uint32_t kEntryHead = 24;                  // bytes of an entry in front of its key
constexpr uint64_t kEntryMask = (1ull << 40) - 1;
constexpr uint32_t kFlagExcluded = 1u, kFlagNoLca = 2u;

// ---- keys ---------------------------------------------------------------------------------------------------------
KJF_HD uint64_t load_word(const uint8_t *p, uint32_t n) {      // n <= 8 bytes, the rest zero
  uint64_t w = 0;
  if (n == 8) { __builtin_memcpy(&w, p, 8); return w; }
  for (uint32_t k = 0; k < n; k++) w |= (uint64_t)p[k] << (8 * k);
  return w;
}
KJF_HD uint64_t mix(uint64_t h, uint64_t w) { h = (h ^ w) * 0x9e3779b97f4a7c15ull; return h ^ (h >> 29); }
// 16 bytes a step; the length goes in, so that "A" and "A\0" differ
KJF_HD uint64_t key_hash(const uint8_t *p, uint32_t n) {
  uint64_t h = 0x2545f4914f6cdd1dull ^ n;
  uint32_t k = 0;
  for (; k + 16 <= n; k += 16) { h = mix(h, load_word(p + k, 8)); h = mix(h, load_word(p + k + 8, 8)); }
  if (n - k > 8) { h = mix(h, load_word(p + k, 8)); h = mix(h, load_word(p + k + 8, n - k - 8)); }
  else if (n - k) h = mix(h, load_word(p + k, n - k));
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return h;
}
KJF_HD bool key_equal(const uint8_t *x, const uint8_t *y, uint32_t n) {
  uint32_t k = 0;
  for (; k + 16 <= n; k += 16)
    if (load_word(x + k, 8) != load_word(y + k, 8) || load_word(x + k + 8, 8) != load_word(y + k + 8, 8)) return false;
  for (; k < n; k++) if (x[k] != y[k]) return false;
  return true;
}
KJF_HD uint64_t slot_tag(uint64_t h) { return h >> 40; }                     // 24 bits
KJF_HD uint64_t slot_home(uint64_t h, uint64_t mask) { return (h * 0x9e3779b97f4a7c15ull >> 20) & mask; }
KJF_HD uint64_t entry_bytes(uint32_t key_len) { return kEntryHead + (((uint64_t)key_len + 7) & ~7ull); }

struct Map {
  const uint64_t *slots;       // nullptr: the empty map
  uint64_t mask;               // slots - 1
  const uint8_t *arena;
};
KJF_HD uint64_t entry_ord(const uint8_t *e) { uint64_t v; __builtin_memcpy(&v, e, 8); return v; }
KJF_HD uint64_t entry_taxon(const uint8_t *e) { uint64_t v; __builtin_memcpy(&v, e + 8, 8); return v; }
KJF_HD uint32_t entry_len(const uint8_t *e) { uint32_t v; __builtin_memcpy(&v, e + 16, 4); return v; }
// the entry of key[0, n), or nullptr.  At most mask + 1 probes
KJF_HD const uint8_t *map_find(const Map &M, const uint8_t *key, uint32_t n, uint32_t *probes) {
  *probes = 0;
  if (!M.slots) return nullptr;
  const uint64_t h = key_hash(key, n), tag = slot_tag(h);
  uint64_t s = slot_home(h, M.mask);
  for (uint64_t i = 0; i <= M.mask; i++, s = (s + 1) & M.mask) {
    const uint64_t v = M.slots[s];
    ++*probes;
    if (v == 0) return nullptr;
    if ((v >> 40) != tag) continue;
    const uint8_t *e = M.arena + ((v & kEntryMask) - 1) * 8;
    if (entry_len(e) == n && key_equal(e + kEntryHead, key, n)) return e;
  }
  return nullptr;
}

// ---- a line of the map file ---------------------------------------------------------------------------------------
// strtoul of text[p, e) (e: where the C string ends)
KJF_HD uint64_t field_strtoul(const uint8_t *text, uint64_t p, uint64_t e) {
  while (p < e && (text[p] == ' ' || (text[p] >= '\t' && text[p] <= '\r'))) p++;
  bool neg = false;
  if (p < e && (text[p] == '+' || text[p] == '-')) { neg = text[p] == '-'; p++; }
  uint64_t acc = 0;
  bool over = false;
  for (; p < e; p++) {
    const uint32_t d = (uint32_t)text[p] - '0';
    if (d > 9) break;
    if (acc > kjm::kMaxTenth || (acc == kjm::kMaxTenth && d > 5)) over = true;
    acc = acc * 10 + d;
  }
  if (over) return kSkip;
  return neg ? 0 - acc : acc;
}
struct MapLine { uint64_t key, key_end, taxon; bool valid; };
// line [a, e), a < e.  keys_only: the whole line is the key, the taxon is `value`
KJF_HD MapLine parse_map_line(const uint8_t *text, uint64_t a, uint64_t e, bool keys_only, uint64_t value) {
  MapLine L{a, e, value, true};
  if (keys_only) return L;
  uint64_t tab[2];
  const uint32_t seen = kjm::find_tabs(text, a, e, 2, tab);
  L.key = seen >= 1 ? tab[0] + 1 : a;
  L.key_end = seen >= 2 ? tab[1] : e;
  uint64_t z = seen >= 2 ? tab[1] + 1 : a;                   // (strtoul reads a C string: a NUL ends it)
  uint64_t ze = z;
  while (ze < e && text[ze]) ze++;
  L.taxon = field_strtoul(text, z, ze);
  L.valid = L.taxon != kSkip;
  return L;
}
struct Merged { const uint64_t *from, *to; uint32_t n; };    // sorted by `from`, one pair per id
// the node a taxon of the map file stands for: *slot, or false.  *via_merged: the taxon itself is no node, `merged` gave the node
KJF_HD bool resolve_taxon(const Tree &T, const Merged &G, uint64_t *taxon, uint32_t *slot, bool *via_merged = nullptr) {
  uint32_t s = kjm::find_slot(T, *taxon);
  if (via_merged) *via_merged = s == kNoSlot;
  if (s == kNoSlot) {
    uint32_t lo = 0, hi = G.n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (G.from[mid] < *taxon) lo = mid + 1; else hi = mid; }
    if (lo >= G.n || G.from[lo] != *taxon) return false;
    *taxon = G.to[lo];
    s = kjm::find_slot(T, *taxon);
    if (s == kNoSlot) return false;
  }
  *slot = s;
  return true;
}

// ---- the header ---------------------------------------------------------------------------------------------------
// p is a mark of the header line [a, e) (a itself, or a '\x01'): does an entry start behind it?  *acc_end: its first space
KJF_HD bool entry_at(const uint8_t *text, uint64_t a, uint64_t e, uint64_t p, uint64_t *acc_end) {
  if (p != a) {                                              // a separator: a space between the mark in front and p
    bool space = false;
    for (uint64_t q = p; q-- > a;) {
      if (text[q] == ' ') { space = true; break; }
      if (text[q] == 1 || q == a) break;
    }
    if (!space) return false;
  }
  for (uint64_t q = p + 1; q < e; q++)
    if (text[q] == ' ') { *acc_end = q; return true; }
  return false;
}

// ---- kaiju-convertRefSeq ------------------------------------------------------------------------------------------
// The second rule set (kRulesRefSeq): kaiju-convertRefSeq.cpp:145-262 of the reference, observed on the unmodified tool
// (tests/golden/refseq/).  What it shares with kaiju-convertNR - lines, the include walk, the letters, the '\n' per record, the
// overflow rule - is the code above and below; what differs:
//   map       two columns, accession.version '\t' taxon.  The first line is skipped, empty lines are skipped.  t = find('\t'):
//             a line without a tab inserts nothing (there it is a key).  The line must begin with the three bytes "WP_"
//             (observed: "wp_", "NP_", "XP_" insert nothing; a "WP_" line has t >= 3).  The taxon is strtoul(c_str() + t + 1),
//             field_strtoul as it is; ULONG_MAX and 0 insert nothing, so a four-column line ("WP_1\tWP_1.1\t562\t9" parses
//             "WP_1.1": 0) inserts nothing.  A taxon that is a node: the key is [0, t).  A taxon that is no node but that
//             `merged` maps to a node: the key is [0, t - 1) - substr(0, start - 1), the accession loses its last byte (observed:
//             "WP_123\t666" is found as "WP_12", "WP_\t666" as "WP").  Neither: nothing.  emplace: the first line that inserts a
//             key wins, whichever of the two forms gave the key ("WP_12\t562" in front of "WP_123\t666": 562)
//   header    the accession is [1, first space); a header without a space is dropped without a lookup.  No loop over '\x01':
//             it is a byte of the accession or of the description like any other.  Found in the map: the record's taxon is the
//             entry's; not found: dropped.  No LCA, no excluded set
//   output    '>' [accession '_'] taxon '\n' letters '\n' as above; -a writes the accession looked up
//   counters  n_entries: headers with a space; n_hits: those found; dropped_excluded and dropped_no_lca stay 0
// Passes: those above, with `entries` replaced by `first`: one lane per record reads its header in 16-byte chunks from the
// line start up to the first space or the line end, one map_find, one find_slot, plain stores.
constexpr int kRulesNr = 0, kRulesRefSeq = 1;

// line [a, e) of the map file, a < e: the key and the node's id, or !valid
KJF_HD MapLine refseq_map_line(const uint8_t *text, uint64_t a, uint64_t e, const Tree &T, const Merged &G) {
  MapLine L{a, e, 0, false};
  uint64_t t;
  if (!kjm::find_tabs(text, a, e, 1, &t)) return L;
  if (e - a < 3 || text[a] != 'W' || text[a + 1] != 'P' || text[a + 2] != '_') return L;
  uint64_t ze = t + 1;                                         // (strtoul reads a C string: a NUL ends it)
  while (ze < e && text[ze]) ze++;
  L.taxon = field_strtoul(text, t + 1, ze);
  if (L.taxon == kSkip || L.taxon == 0) return L;
  uint32_t slot;
  bool via_merged;
  if (!resolve_taxon(T, G, &L.taxon, &slot, &via_merged)) return L;
  L.key_end = via_merged ? t - 1 : t;                          // (t >= a + 3)
  L.valid = true;
  return L;
}

// the first space of the header line [a, e) behind its '>', e where there is none
KJF_HD uint64_t first_space(const uint8_t *text, uint64_t a, uint64_t e) {
  for (uint64_t c = (a + 1) / kChunk; c * kChunk < e; c++) {
    const uint32_t m = kji::eq_mask(kji::load_chunk(text, c), ' ') & kji::range_mask(c * kChunk, a + 1, e);
    if (m) return c * kChunk + kji::ctz16(m);
  }
  return e;
}
struct First { uint32_t slot, first; bool entry, hit; };       // slot, first: kNone without a hit
// the one entry of the header line [a, e): is there one, does the map hold it, the slot of its taxon
KJF_HD First first_entry(const uint8_t *text, uint64_t a, uint64_t e, const Map &M, const Tree &T) {
  First F{kNone, kNone, false, false};
  const uint64_t sp = first_space(text, a, e);
  if (sp >= e) return F;
  F.entry = true;
  uint32_t probes;
  const uint8_t *ent = map_find(M, text + a + 1, (uint32_t)(sp - a - 1), &probes);
  if (!ent || entry_taxon(ent) == 0) return F;
  const uint32_t slot = kjm::find_slot(T, entry_taxon(ent));
  if (slot == kNoSlot) return F;                               // (the map holds nodes only)
  F.slot = slot; F.first = (uint32_t)(a + 1); F.hit = true;
  return F;
}

// ---- the tree -----------------------------------------------------------------------------------------------------
// the lowest common ancestor of slots x and y; kNoSlot where their paths do not meet
KJF_HD uint32_t lca_pair(const Tree &T, uint32_t x, uint32_t y) {
  uint32_t dx = T.depth[x], dy = T.depth[y];
  while (dx > dy) { x = kjm::up(T, x); dx--; }
  while (dy > dx) { y = kjm::up(T, y); dy--; }
  while (x != y && dx > 0) { x = kjm::up(T, x); y = kjm::up(T, y); dx--; }
  return x == y ? x : kNoSlot;
}
// `while (node(id) && id != 1) { if (listed(id)) keep; id = parent(id); }` from slot s, at most depth + 1 steps
KJF_HD uint8_t include_walk(const Tree &T, const uint8_t *listed, uint32_t s) {
  for (uint32_t d = T.depth[s] + 1; d > 0; d--) {
    if (T.key[s] == 1) return 0;
    if (listed[s]) return 1;
    const uint32_t p = T.parent_slot[s];
    if (p == kNoSlot || p == s) return 0;
    s = p;
  }
  return 0;
}

// ---- letters ------------------------------------------------------------------------------------------------------
constexpr uint32_t kAaBits = (1u << ('A' - 'A')) | (1u << ('R' - 'A')) | (1u << ('N' - 'A')) | (1u << ('D' - 'A')) | (1u << ('C' - 'A')) |
                             (1u << ('Q' - 'A')) | (1u << ('E' - 'A')) | (1u << ('G' - 'A')) | (1u << ('H' - 'A')) | (1u << ('I' - 'A')) |
                             (1u << ('L' - 'A')) | (1u << ('K' - 'A')) | (1u << ('M' - 'A')) | (1u << ('F' - 'A')) | (1u << ('P' - 'A')) |
                             (1u << ('S' - 'A')) | (1u << ('T' - 'A')) | (1u << ('W' - 'A')) | (1u << ('Y' - 'A')) | (1u << ('V' - 'A'));
KJF_HD bool is_aa(uint32_t b) { const uint32_t k = b - 'A'; return k < 26u && ((kAaBits >> k) & 1u); }
// bit k set: byte k of chunk c is one of the twenty letters and lies in [a, e)
KJF_HD uint32_t aa_mask(const uint8_t *text, uint64_t c, uint64_t a, uint64_t e) {
  const kji::Chunk v = kji::load_chunk(text, c);
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < kChunk; k++) m |= (is_aa(kji::chunk_byte(v, k)) ? 1u : 0u) << k;
  return m & kji::range_mask(c * kChunk, a, e);
}
KJF_HD uint32_t count_letters(const uint8_t *text, uint64_t a, uint64_t e) {
  uint32_t n = 0;
  for (uint64_t c = a / kChunk; c * kChunk < e; c++) n += kji::popc16(aa_mask(text, c, a, e));
  return n;
}
// the position of letter j (from 0) of [a, e); there is one
KJF_HD uint64_t nth_letter(const uint8_t *text, uint64_t a, uint64_t e, uint32_t j) {
  for (uint64_t c = a / kChunk; c * kChunk < e; c++) {
    uint32_t m = aa_mask(text, c, a, e);
    const uint32_t n = kji::popc16(m);
    if (j >= n) { j -= n; continue; }
    for (; j; j--) m &= m - 1;
    return c * kChunk + kji::ctz16(m);
  }
  return e;
}

// ---- records, lengths ---------------------------------------------------------------------------------------------
struct View {
  const uint8_t *text;
  const uint32_t *line_start;  // [n_lines + 1]
  const uint8_t *is_header;    // [n_lines]
  const uint64_t *hdr_pos;     // [n_lines + 1] headers in front of the line
  const uint32_t *rec_line;    // [n_records + 1], the last: n_lines
  const uint64_t *rec_taxon;   // [n_records] 0: dropped
  const uint32_t *rec_first;   // [n_records] where the accession of -a starts
  uint32_t n_lines, n_records;
  int add_acc;
};
// the record line i belongs to, kNone in front of the first header
KJF_HD uint32_t record_of(const View &V, uint32_t i) { const uint64_t h = V.hdr_pos[i] + V.is_header[i]; return h ? (uint32_t)(h - 1) : kNone; }
KJF_HD uint32_t acc_len(const View &V, uint32_t r) {
  const uint64_t e = (uint64_t)V.line_start[V.rec_line[r] + 1] - 1;
  uint64_t q = V.rec_first[r];
  while (q < e && V.text[q] != ' ') q++;
  return (uint32_t)(q - V.rec_first[r]);
}
KJF_HD uint32_t header_len(const View &V, uint32_t r) { return 1 + (V.add_acc ? acc_len(V, r) + 1 : 0) + kjf::digits_u64(V.rec_taxon[r]) + 1; }
// bytes line i gives to the output
KJF_HD uint32_t line_out_len(const View &V, uint32_t i) {
  const uint32_t r = record_of(V, i);
  if (r == kNone || V.rec_taxon[r] == 0) return 0;
  const uint32_t last = i + 1 == V.rec_line[r + 1] ? 1u : 0u;                     // the '\n' behind the record
  if (V.is_header[i]) return header_len(V, r) + last;
  return count_letters(V.text, V.line_start[i], (uint64_t)V.line_start[i + 1] - 1) + last;
}

// ---- write --------------------------------------------------------------------------------------------------------
struct Unit {
  uint64_t off, len;
  uint32_t line, rec, alen, digits;
  uint64_t a, e, cursor;       // of a sequence line: its bytes, the letter written last
  kjf::Bcd bcd;
  bool header, fits;
};
KJF_HD Unit load_unit(const View &V, const uint64_t *line_off, uint32_t i, uint64_t out_cap) {
  Unit U{};
  U.off = line_off[i]; U.len = line_off[i + 1] - U.off;
  U.line = i;
  if (!U.len) return U;
  U.rec = record_of(V, i);
  U.header = V.is_header[i];
  U.fits = line_off[V.rec_line[U.rec + 1]] <= out_cap;        // the whole record lies in front of out_cap
  U.a = V.line_start[i]; U.e = (uint64_t)V.line_start[i + 1] - 1;
  U.cursor = kSkip;
  if (U.header) {
    U.alen = V.add_acc ? acc_len(V, U.rec) : 0;
    U.digits = kjf::digits_u64(V.rec_taxon[U.rec]);
    U.bcd = kjf::to_bcd(V.rec_taxon[U.rec]);
  }
  return U;
}
// byte p of the unit (p < U.len); the bytes of a sequence line are asked for in rising order
KJF_HD uint32_t unit_byte(const View &V, Unit &U, uint64_t p) {
  if (U.header) {
    if (p == 0) return '>';
    p -= 1;
    if (V.add_acc) {
      if (p < U.alen) return V.text[V.rec_first[U.rec] + p];
      if (p == U.alen) return '_';
      p -= U.alen + 1;
    }
    if (p < U.digits) return '0' + kjf::bcd_digit(U.bcd, U.digits - 1 - (uint32_t)p);
    return '\n';                                              // the header's, or behind it the record's
  }
  uint64_t q;
  if (U.cursor == kSkip) q = nth_letter(V.text, U.a, U.e, (uint32_t)p);
  else for (q = U.cursor + 1; q < U.e && !is_aa(V.text[q]); q++) {}
  if (q >= U.e) return '\n';                                  // behind the last letter: the record's '\n'
  U.cursor = q;
  return V.text[q];
}
// the bytes of chunk c of the output; lo, hi: the lines the chunk's block touches
KJF_HD uint32_t convert_chunk(uint64_t c, const View &V, const uint64_t *line_off, uint32_t lo, uint32_t hi, uint64_t total, uint64_t out_cap, Chunk *v) {
  const uint64_t o = c * kChunk;
  *v = Chunk{{0, 0, 0, 0}};
  if (o >= total) return 0;
  uint32_t i = kjf::find_record(line_off, lo, hi, o);          // the largest line with line_off[i] <= o: it has bytes
  Unit U = load_unit(V, line_off, i, out_cap);
  uint64_t w0 = 0, w1 = 0;
  uint32_t m = 0;
  for (uint32_t k = 0; k < kChunk; k++) {
    const uint64_t pos = o + k;
    if (pos >= total) break;
    while (pos - U.off >= U.len) U = load_unit(V, line_off, ++i, out_cap);
    if (!U.fits) continue;
    const uint64_t byte = unit_byte(V, U, pos - U.off);
    if (k < 8) w0 |= byte << (8 * k); else w1 |= byte << (8 * (k - 8));
    m |= 1u << k;
  }
  v->w[0] = (uint32_t)w0; v->w[1] = (uint32_t)(w0 >> 32); v->w[2] = (uint32_t)w1; v->w[3] = (uint32_t)(w1 >> 32);
  return m;
}
// bytes of the whole records in front of out_cap
KJF_HD uint64_t written_bytes(const View &V, const uint64_t *line_off, uint64_t out_cap) {
  const uint64_t total = line_off[V.n_lines];
  if (total <= out_cap) return total;
  uint32_t lo = 0, hi = V.n_records;                          // the first record that ends behind out_cap
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (line_off[V.rec_line[mid + 1]] <= out_cap) lo = mid + 1; else hi = mid; }
  return lo < V.n_records ? line_off[V.rec_line[lo]] : total;
}

}  // namespace kjc

// what accmap.hip offers convert.hip: the pointers of a map as they are now (a map may grow between two conversions), the
// taxonomy it was built on and its device
#if defined(__HIPCC__)
struct kaiju_gpu_accmap;
struct kaiju_gpu_taxonomy;
#pragma GCC visibility push(hidden)
kjc::Map kj_accmap_view(const kaiju_gpu_accmap *m, const kaiju_gpu_taxonomy **tax, int *device);
int kj_accmap_rules(const kaiju_gpu_accmap *m);               // kRulesNr or kRulesRefSeq: what its lines were parsed by
#pragma GCC visibility pop
#endif

#endif  // KJ_CONVERT_H
