// kj_krona.h — kaiju2krona's text from the counts of a tally: the per-lane logic, for the device (krona.hip) and for the host
// (tests/emu/krona_emu.cpp drives the same functions pass by pass).  The tally of kj_tally.h keeps direct[] per slot of the
// tree; this writes one line per taxon that holds reads, "<count>\t<name>\t<name>...\n" with the lineage root first, without
// ever storing a lineage.
//
// The rules are those of kaiju2krona.cpp:116-190 of the reference, observed on the unmodified tool:
//   lines, byte 0, id, bad id, unknown id     exactly those of kj_tally.h (the tool's substr / stoul give the same set: "22abc",
//             "0022\r" and "22\t..." read 22; " 22", "+22", "-3", fewer than two tabs and values above 2^64 - 1 count
//             nowhere).  The tally's count pass is used as it is
//   -u        the number of non-empty lines whose byte 0 is not 'C', if above 0, is the last line: "<n>\tUnclassified\n"
//   a line    for every taxon t with direct > 0 that is a node and has a name of its own.  No node: nothing.  No name:
//             nothing (the tool warns on stderr)
//   own name  printed only if the PARENT'S ID has a name in names.dmp and, with -l, the rank of t is in the list.  The root is
//             its own parent and prints its name.  A genus whose family has no name prints its ancestors alone
//   ancestors walk id = parent(id) while id is a node and not its own parent.  Every parent that has a name (and, with -l, a
//             listed rank) goes in front of what is there: root first, the self-parent root included.  A parent without a name
//             is skipped and the walk goes on.  A parent that is NO node but has a name in names.dmp is printed without -l
//             and never with it; the walk ends behind it
//   -l        items between commas, empty ones dropped; the whole rank string is compared and "no rank" is a rank like any
//             other.  A list that no node satisfies gives lines of the count alone
//   format    the decimal count, "\t<name>" per kept name, "\n".  The tool's line order is that of its unordered_map; here it
//             is ascending slot order (that of kaiju_gpu_tally_result) with the Unclassified line last
//
// Tables, once per (tree, list), one lane per slot (a: a slot; named(a): the node has a name of its own):
//   keep[s]     no list, or the rank string of s (rank_of[] / rank_names of taxon_names.h) is listed
//   piece(a)    named(a) && keep[a] ? 1 + name_len(a) : 0           the bytes "\t<name>" of a as an ancestor
//   anc_len[s]  piece(s) + (nothing for a self-parent | anc_len[parent(s)] | the piece of a dangling parent - no node, but a name,
//               and no list)
//   own_ok[s]   the parent's id is named && keep[s]
// The piece of ancestor a lies at bytes [anc_len[parent(a)], anc_len[a]) of the lineage of every descendant, so the byte q of
// a lineage is found walking up from the taxon: the first a with anc_len[parent(a)] <= q (two loads per step, one walk per
// name and not per byte).
//
// Passes (every one works on independent units; the units of a pass may run in any order):
//   select   one lane per slot: direct summed over the tallies; flag[s] = it is above 0 and s gives a line.  Unnamed taxa and
//            their reads are counted
//   compact  prefix sum of flag[] (kj_lines.h), then sel[] / cnt[] dense in slot order; one lane appends the Unclassified line
//   len      one lane per line: digits + anc_len[parent] + own piece + 1
//   offsets  prefix sum of the lengths
//   write    one lane per 16 aligned bytes of the output (kj_lines.h: write_blocks); a line is written whole or not at all
//   finish   the info
#ifndef KJ_KRONA_H
#define KJ_KRONA_H

#include "kj_format_names.h"

namespace kjk {

using kjf::Bcd;
using kjf::Chunk;
using kjf::kChunk;
using kjn::kGenerated;
using kjn::kNone;

constexpr uint32_t kMaxTallies = KAIJU_GPU_KRONA_MAX_TALLIES;
constexpr uint64_t kMaxLineage = kjn::kMaxAnnotation;    // anc_len is below this
constexpr uint32_t kUnclassifiedLen = 13;                // "\tUnclassified"

struct Tab {
  const uint64_t *key;
  const uint32_t *parent, *name_pos, *name_len;
  const uint8_t *blob;
  const uint32_t *dang_pos, *dang_len;   // the name of a parent id that is no node (taxon_names.h)
  const uint8_t *dang_blob;
  const uint8_t *keep, *own_ok;          // built here
  const uint32_t *anc_len;
  uint32_t cap, has_list;
};

// ---- the tables (one lane per slot) -----------------------------------------------------------------------------------
KJF_HD bool named(const Tab &T, uint32_t a) { return T.key[a] != ~0ull && !(T.name_len[a] & kGenerated); }
// listed[k]: rank string k of the tree is in the list
KJF_HD uint8_t build_keep(const Tab &T, const uint16_t *rank_of, const uint8_t *listed, uint32_t s) {
  if (T.key[s] == ~0ull) return 0;
  return !T.has_list || listed[rank_of[s]] ? 1 : 0;
}
KJF_HD uint32_t piece(const Tab &T, uint32_t a) { return named(T, a) && T.keep[a] ? 1u + T.name_len[a] : 0u; }
// the piece of the parent of s where that is no node (0: it is one, or has no name, or there is a list)
KJF_HD uint32_t dang_piece(const Tab &T, uint32_t s) { return T.parent[s] == kNone && !T.has_list && T.dang_len[s] ? 1u + T.dang_len[s] : 0u; }
KJF_HD uint8_t build_own_ok(const Tab &T, uint32_t s) {
  if (T.key[s] == ~0ull || !T.keep[s]) return 0;
  const uint32_t p = T.parent[s];
  return (p == kNone ? T.dang_len[s] != 0 : named(T, p)) ? 1 : 0;
}
// The tree has no cycle but the self-parent (the loader refuses any other), so the walk ends.  64 bit: the caller refuses kMaxLineage
KJF_HD uint64_t build_anc_len(const Tab &T, uint32_t s) {
  if (T.key[s] == ~0ull) return 0;
  uint64_t sum = 0;
  for (uint32_t a = s;;) {
    sum += piece(T, a);
    const uint32_t p = T.parent[a];
    if (p == a) break;
    if (p == kNone) { sum += dang_piece(T, a); break; }
    a = p;
  }
  return sum;
}
// bytes of the names above s in its line
KJF_HD uint32_t above(const Tab &T, uint32_t s) {
  const uint32_t p = T.parent[s];
  return p == s ? 0u : p == kNone ? dang_piece(T, s) : T.anc_len[p];
}

// ---- select -----------------------------------------------------------------------------------------------------------
// does slot s with d reads give a line; *unnamed: it holds reads and has no name
KJF_HD uint32_t selects(const Tab &T, uint32_t s, uint64_t d, uint32_t *unnamed) {
  *unnamed = 0;
  if (!d || T.key[s] == ~0ull) return 0;
  if (!named(T, s)) { *unnamed = 1; return 0; }
  return 1;
}

// ---- len --------------------------------------------------------------------------------------------------------------
KJF_HD uint32_t own_len(const Tab &T, uint32_t s) { return T.own_ok[s] ? 1u + T.name_len[s] : 0u; }
// the line of slot s (kNone: the Unclassified line) with `count` reads
KJF_HD uint32_t line_len(const Tab &T, uint32_t s, uint64_t count) {
  const uint32_t d = kjf::digits_u64(count);
  return s == kNone ? d + kUnclassifiedLen + 1 : d + above(T, s) + own_len(T, s) + 1;
}

// ---- write ------------------------------------------------------------------------------------------------------------
struct Line {
  uint64_t off;
  uint32_t len, slot, digits, up;      // up: above(slot)
  Bcd bcd;
  bool fits;
};
KJF_HD Line load_line(const Tab &T, const uint64_t *line_off, const uint32_t *sel, const uint64_t *cnt, uint32_t r, uint64_t out_cap) {
  Line L;
  const uint64_t next = line_off[r + 1];
  L.off = line_off[r];
  L.len = (uint32_t)(next - L.off);
  L.slot = sel[r];
  L.digits = kjf::digits_u64(cnt[r]);
  L.bcd = kjf::to_bcd(cnt[r]);
  L.up = L.slot == kNone ? 0u : above(T, L.slot);
  L.fits = next <= out_cap;
  return L;
}
// one name of a lineage: bytes [start, end) of it, the tab in front included
struct Piece { uint32_t start, end; const uint8_t *name; };
// the piece that holds byte q of the lineage above slot s (q < above(T, s))
KJF_HD Piece locate(const Tab &T, uint32_t s, uint32_t q) {
  uint32_t a = T.parent[s];
  if (a == kNone) return Piece{0, dang_piece(T, s), T.dang_blob + T.dang_pos[s]};
  uint32_t base;
  for (;;) {                           // q < anc_len[a] holds, so the a it ends at has a piece
    const uint32_t p = T.parent[a];
    if (p == a) { base = 0; break; }
    if (p == kNone) {
      base = dang_piece(T, a);
      if (q < base) return Piece{0, base, T.dang_blob + T.dang_pos[a]};
      break;
    }
    base = T.anc_len[p];
    if (base <= q) break;
    a = p;
  }
  return Piece{base, base + 1u + T.name_len[a], T.blob + T.name_pos[a]};
}
KJF_HD uint32_t unclassified_byte(uint32_t i) { return (uint32_t)(uint8_t) "\tUnclassified"[i]; }
// byte p of the line (p < L.len); P: the piece of the last call (end == 0: none yet)
KJF_HD uint32_t line_byte(const Tab &T, const Line &L, uint32_t p, Piece *P) {
  if (p < L.digits) return '0' + kjf::bcd_digit(L.bcd, L.digits - 1 - p);
  if (p + 1 == L.len) return '\n';
  uint32_t q = p - L.digits;
  if (L.slot == kNone) return unclassified_byte(q);
  if (q >= L.up) {                     // the taxon's own name
    q -= L.up;
    return q ? T.blob[(uint64_t)T.name_pos[L.slot] + q - 1] : '\t';
  }
  if (q >= P->end || q < P->start) *P = locate(T, L.slot, q);
  q -= P->start;
  return q ? P->name[q - 1] : '\t';
}
// the bytes of chunk c of the output; r_lo, r_hi: block_records of the chunk's block.  Returns the mask of the bytes to
// write: those of lines that end at or in front of out_cap
KJF_HD uint32_t format_chunk(uint64_t c, const Tab &T, const uint64_t *line_off, const uint32_t *sel, const uint64_t *cnt, uint32_t r_lo, uint32_t r_hi,
                             uint64_t total, uint64_t out_cap, Chunk *v) {
  const uint64_t o = c * kChunk;
  *v = Chunk{{0, 0, 0, 0}};
  if (o >= total) return 0;
  uint32_t r = kjf::find_record(line_off, r_lo, r_hi, o);
  Line L = load_line(T, line_off, sel, cnt, r, out_cap);
  Piece P{0, 0, nullptr};
  uint64_t lo = 0, hi = 0;
  uint32_t m = 0;
  for (uint32_t k = 0; k < kChunk; k++) {
    const uint64_t pos = o + k;
    if (pos >= total) break;
    if (pos - L.off >= L.len) { L = load_line(T, line_off, sel, cnt, ++r, out_cap); P.end = 0; }   // (no line is empty)
    if (!L.fits) continue;
    const uint64_t byte = line_byte(T, L, (uint32_t)(pos - L.off), &P);
    if (k < 8) lo |= byte << (8 * k); else hi |= byte << (8 * (k - 8));
    m |= 1u << k;
  }
  v->w[0] = (uint32_t)lo; v->w[1] = (uint32_t)(lo >> 32); v->w[2] = (uint32_t)hi; v->w[3] = (uint32_t)(hi >> 32);
  return m;
}

// ---- finish -----------------------------------------------------------------------------------------------------------
// n_lines lines of line_off[]; the lines that fit are line_off[0 .. k] with line_off[k] <= out_cap
KJF_HD kaiju_gpu_krona_info make_info(const uint64_t *line_off, uint32_t n_lines, uint64_t out_cap, uint64_t unnamed_taxa, uint64_t unnamed_reads,
                                      uint64_t n_unclassified) {
  kaiju_gpu_krona_info o;
  const uint64_t total = line_off[n_lines];
  const uint32_t k = total <= out_cap ? n_lines : kjn::find_last_start(line_off, 0, n_lines + 1, out_cap);
  o.text_bytes = total;
  o.written_bytes = line_off[k];
  o.n_lines = n_lines;
  o.n_written = k;
  o.n_unnamed_taxa = unnamed_taxa;
  o.n_unnamed_reads = unnamed_reads;
  o.n_unclassified = n_unclassified;
  o.overflow = total > out_cap ? 1u : 0u;
  o.reserved = 0;
  return o;
}

}  // namespace kjk

// what format_names.hip and tally.hip offer krona.hip
#if defined(__HIPCC__)
struct kaiju_krona_source;             // taxon_names.h
const kaiju_krona_source *kj_fn_krona_source(const kaiju_gpu_taxon_names *names);
struct kj_tally_view {
  const kaiju_gpu_taxon_names *names;
  int device;
  const uint64_t *direct, *totals;     // [cap]; used, n_lines, the five counts of kj_tally.h
  hipEvent_t done;                     // behind the tally's last call; a reader records it behind itself
};
kj_tally_view kj_tally_view_of(const kaiju_gpu_tally *t);
#endif

#endif  // KJ_KRONA_H
