// kj_format_names.h — the three-column lines of kj_format.h with the column of kaiju-addTaxonNames behind them: the per-lane
// logic, for the device (format_names.hip) and for the host (tests/emu/format_names_emu.cpp drives the same functions).
//
// The rules are those of kaiju-addTaxonNames.cpp and util.cpp:123-192 of the reference, on the lines of kj_format.h:
//   'U' line    unchanged, or - with drop_unclassified - no line at all (a record of length 0)
//   'C' line    the taxon is no node of the tree, or the taxon itself has no name: unchanged (no tab, no column)
//               else line "\t" annotation "\n"
//   annotation  name   the name of the taxon
//               path   walk id = taxon; while id is a node and parent(id) != id: emit id; id = parent(id).  The names of the
//                      emitted ids root first, each followed by "; ".  An emitted id without a name prints "taxonid:<id>"
//               ranks  the same walk; an emitted id whose rank is in the list (and is not "no rank") overwrites the value of its
//                      rank, so the node nearest the root wins.  The values in list order, "NA" where none, each followed by "; "
//
// Tables (one slot per node of the tree, open addressing over the taxon id as in kj_core.h: tax_hash, linear probing):
//   key, parent (slot), name_pos / name_len into one blob of names, rank (index in the de-duplicated list)      from the host
//   path_len[s]   bytes of the path annotation of s: path_len[parent(s)] + entry_len(s) + 2, 0 for a node that is its own
//                 parent.  Byte q of the annotation of s belongs to the ancestor a with path_len[parent(a)] <= q < path_len[a]:
//                 walking from s towards the root, the first a whose parent's path_len is <= q.  No lineage is ever stored
//   rank_src[s][k], rank_len[s]   the slot whose name is the value of rank k for s (kNone: "NA"); the annotation's length
// "taxonid:<id>" is generated from the key of the slot (to_bcd of kj_format.h), never stored.
//
// Passes: those of kj_format.h.  Lines may be empty here, so the search takes the LAST record that starts at or before a
// byte, and the loop over the bytes of a chunk steps over empty lines.
#ifndef KJ_FORMAT_NAMES_H
#define KJ_FORMAT_NAMES_H

#include "kj_format.h"

namespace kjn {

using kjf::Bcd;
using kjf::Chunk;
using kjf::Params;
using kjf::kBlockBytes;
using kjf::kBlockLanes;
using kjf::kChunk;
using kjf::kScanBlock;

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kGenerated = 0x80000000u;             // in name_len: the node has no name, the length is that of "taxonid:<id>"
constexpr uint32_t kLenMask = 0x7fffffffu;
constexpr uint32_t kNoRank = 0xffu;
constexpr uint32_t kMaxRanks = KAIJU_NAMES_MAX_RANKS;    // distinct ranks of a list
constexpr uint32_t kMaxList = KAIJU_NAMES_MAX_LIST;      // items of a list
constexpr uint64_t kMaxAnnotation = 1ull << 24;          // an annotation is shorter than this
constexpr uint32_t kNamesExtra = kjf::kLineExtra + 1;    // a line is at most its name, 24 bytes, the tab and the annotation

enum { kWhyNone = 0, kWhyUnknown = 1, kWhyUnnamed = 2, kWhyDropped = 3 };

struct Tab {
  const uint64_t *key;
  const uint32_t *parent, *name_pos, *name_len;
  const uint8_t *rank, *blob;
  const uint32_t *path_len;            // [cap]             (path mode)
  const uint32_t *rank_src, *rank_len; // [cap * n_ranks], [cap]   (ranks mode)
  uint32_t cap_mask, mode, n_ranks, n_list;
  uint8_t list[kMaxList];
};

// tax_hash of kj_core.h, written out: this header is also compiled into host programs that do not see the kernels' header
// (the table is this file's own, so nothing but the spread of the ids depends on the two staying alike)
KJF_HD uint32_t hash_id(uint64_t id) {
  id ^= id >> 33; id *= 0xff51afd7ed558ccdULL; id ^= id >> 33; id *= 0xc4ceb9fe1a85ec53ULL; id ^= id >> 33;
  return (uint32_t)id;
}
// tax_find of kj_core.h; the id 2^64 - 1 marks an empty slot, is never a node (the loader refuses it) and is never found
KJF_HD uint32_t find_slot(const uint64_t *key, uint32_t cap_mask, uint64_t id) {
  uint32_t s = hash_id(id) & cap_mask;
  for (;;) {
    const uint64_t k = key[s];
    if (k == ~0ull) return kNone;
    if (k == id) return s;
    s = (s + 1) & cap_mask;
  }
}
KJF_HD uint32_t entry_len(const Tab &T, uint32_t s) { return T.name_len[s] & kLenMask; }

// ---- the tables built at upload (one lane per slot) ---------------------------------------------------------------
// The tree has no cycle but the self-parent (the loader refuses any other), so every walk ends.
KJF_HD uint64_t build_path_len(const Tab &T, uint32_t s) {
  uint64_t sum = 0;
  if (T.key[s] == ~0ull) return 0;
  for (uint32_t a = s; a != kNone && T.parent[a] != a; a = T.parent[a]) sum += (uint64_t)entry_len(T, a) + 2;
  return sum;
}
// src: the n_ranks words of slot s.  Returns the annotation's length
KJF_HD uint64_t build_ranks(const Tab &T, uint32_t s, uint32_t *src) {
  for (uint32_t k = 0; k < T.n_ranks; k++) src[k] = kNone;
  if (T.key[s] == ~0ull) return 0;
  for (uint32_t a = s; a != kNone && T.parent[a] != a; a = T.parent[a])
    if (T.rank[a] != kNoRank) src[T.rank[a]] = a;        // overwritten on the way up: the node nearest the root wins
  uint64_t sum = 0;
  for (uint32_t j = 0; j < T.n_list; j++) {
    const uint32_t a = src[T.list[j]];
    sum += (a == kNone ? 2ull : (uint64_t)entry_len(T, a)) + 2;
  }
  return sum;
}
KJF_HD uint32_t clamp32(uint64_t v) { return v > 0xffffffffull ? 0xffffffffu : (uint32_t)v; }

// ---- lengths ------------------------------------------------------------------------------------------------------
// the annotation of a 'C' line of `taxon`: its slot and length, or kNone (*why says which rule left the line unchanged)
KJF_HD uint32_t annotation_of(const Tab &T, uint64_t taxon, uint32_t *len, uint32_t *why) {
  *len = 0;
  const uint32_t s = find_slot(T.key, T.cap_mask, taxon);
  if (s == kNone) { *why = kWhyUnknown; return kNone; }
  if (T.name_len[s] & kGenerated) { *why = kWhyUnnamed; return kNone; }
  *why = kWhyNone;
  *len = T.mode == KAIJU_NAMES_NAME ? T.name_len[s] : T.mode == KAIJU_NAMES_PATH ? T.path_len[s] : T.rank_len[s];
  return s;
}
// length of the line of record r (0: no line); *taxon, *aslot: what pass `write` prints
KJF_HD uint32_t record_line(const kaiju_gpu_compact *recs, const uint64_t *off, const kaiju_gpu_name_span *names, uint32_t r, uint64_t bytes1,
                            const Params &P, const double *pw, const Tab &T, int drop, uint64_t *taxon, uint32_t *aslot, uint32_t *why) {
  const uint32_t base = kjf::record_line(recs, off, names, r, bytes1, P, pw, taxon);
  *aslot = kNone; *why = kWhyNone;
  if (*taxon == 0) {
    if (drop) { *why = kWhyDropped; return 0; }
    return base;
  }
  uint32_t alen;
  *aslot = annotation_of(T, *taxon, &alen, why);
  return *aslot == kNone ? base : base + 1 + alen;
}

// ---- write --------------------------------------------------------------------------------------------------------
// the largest r in [lo, hi) with line_off[r] <= o (line_off[lo] <= o).  line_off[] rises, but not strictly: of the records
// that start at the same byte all but the last are empty, and the last one is the answer
KJF_HD uint32_t find_last_start(const uint64_t *line_off, uint32_t lo, uint32_t hi, uint64_t o) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (line_off[mid] <= o) lo = mid; else hi = mid;
  }
  return lo;
}
// the records the bytes of block b of the output touch: [*r_lo, *r_hi).  lim: bytes the pass writes at most (> b * kBlockBytes)
KJF_HD void block_records(const uint64_t *line_off, uint32_t n, uint64_t b, uint64_t lim, uint32_t *r_lo, uint32_t *r_hi) {
  const uint64_t o0 = b * kBlockBytes, o1 = o0 + kBlockBytes < lim ? o0 + kBlockBytes : lim;
  *r_lo = find_last_start(line_off, 0, n, o0);
  *r_hi = find_last_start(line_off, 0, n, o1 - 1) + 1;
}
struct Line {
  kjf::Line L;              // the three columns; L.len: the whole line
  uint32_t base;            // bytes in front of the tab of the annotation (or of the newline)
  uint32_t aslot, alen;
};
KJF_HD Line load_line(const uint64_t *line_off, const uint64_t *tax, const uint32_t *aslot, const kaiju_gpu_name_span *names, uint32_t r, uint64_t bytes1,
                      uint64_t out_cap) {
  Line N;
  const uint64_t next = line_off[r + 1];
  const kaiju_gpu_name_span s = kjf::name_of(names, r, bytes1);
  N.L.off = line_off[r];
  N.L.len = (uint32_t)(next - N.L.off);
  N.L.taxon = tax[r];
  N.L.name_pos = s.pos; N.L.name_len = s.len;
  N.L.digits = kjf::digits_u64(N.L.taxon);
  N.L.bcd = N.L.taxon ? kjf::to_bcd(N.L.taxon) : Bcd{0, 0};
  N.L.fits = next <= out_cap;
  N.base = 3 + s.len + N.L.digits;
  N.aslot = aslot[r];
  N.alen = N.aslot == kNone || N.L.len == 0 ? 0 : N.L.len - N.base - 2;
  return N;
}
// one piece of an annotation: a name (or "taxonid:<id>", or "NA") and - but in name mode - "; " behind it
struct Entry {
  uint32_t a;               // the slot, kNone: "NA"
  uint32_t start, end;      // bytes [start, end) of the annotation
  uint32_t len;             // of the name
  uint32_t pos;             // of the name in the blob
  bool generated;
  Bcd bcd;
};
KJF_HD Entry make_entry(const Tab &T, uint32_t a, uint32_t start, uint32_t tail) {
  Entry E;
  E.a = a; E.start = start; E.pos = 0; E.generated = false; E.bcd = Bcd{0, 0};
  if (a == kNone) { E.len = 2; }
  else {
    E.len = entry_len(T, a);
    E.pos = T.name_pos[a];
    E.generated = (T.name_len[a] & kGenerated) != 0;
    if (E.generated) E.bcd = kjf::to_bcd(T.key[a]);
  }
  E.end = start + E.len + tail;
  return E;
}
// the piece that holds byte q of the annotation of slot s (q below its length)
KJF_HD Entry locate(const Tab &T, uint32_t s, uint32_t q) {
  if (T.mode == KAIJU_NAMES_NAME) return make_entry(T, s, 0, 0);
  if (T.mode == KAIJU_NAMES_PATH) {
    uint32_t a = s, base;
    for (;;) {
      const uint32_t p = T.parent[a];
      base = p == kNone ? 0u : T.path_len[p];
      if (base <= q) break;
      a = p;
    }
    return make_entry(T, a, base, 2);
  }
  uint32_t acc = 0;
  Entry E = make_entry(T, kNone, 0, 2);
  for (uint32_t j = 0; j < T.n_list; j++) {
    const uint32_t a = T.rank_src[(uint64_t)s * T.n_ranks + T.list[j]];
    const uint32_t l = (a == kNone ? 2u : entry_len(T, a)) + 2;
    if (q < acc + l || j + 1 == T.n_list) { E = make_entry(T, a, acc, 2); break; }
    acc += l;
  }
  return E;
}
KJF_HD uint32_t entry_byte(const Tab &T, const Entry &E, uint32_t q) {
  uint32_t p = q - E.start;
  if (p < E.len) {
    if (E.a == kNone) return p ? 'A' : 'N';
    if (!E.generated) return T.blob[(uint64_t)E.pos + p];
    if (p < 8) return (uint32_t)(0x3a64696e6f786174ull >> (8 * p)) & 255u;      // "taxonid:"
    return '0' + kjf::bcd_digit(E.bcd, E.len - 1 - p);
  }
  return p == E.len ? ';' : ' ';
}
// the bytes of chunk c of the output; r_lo, r_hi: block_records of the chunk's block.  Returns the mask of the bytes to
// write: those of lines that end at or in front of out_cap
KJF_HD uint32_t format_chunk(uint64_t c, const uint8_t *text, uint64_t bytes1, const kaiju_gpu_name_span *names, const uint64_t *line_off, const uint64_t *tax,
                             const uint32_t *aslot, const Tab &T, uint32_t r_lo, uint32_t r_hi, uint64_t total, uint64_t out_cap, Chunk *v) {
  const uint64_t o = c * kChunk;
  *v = Chunk{{0, 0, 0, 0}};
  if (o >= total) return 0;
  uint32_t r = find_last_start(line_off, r_lo, r_hi, o);
  Line N = load_line(line_off, tax, aslot, names, r, bytes1, out_cap);
  Entry E = make_entry(T, kNone, 0, 0);
  E.end = 0;                                               // (no piece yet)
  uint64_t lo = 0, hi = 0;
  uint32_t m = 0;
  for (uint32_t k = 0; k < kChunk; k++) {
    const uint64_t pos = o + k;
    if (pos >= total) break;
    while (pos - N.L.off >= N.L.len) { N = load_line(line_off, tax, aslot, names, ++r, bytes1, out_cap); E.end = 0; }
    if (!N.L.fits) continue;
    const uint32_t p = (uint32_t)(pos - N.L.off);
    uint32_t byte;
    if (p < N.base) byte = kjf::line_byte(text, N.L, p);
    else if (p + 1 == N.L.len) byte = '\n';
    else if (p == N.base) byte = '\t';
    else {
      const uint32_t q = p - N.base - 1;
      if (q >= E.end || q < E.start) E = locate(T, N.aslot, q);
      byte = entry_byte(T, E, q);
    }
    if (k < 8) lo |= (uint64_t)byte << (8 * k); else hi |= (uint64_t)byte << (8 * (k - 8));
    m |= 1u << k;
  }
  v->w[0] = (uint32_t)lo; v->w[1] = (uint32_t)(lo >> 32); v->w[2] = (uint32_t)hi; v->w[3] = (uint32_t)(hi >> 32);
  return m;
}

// ---- finish -------------------------------------------------------------------------------------------------------
KJF_HD kaiju_gpu_format_names_info make_info(uint64_t total, uint32_t n, uint32_t n_classified, uint32_t n_inexact, uint64_t out_cap, uint32_t n_unknown,
                                             uint32_t n_unnamed, uint32_t n_dropped) {
  kaiju_gpu_format_names_info o;
  o.text_bytes = total;
  o.n_records = n;
  o.n_classified = n_classified;
  o.overflow = total > out_cap ? 1u : 0u;
  o.n_inexact = n_inexact;
  o.n_unknown_taxon = n_unknown;
  o.n_unnamed_taxon = n_unnamed;
  o.n_dropped = n_dropped;
  o.reserved = 0;
  return o;
}

}  // namespace kjn

// what format_names.hip offers capi_text.hip
#if defined(__HIPCC__)
// queues every pass on `stream`; grows st.mem, st.written as after kj_format_launch.  Returns 0, or a kaiju_gpu_status with *err set
int kj_fn_launch(kjl::Lines &st, hipStream_t stream, const kjf::Params &P, const double *d_pw, const kaiju_gpu_compact *d_recs,
                 const uint64_t *d_off, uint32_t n, const void *d_text1, uint64_t bytes1, const kaiju_gpu_name_span *d_names,
                 const kaiju_gpu_taxon_names *names, int drop_unclassified, void *d_out, uint64_t out_cap, kaiju_gpu_format_names_info *d_info,
                 const char **err);
int kj_fn_device(const kaiju_gpu_taxon_names *names);
#endif

#endif  // KJ_FORMAT_NAMES_H
