// kj_merge.h — kaiju-mergeOutputs on two texts of output lines: the per-lane logic, for the device (merge.hip) and for the
// host (tests/emu/merge_emu.cpp drives the same functions pass by pass).
//
// The rules are those of kaiju-mergeOutputs.cpp:110-295, :355-399 and util.cpp:42-77 of the reference (getline on both files,
// find('\t'), find_first_not_of, stod, stoul, calc_lca, is_ancestor), observed on the unmodified tool:
//   lines     a line ends at '\n'; the last one may lack it.  Every other byte, '\r' and NUL included, is a byte of the line.
//             Line k of text 1 pairs with line k of text 2.  An empty line is a line (and stops the run: byte 0)
//   stop      the first pair that fails ends the run: the pairs in front of it are written, nothing at or behind it is.  The
//             checks of a pair in order: line 1 (byte 0 is 'C' / 'U', two tabs, the id / score column), text 2 has the line,
//             the same on line 2, the names (bytes between tab 1 and tab 2) are equal byte for byte
//   parse     without use_score, or on a 'U' line: the id is the run of [0-9] behind tab 2 (it may be empty, what follows it
//             is ignored; tab 2 as the last byte stops).  With use_score on a 'C' line: tab 3 must exist, the id is every byte
//             between tab 2 and tab 3, the score the run of [.0-9] behind tab 3 (may be empty; tab 3 as the last byte stops)
//   output    U,U "U\t" name "\t0\n" (never a score);  C,U / U,C "C\t" name "\t" id ["\t" score] "\n" of the 'C' side;
//             C,C: equal id texts: id1, the score text of the larger value (score1 on a tie); else different values: id and
//             score of the larger value; else score1 and the id by the conflict mode: id1, id2, mlca(id1, id2) printed as a
//             number, or - lowest - id2 if anc(id1, id2), id1 if anc(id2, id1), else mlca.  An mlca of 0 prints id1's text
//   number    of an id, stoul: leading " \t\n\v\f\r", one '+' or '-', decimal digits; no digit or a magnitude above 2^64 - 1
//             is bad ('-' negates modulo 2^64).  A bad number on either side: mlca 0, anc false
//   mlca      neither a node: 0; one a node: that one; both: x = parent(n2), while x is neither n1 nor an ancestor of n1 and
//             x != parent(x): x = parent(x).  (The tool's own rule, not lca_from_ids: a node and its ancestor give the
//             ancestor's parent.)  Here by depth: n1's path is raised to the depth of x and compared - no set
//   anc(a, b) both nodes, and a == b or a on b's parent chain
//   score     stod of a [.0-9]* text: the longest prefix digits[.digits] with a digit; none: 0.  Values are compared as
//             decimals (exponent of the first significant digit, fifteen digits from it on): equal to the comparison of the
//             doubles when every value is 0 / invalid, at or above 10^309 (stod: out of range, 0), or has at most 15 digits
//             from its first to its last non-zero digit and lies in [10^-300, 10^300).  Anything else on a C,C pair is the
//             stop kStopScoreWide: never a guess
//
// Passes (every one works on independent units; the units of a pass may run in any order):
//   lines   that of kj_ingest.h on both texts
//   plan    by one lane: the lines of both texts, the pairs, the bytes used
//   pair    one lane per pair: parse_line twice, resolve_pair: rec[pair] and the smallest pair index that stops
//   count   the pairs in front of the stop: olen[pair], the counters
//   offsets kjl::launch_offsets over olen[]
//   write   kjl::write_blocks over merge_chunk: spans of the two texts and the digits of a number, nothing else
//   finish  kaiju_gpu_merge_info
//
// Every walk in the tree is bounded by the depth stored with the slot, whatever the tree looks like; a parent that is no node
// makes its child a root.  Positions inside a text fit 32 bits (kji::kMaxBytes); output offsets are 64 bit.
#ifndef KJ_MERGE_H
#define KJ_MERGE_H

#include "kj_format.h"
#include "kj_ingest.h"

namespace kjm {

using kjf::Chunk;
using kjf::kChunk;

static_assert(kji::kChunk == kjf::kChunk && kji::kTileBytes == kjf::kBlockBytes, "the chunks of the input are those of the output");

enum { kModeFirst = KAIJU_GPU_MERGE_FIRST, kModeSecond = KAIJU_GPU_MERGE_SECOND, kModeLca = KAIJU_GPU_MERGE_LCA, kModeLowest = KAIJU_GPU_MERGE_LOWEST };
enum {
  kStopNone = KAIJU_GPU_MERGE_STOP_NONE, kStop1Class = KAIJU_GPU_MERGE_STOP_1_CLASS, kStop1Tabs = KAIJU_GPU_MERGE_STOP_1_TABS,
  kStop1Column = KAIJU_GPU_MERGE_STOP_1_COLUMN, kStopShort2 = KAIJU_GPU_MERGE_STOP_2_SHORT, kStop2Class = KAIJU_GPU_MERGE_STOP_2_CLASS,
  kStop2Tabs = KAIJU_GPU_MERGE_STOP_2_TABS, kStop2Column = KAIJU_GPU_MERGE_STOP_2_COLUMN, kStopNames = KAIJU_GPU_MERGE_STOP_NAMES,
  kStopScoreWide = KAIJU_GPU_MERGE_STOP_SCORE_WIDE
};
enum { kKindU = 0, kKindC1 = 1, kKindC2 = 2, kKindC12 = 3, kKindCount = 4 };
enum { kIdText1 = 0, kIdText2 = 1, kIdNumber = 2 };
enum { kScoreNone = 0, kScoreText1 = 1, kScoreText2 = 2 };
constexpr uint32_t kNoSlot = 0xffffffffu;
constexpr uint32_t kNoStop = 0xffffffffu;
constexpr uint64_t kMaxTenth = 1844674407370955161ull;   // (2^64 - 1) / 10; 2^64 - 1 ends in 5

// kj::DevTaxonomy of kj_core.h, written out: this header is also compiled into host programs that do not see the kernels'
// header.  key == nullptr: the empty tree
struct Tree {
  const uint64_t *key;          // [cap] taxon id of the slot, ~0 = empty
  const uint32_t *parent_slot;  // [cap] ~0: the parent is no node
  const uint32_t *depth;        // [cap]
  uint32_t cap_mask;
};
KJF_HD uint32_t tax_hash(uint64_t id) {
  id ^= id >> 33; id *= 0xff51afd7ed558ccdULL; id ^= id >> 33; id *= 0xc4ceb9fe1a85ec53ULL; id ^= id >> 33;
  return (uint32_t)id;
}
// the slot of id; 2^64 - 1 marks an empty slot and is never a node
KJF_HD uint32_t find_slot(const Tree &t, uint64_t id) {
  if (!t.key || id == ~0ull) return kNoSlot;
  uint32_t s = tax_hash(id) & t.cap_mask;
  for (;;) {
    const uint64_t k = t.key[s];
    if (k == id) return s;
    if (k == ~0ull) return kNoSlot;
    s = (s + 1) & t.cap_mask;
  }
}
KJF_HD uint32_t up(const Tree &t, uint32_t s) { const uint32_t p = t.parent_slot[s]; return p == kNoSlot ? s : p; }

// ---- parse --------------------------------------------------------------------------------------------------------
struct Parsed {
  uint32_t why;                 // kStopNone, or kStop1Class / kStop1Tabs / kStop1Column (of either line)
  uint32_t classified;          // byte 0 is 'C'
  uint32_t name, name_len, id, id_len, score, score_len;   // spans of the text; score_len is 0 without a score column
  bool has_score;
};
// the positions of the first `want` '\t' of text[a, e), a < e: 16 aligned bytes at a time (text: the contract of kji::load_chunk)
KJF_HD uint32_t find_tabs(const uint8_t *text, uint64_t a, uint64_t e, uint32_t want, uint64_t *tab) {
  uint32_t seen = 0;
  for (uint64_t c = a / kChunk; c * kChunk < e && seen < want; c++)
    for (uint32_t m = kji::eq_mask(kji::load_chunk(text, c), '\t') & kji::range_mask(c * kChunk, a, e); m && seen < want; m &= m - 1)
      tab[seen++] = c * kChunk + kji::ctz16(m);
  return seen;
}
// the end of the run of [0-9] (dot: [.0-9]) at text[p, e)
KJF_HD uint64_t run_end(const uint8_t *text, uint64_t p, uint64_t e, bool dot) {
  for (; p < e; p++) {
    const uint32_t b = text[p];
    if (b - '0' > 9u && !(dot && b == '.')) break;
  }
  return p;
}
KJF_HD Parsed parse_line(const uint8_t *text, uint64_t a, uint64_t e, int use_score) {
  Parsed P{};
  if (a >= e || (text[a] != 'C' && text[a] != 'U')) { P.why = kStop1Class; return P; }
  P.classified = text[a] == 'C' ? 1u : 0u;
  P.has_score = use_score && P.classified;
  uint64_t tab[3];
  const uint32_t seen = find_tabs(text, a, e, P.has_score ? 3u : 2u, tab);
  if (seen < 2) { P.why = kStop1Tabs; return P; }
  P.name = (uint32_t)(tab[0] + 1);
  P.name_len = (uint32_t)(tab[1] - tab[0] - 1);
  P.id = (uint32_t)(tab[1] + 1);
  if (P.has_score) {
    if (seen < 3 || tab[2] + 1 == e) { P.why = kStop1Column; return P; }
    P.id_len = (uint32_t)(tab[2] - tab[1] - 1);
    P.score = (uint32_t)(tab[2] + 1);
    P.score_len = (uint32_t)(run_end(text, tab[2] + 1, e, true) - (tab[2] + 1));
  } else {
    if (tab[1] + 1 == e) { P.why = kStop1Column; return P; }
    P.id_len = (uint32_t)(run_end(text, tab[1] + 1, e, false) - (tab[1] + 1));
  }
  return P;
}

// ---- resolve ------------------------------------------------------------------------------------------------------
KJF_HD bool same_bytes(const uint8_t *x, const uint8_t *y, uint32_t n) {
  uint32_t k = 0;
  for (; k + 8 <= n; k += 8) {
    uint64_t u, v;
    __builtin_memcpy(&u, x + k, 8);
    __builtin_memcpy(&v, y + k, 8);
    if (u != v) return false;
  }
  for (; k < n; k++) if (x[k] != y[k]) return false;
  return true;
}
// stoul of text[p, p + n): false when it is bad
KJF_HD bool id_number(const uint8_t *text, uint32_t p, uint32_t n, uint64_t *id) {
  const uint8_t *s = text + p, *e = s + n;
  while (s < e && (*s == ' ' || (*s >= '\t' && *s <= '\r'))) s++;
  bool neg = false;
  if (s < e && (*s == '+' || *s == '-')) { neg = *s == '-'; s++; }
  uint64_t acc = 0;
  bool any = false, over = false;
  for (; s < e; s++) {
    const uint32_t d = (uint32_t)*s - '0';
    if (d > 9) break;
    any = true;
    if (acc > kMaxTenth || (acc == kMaxTenth && d > 5)) over = true;
    acc = acc * 10 + d;
  }
  *id = neg ? 0 - acc : acc;
  return any && !over;
}
// the value of a score text as a decimal: kind 0 zero (or invalid, or out of the range of a double), 1 a value 0.m * 10^(exp + 1)
// with the fifteen digits m, 2 outside the domain
struct Score { uint32_t kind; int32_t exp; uint64_t mant; };
enum { kScoreZero = 0, kScoreValue = 1, kScoreWide = 2 };
KJF_HD Score score_value(const uint8_t *text, uint32_t p, uint32_t n) {
  bool dot = false, found = false;
  uint64_t int_digits = 0, k = 0, first = 0, last = 0, mant = 0;
  uint32_t taken = 0;
  for (uint32_t q = 0; q < n; q++) {
    const uint32_t b = text[(uint64_t)p + q];
    if (b == '.') { if (dot) break; dot = true; continue; }
    const uint32_t d = b - '0';
    if (d > 9) break;
    if (!dot) int_digits++;
    if (d && !found) { found = true; first = k; }
    if (d) last = k;
    if (found && k - first < 15) { mant = mant * 10 + d; taken++; }
    k++;
  }
  if (!found) return Score{kScoreZero, 0, 0};
  const int64_t exp = (int64_t)int_digits - 1 - (int64_t)first;        // the value lies in [10^exp, 10^(exp + 1))
  if (exp >= 309) return Score{kScoreZero, 0, 0};                      // above the largest double
  if (last - first >= 15 || exp >= 300 || exp < -300) return Score{kScoreWide, 0, 0};
  for (; taken < 15; taken++) mant *= 10;
  return Score{kScoreValue, (int32_t)exp, mant};
}
// -1, 0, 1: x below, equal to, above y (neither is kScoreWide)
KJF_HD int score_cmp(const Score &x, const Score &y) {
  if (x.kind != y.kind) return x.kind > y.kind ? 1 : -1;
  if (x.kind == kScoreZero) return 0;
  if (x.exp != y.exp) return x.exp > y.exp ? 1 : -1;
  return x.mant == y.mant ? 0 : x.mant > y.mant ? 1 : -1;
}
// calc_lca of slots s1, s2 (either may be kNoSlot) of ids n1, n2
KJF_HD uint64_t mlca(const Tree &t, uint32_t s1, uint32_t s2, uint64_t n1, uint64_t n2) {
  if (s1 == kNoSlot && s2 == kNoSlot) return 0;
  if (s1 == kNoSlot) return n2;
  if (s2 == kNoSlot) return n1;
  uint32_t x = up(t, s2), y = s1;
  uint32_t dx = t.depth[x], dy = t.depth[y];
  for (;;) {
    while (dy > dx) { y = up(t, y); dy--; }                            // the one node of n1's path that can be x
    if ((dy == dx && y == x) || x == up(t, x) || dx == 0) return t.key[x];
    x = up(t, x); dx--;
  }
}
KJF_HD bool anc(const Tree &t, uint32_t sa, uint32_t sb) {
  if (sa == kNoSlot || sb == kNoSlot) return false;
  const uint32_t da = t.depth[sa];
  for (uint32_t db = t.depth[sb]; db > da; db--) sb = up(t, sb);
  return sa == sb;
}

struct Rec {
  uint32_t name, name_len;      // of text 1
  uint32_t id, id_len;          // a span of text 1 or 2; kIdNumber: the low and the high half of the number
  uint32_t score, score_len;
  uint32_t flags;               // kind | id source << 2 | score source << 4 | why << 8
  uint32_t pad;
};
KJF_HD uint32_t rec_kind(const Rec &R) { return R.flags & 3u; }
KJF_HD uint32_t rec_id_src(const Rec &R) { return (R.flags >> 2) & 3u; }
KJF_HD uint32_t rec_score_src(const Rec &R) { return (R.flags >> 4) & 3u; }
KJF_HD uint32_t rec_why(const Rec &R) { return R.flags >> 8; }
KJF_HD uint64_t rec_number(const Rec &R) { return (uint64_t)R.id_len << 32 | R.id; }
KJF_HD uint32_t rec_id_len(const Rec &R) { return rec_id_src(R) == kIdNumber ? kjf::digits_u64(rec_number(R)) : R.id_len; }
// bytes of the line: 'C' '\t' name '\t' id ['\t' score] '\n'
KJF_HD uint64_t rec_olen(const Rec &R) {
  return 2 + (uint64_t)R.name_len + 1 + rec_id_len(R) + (rec_score_src(R) ? 1 + (uint64_t)R.score_len : 0) + 1;
}
KJF_HD Rec stop_rec(uint32_t why) { Rec R{}; R.flags = why << 8; return R; }
KJF_HD void take(Rec &R, const Parsed &P, uint32_t side, bool id, bool score) {
  if (id) { R.id = P.id; R.id_len = P.id_len; R.flags |= (side == 1 ? kIdText1 : kIdText2) << 2; }
  if (score && P.has_score) { R.score = P.score; R.score_len = P.score_len; R.flags |= (side == 1 ? kScoreText1 : kScoreText2) << 4; }
}
// the pair of line [a1, e1) of text 1 and [a2, e2) of text 2; have2: text 2 has the line
KJF_HD Rec resolve_pair(const uint8_t *text1, uint64_t a1, uint64_t e1, const uint8_t *text2, uint64_t a2, uint64_t e2, bool have2,
                        const Tree &t, int mode, int use_score) {
  const Parsed P1 = parse_line(text1, a1, e1, use_score);
  if (P1.why) return stop_rec(P1.why);
  if (!have2) return stop_rec(kStopShort2);
  const Parsed P2 = parse_line(text2, a2, e2, use_score);
  if (P2.why) return stop_rec(P2.why + (kStop2Class - kStop1Class));
  if (P1.name_len != P2.name_len || !same_bytes(text1 + P1.name, text2 + P2.name, P1.name_len)) return stop_rec(kStopNames);
  Rec R{};
  R.name = P1.name; R.name_len = P1.name_len;
  if (!P1.classified && !P2.classified) {                              // "U\t" name "\t0\n"
    R.flags = kKindU | kIdNumber << 2;
    return R;
  }
  if (!P2.classified) { R.flags = kKindC1; take(R, P1, 1, true, true); return R; }
  if (!P1.classified) { R.flags = kKindC2; take(R, P2, 2, true, true); return R; }
  R.flags = kKindC12;
  int cmp = 0;                                                         // score 1 against score 2
  if (use_score) {
    const Score v1 = score_value(text1, P1.score, P1.score_len), v2 = score_value(text2, P2.score, P2.score_len);
    if (v1.kind == kScoreWide || v2.kind == kScoreWide) return stop_rec(kStopScoreWide);
    cmp = score_cmp(v1, v2);
  }
  if (P1.id_len == P2.id_len && same_bytes(text1 + P1.id, text2 + P2.id, P1.id_len)) {
    take(R, P1, 1, true, false);
    if (cmp < 0) take(R, P2, 2, false, true); else take(R, P1, 1, false, true);
    return R;
  }
  if (cmp) {
    if (cmp > 0) take(R, P1, 1, true, true); else take(R, P2, 2, true, true);
    return R;
  }
  take(R, P1, 1, false, true);
  if (mode == kModeFirst) { take(R, P1, 1, true, false); return R; }
  if (mode == kModeSecond) { take(R, P2, 2, true, false); return R; }
  uint64_t n1 = 0, n2 = 0, L = 0;
  if (id_number(text1, P1.id, P1.id_len, &n1) && id_number(text2, P2.id, P2.id_len, &n2)) {
    const uint32_t s1 = find_slot(t, n1), s2 = find_slot(t, n2);
    if (mode == kModeLowest && anc(t, s1, s2)) { take(R, P2, 2, true, false); return R; }
    if (mode == kModeLowest && anc(t, s2, s1)) { take(R, P1, 1, true, false); return R; }
    L = mlca(t, s1, s2, n1, n2);
  }
  if (L == 0) { take(R, P1, 1, true, false); return R; }
  R.id = (uint32_t)L; R.id_len = (uint32_t)(L >> 32); R.flags |= kIdNumber << 2;
  return R;
}

// ---- write --------------------------------------------------------------------------------------------------------
struct Line {
  uint64_t off, olen;
  Rec R;
  const uint8_t *id_text, *score_text;
  uint32_t id_len;
  kjf::Bcd bcd;
  bool fits;
};
KJF_HD Line load_line(const uint8_t *text1, const uint8_t *text2, const Rec *rec, const uint64_t *out_off, uint32_t r, uint64_t out_cap) {
  Line L;
  const uint64_t next = out_off[r + 1];
  L.off = out_off[r];
  L.olen = next - L.off;
  L.R = rec[r];
  L.id_len = rec_id_len(L.R);
  const uint32_t src = rec_id_src(L.R);
  L.id_text = src == kIdNumber ? nullptr : (src == kIdText1 ? text1 : text2) + L.R.id;
  L.bcd = src == kIdNumber ? kjf::to_bcd(rec_number(L.R)) : kjf::Bcd{0, 0};
  L.score_text = (rec_score_src(L.R) == kScoreText2 ? text2 : text1) + L.R.score;
  L.fits = next <= out_cap;
  return L;
}
// byte p of the line (p < L.olen)
KJF_HD uint32_t line_byte(const uint8_t *text1, const Line &L, uint64_t p) {
  if (p == 0) return rec_kind(L.R) == kKindU ? 'U' : 'C';
  if (p == 1) return '\t';
  if (p + 1 == L.olen) return '\n';
  p -= 2;
  if (p < L.R.name_len) return text1[(uint64_t)L.R.name + p];
  p -= L.R.name_len;
  if (p == 0) return '\t';
  p -= 1;
  if (p < L.id_len) return L.id_text ? L.id_text[p] : '0' + kjf::bcd_digit(L.bcd, L.id_len - 1 - (uint32_t)p);
  p -= L.id_len;
  if (p == 0) return '\t';
  return L.score_text[p - 1];
}
// the bytes of chunk c of the output; r_lo, r_hi: the pairs the chunk's block touches.  Returns the mask of the bytes to
// write: those of lines that end at or in front of out_cap
KJF_HD uint32_t merge_chunk(uint64_t c, const uint8_t *text1, const uint8_t *text2, const Rec *rec, const uint64_t *out_off, uint32_t r_lo, uint32_t r_hi,
                            uint64_t total, uint64_t out_cap, Chunk *v) {
  const uint64_t o = c * kChunk;
  *v = Chunk{{0, 0, 0, 0}};
  if (o >= total) return 0;
  uint32_t r = kjf::find_record(out_off, r_lo, r_hi, o);               // (no line is empty: out_off[] rises strictly)
  Line L = load_line(text1, text2, rec, out_off, r, out_cap);
  uint64_t lo = 0, hi = 0;
  uint32_t m = 0;
  for (uint32_t k = 0; k < kChunk; k++) {
    const uint64_t pos = o + k;
    if (pos >= total) break;
    if (pos - L.off >= L.olen) L = load_line(text1, text2, rec, out_off, ++r, out_cap);
    if (!L.fits) continue;
    const uint64_t byte = line_byte(text1, L, pos - L.off);
    if (k < 8) lo |= byte << (8 * k); else hi |= byte << (8 * (k - 8));
    m |= 1u << k;
  }
  v->w[0] = (uint32_t)lo; v->w[1] = (uint32_t)(lo >> 32); v->w[2] = (uint32_t)hi; v->w[3] = (uint32_t)(hi >> 32);
  return m;
}

// ---- plan, finish -------------------------------------------------------------------------------------------------
// lines of a text with n_nl '\n' bytes: without `final` only those a '\n' ends; *sentinel: line_start[n_lines]
KJF_HD uint32_t merge_line_count(const uint8_t *text, uint64_t bytes, uint32_t n_nl, uint32_t last_nl_end, int final, uint32_t *sentinel) {
  if (final) return kji::line_count(text, bytes, n_nl, sentinel);
  *sentinel = last_nl_end;
  return n_nl;
}
// pairs the pair pass looks at.  A line that passes its checks has four bytes at least ("C\t\t7"), so a run without a stop
// in its first k pairs has used 4 k bytes of either text: the first stop, if any, lies in front of min(bytes) / 4 + 2
KJF_HD uint32_t pair_cap(uint64_t bytes1, uint64_t bytes2) { return (uint32_t)((bytes1 < bytes2 ? bytes1 : bytes2) / 4 + 2); }
KJF_HD uint32_t pairs_looked_at(uint32_t n1, uint32_t n2, int final, uint64_t bytes1, uint64_t bytes2) {
  const uint32_t n = final ? n1 : (n1 < n2 ? n1 : n2), cap = pair_cap(bytes1, bytes2);
  return n < cap ? n : cap;
}
// count[]: written pairs per kind
KJF_HD kaiju_gpu_merge_info make_info(uint64_t total, uint64_t used1, uint64_t used2, uint32_t n1, uint32_t n2, uint32_t n_out, uint32_t stop,
                                      uint32_t stop_why, const uint32_t *count, uint32_t more_in_2, uint64_t out_cap) {
  kaiju_gpu_merge_info o;
  o.text_bytes = total;
  o.used1 = used1; o.used2 = used2;
  o.n_pairs = n1 < n2 ? n1 : n2;
  o.count = (uint64_t)n_out + (stop != kNoStop ? 1 : 0);
  o.count_c1 = (uint64_t)count[kKindC1] + count[kKindC12];
  o.count_c2 = (uint64_t)count[kKindC2] + count[kKindC12];
  o.count_c12 = count[kKindC12];
  o.count_c3 = (uint64_t)count[kKindC1] + count[kKindC2] + count[kKindC12];
  o.count_c1_not_c2 = count[kKindC1];
  o.count_c2_not_c1 = count[kKindC2];
  o.stop_pair = stop != kNoStop ? stop : ~0ull;
  o.stop_why = stop != kNoStop ? stop_why : (uint32_t)kStopNone;
  o.more_in_2 = stop != kNoStop ? 0u : more_in_2;
  o.overflow = total > out_cap ? 1u : 0u;
  o.reserved = 0;
  return o;
}
// an out_cap that cannot overflow: a line of the output is at most the two lines it comes from and the twenty digits of a number
KJF_HD uint64_t bound(uint64_t bytes1, uint64_t bytes2) { return bytes1 + bytes2 + 2 + 20 * (uint64_t)pair_cap(bytes1, bytes2); }

}  // namespace kjm

#endif  // KJ_MERGE_H
