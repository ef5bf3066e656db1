// kj_gbk.h — kaiju-gbk2faa on blocks of GenBank flat-file text: the per-lane logic, for the device (gbk.hip) and for the host
// (tests/emu/gbk_emu.cpp drives the same functions pass by pass).
//
// The rules are those of util/kaiju-gbk2faa.pl of the reference (one chain of if / elsif over regular expressions per line),
// observed on the unmodified script (tests/golden/gbk/):
//   lines     a line ends at '\n', the last one may lack it; '\r' and NUL are bytes of the line.  Every line has exactly one
//             kind, by the first of the tests below that holds
//   kind 1    taxon: the line holds `/db_xref="taxon:`, one or more ASCII digits, `"`.  The leftmost occurrence at which the whole
//             pattern matches counts (`/db_xref="taxon:12a" /db_xref="taxon:13"` gives 13).  The taxon is the digit string as
//             written (leading zeros stay, any length).  Nothing is printed, the state below does not change
//   kind 2    protein id: `/protein_id="`, one or more bytes that are no `"`, `"`; the leftmost occurrence that matches
//             (`/protein_id="" /protein_id="P2"` gives P2).  Nothing is printed, the state does not change
//   kind 3    whole translation: a byte of " \t\n\v\f\r" directly in front of `/translation="`, then one or more bytes that are
//             no `"`, then `"`; the leftmost occurrence that matches.  Printed: the header, the filtered capture, '\n'.  The state
//             does not change (inside a translation the following lines keep printing)
//   kind 4    translation opens: the same prefix, then one or more bytes that are no `"` up to the end of the line.  Printed as
//             kind 3; the state becomes "inside".  Inside a translation it prints a second header
//   kind 5    every other line.  Inside a translation the filtered line and '\n' are printed (an empty line prints "\n", bytes
//             behind a `"` are printed too), and a line that holds a `"` makes the state "outside".  Outside: nothing
//   header    '>', the protein id seen last (nothing if none was seen), '_', the taxon seen last, '\n'.  A kind 3 / 4 line before
//             any taxon ends the script with an error (status 255); no output can precede it, so the file is empty
//   filter    'B' -> 'D', 'Z' -> 'E' (upper case only), then exactly the bytes of ARNDCQEGHILKMFPSTWYV in either case are kept
// In terms of single bytes: every pattern holds a `"`, so a line without one is kind 5.  Let q be the byte behind the `"` of an
// occurrence and L the last `"` of the line.  `[^"]+"` matches at q iff q is no `"` and L > q, and the capture ends at the first
// `"` behind q.  `[^"]+$` matches at q iff q lies in the line and no `"` follows, that is L == q - 1: only the occurrence whose
// own `"` is the last of the line can open a translation.
//
// The state.  The script keeps $t = "inside a translation": a kind 4 line sets it, a kind 5 line with a `"` clears it when it is
// set.  Clearing a flag that is clear changes nothing, so the condition can be dropped: call a kind 4 line a "set" event and
// every kind 5 line with a `"` a "clear" event, whether $t was set or not.  Then $t in front of line i is decided by the last
// event in front of i alone - set: the flag was set and nothing touched it since; clear: it was cleared or already clear;
// none: the value carried in.  "The last event in front of line i" is an exclusive maximum-scan over the lines of
// 2 (i + 1) + set for the event lines and 0 for the rest.  The taxon and the protein id seen last are the same scan over i + 1
// for the kind 1 and kind 2 lines.  A result of 0 means "carried in from the blocks before": struct Carry and its two strings.
//
// Passes (independent units each; the units of a pass may run in any order):
//   lines    that of kj_ingest.h
//   kinds    one lane per line: the `"` of the line in 16-byte chunks (none: kind 5, nearly every line of a real file), else the
//            '/' of the line against the three literals.  kind[], cap_a[], cap_e[]
//   scans    the three maximum-scans: tax_src[], pid_src[] (line + 1, 0: carried) and in_t[]
//   lengths  one lane per line: bytes of its header line and of its sequence line; the first line that lacks a taxon
//   offsets  kjl::launch_offsets;  write: kjl::write_blocks over gbk_chunk;  finish: kaiju_gpu_gbk_info and the carried state
// A line is one lane in kinds and lengths, and the n-th kept byte of a span is found from the span's start: a line of L bytes
// costs L per lane there and L^2 / 256 bytes read in the write pass.  GenBank lines have 80 bytes.
#ifndef KJ_GBK_H
#define KJ_GBK_H

#include "kj_format.h"
#include "kj_ingest.h"

namespace kjg {

using kjf::Chunk;
using kjf::kChunk;

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint64_t kNoPos = ~0ull;
enum : uint32_t { kTaxon = 1, kProteinId = 2, kWhole = 3, kOpens = 4, kOther = 5 };
constexpr uint32_t kKindMask = 7, kQuoteBit = 8;       // of kind[]: the line holds a `"`

// ---- the kind of a line ---------------------------------------------------------------------------------------------
KJF_HD bool is_space(uint32_t b) { return b == ' ' || (b >= '\t' && b <= '\r'); }      // " \t\n\v\f\r"
KJF_HD bool is_digit(uint32_t b) { return b - '0' < 10u; }
// text[p, e) starts with lit (N - 1 bytes)
template <uint32_t N>
KJF_HD bool lit_at(const uint8_t *text, uint64_t p, uint64_t e, const char (&lit)[N]) {
  if (e - p < N - 1) return false;
#pragma unroll
  for (uint32_t k = 0; k < N - 1; k++)
    if (text[p + k] != (uint8_t)lit[k]) return false;
  return true;
}
KJF_HD uint32_t top16(uint32_t m) { return 31u - (uint32_t)__builtin_clz(m); }
// the last `"` of [a, e), kNoPos without one
KJF_HD uint64_t last_quote(const uint8_t *text, uint64_t a, uint64_t e) {
  uint64_t last = kNoPos;
  for (uint64_t c = a / kChunk; c * kChunk < e; c++) {
    const uint32_t m = kji::eq_mask(kji::load_chunk(text, c), '"') & kji::range_mask(c * kChunk, a, e);
    if (m) last = c * kChunk + top16(m);
  }
  return last;
}
KJF_HD uint64_t next_quote(const uint8_t *text, uint64_t q, uint64_t e) {
  while (q < e && text[q] != '"') q++;
  return q;
}
struct LineKind { uint32_t kind, cap_a, cap_e; };      // kind with kQuoteBit; the capture of kinds 1 to 4
// line [a, e)
KJF_HD LineKind classify(const uint8_t *text, uint64_t a, uint64_t e) {
  LineKind none{kOther, 0, 0};
  const uint64_t L = last_quote(text, a, e);
  if (L == kNoPos) return none;
  LineKind pid = none, whole = none, opens = none;
  for (uint64_t p = a; p + 13 < e; p++) {                    // (the shortest pattern has 15 bytes)
    if (text[p] != '/') continue;
    if (lit_at(text, p, e, "/db_xref=\"taxon:")) {
      const uint64_t q = p + 16;
      uint64_t r = q;
      while (r < e && is_digit(text[r])) r++;
      if (r > q && r < e && text[r] == '"') return LineKind{kTaxon | kQuoteBit, (uint32_t)q, (uint32_t)r};
    } else if (lit_at(text, p, e, "/protein_id=\"")) {
      const uint64_t q = p + 13;
      if (pid.kind == kOther && q < e && text[q] != '"' && L > q) pid = LineKind{kProteinId | kQuoteBit, (uint32_t)q, (uint32_t)next_quote(text, q, e)};
    } else if (p > a && is_space(text[p - 1]) && lit_at(text, p, e, "/translation=\"")) {
      const uint64_t q = p + 14;
      if (q >= e) continue;
      if (L == q - 1) opens = LineKind{kOpens | kQuoteBit, (uint32_t)q, (uint32_t)e};
      else if (whole.kind == kOther && text[q] != '"' && L > q) whole = LineKind{kWhole | kQuoteBit, (uint32_t)q, (uint32_t)next_quote(text, q, e)};
    }
  }
  if (pid.kind != kOther) return pid;
  if (whole.kind != kOther) return whole;
  if (opens.kind != kOther) return opens;
  return LineKind{kOther | kQuoteBit, 0, 0};
}

// ---- the scans ------------------------------------------------------------------------------------------------------
// what line i with kind byte k gives to the three maximum-scans
KJF_HD void scan_values(uint32_t k, uint32_t i, uint32_t *tax, uint32_t *pid, uint64_t *ev) {
  const uint32_t kind = k & kKindMask;
  *tax = kind == kTaxon ? i + 1 : 0;
  *pid = kind == kProteinId ? i + 1 : 0;
  *ev = kind == kOpens ? 2 * ((uint64_t)i + 1) + 1 : (kind == kOther && (k & kQuoteBit)) ? 2 * ((uint64_t)i + 1) : 0;
}
struct Carry { uint32_t tax_len, pid_len, in_t, reserved; };   // the state behind the blocks so far; a length of 0: none seen
KJF_HD uint32_t inside(uint64_t ev, const Carry &c) { return ev ? (uint32_t)(ev & 1) : c.in_t; }

// ---- letters --------------------------------------------------------------------------------------------------------
#define KJG_BIT(ch) (1u << ((ch) - 'A'))
constexpr uint32_t kAaBits = KJG_BIT('A') | KJG_BIT('R') | KJG_BIT('N') | KJG_BIT('D') | KJG_BIT('C') | KJG_BIT('Q') | KJG_BIT('E') | KJG_BIT('G') | KJG_BIT('H') |
                             KJG_BIT('I') | KJG_BIT('L') | KJG_BIT('K') | KJG_BIT('M') | KJG_BIT('F') | KJG_BIT('P') | KJG_BIT('S') | KJG_BIT('T') | KJG_BIT('W') |
                             KJG_BIT('Y') | KJG_BIT('V');
constexpr uint32_t kUpperBits = kAaBits | KJG_BIT('B') | KJG_BIT('Z');       // 'B' and 'Z' become 'D' and 'E' in front of the filter
#undef KJG_BIT
KJF_HD bool is_kept(uint32_t b) {
  const uint32_t u = b - 'A', l = b - 'a';
  return (u < 26u && ((kUpperBits >> u) & 1u)) || (l < 26u && ((kAaBits >> l) & 1u));
}
KJF_HD uint32_t printed(uint32_t b) { return b == 'B' ? 'D' : b == 'Z' ? 'E' : b; }
// bit k set: byte k of chunk c is kept and lies in [a, e)
KJF_HD uint32_t keep_mask(const uint8_t *text, uint64_t c, uint64_t a, uint64_t e) {
  const kji::Chunk v = kji::load_chunk(text, c);
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < kChunk; k++) m |= (is_kept(kji::chunk_byte(v, k)) ? 1u : 0u) << k;
  return m & kji::range_mask(c * kChunk, a, e);
}
KJF_HD uint64_t count_kept(const uint8_t *text, uint64_t a, uint64_t e) {
  uint64_t n = 0;
  for (uint64_t c = a / kChunk; c * kChunk < e; c++) n += kji::popc16(keep_mask(text, c, a, e));
  return n;
}
// the position of kept byte j (from 0) of [a, e); e if there are fewer
KJF_HD uint64_t nth_kept(const uint8_t *text, uint64_t a, uint64_t e, uint64_t j) {
  for (uint64_t c = a / kChunk; c * kChunk < e; c++) {
    uint32_t m = keep_mask(text, c, a, e);
    const uint32_t n = kji::popc16(m);
    if (j >= n) { j -= n; continue; }
    for (; j; j--) m &= m - 1;
    return c * kChunk + kji::ctz16(m);
  }
  return e;
}

// ---- lengths --------------------------------------------------------------------------------------------------------
struct View {
  const uint8_t *text;
  const uint32_t *line_start;          // [n_lines + 1]
  const uint8_t *kind;                 // [n_lines]
  const uint32_t *cap_a, *cap_e;       // [n_lines] the capture of a kind 1 to 4 line
  const uint32_t *tax_src, *pid_src;   // [n_lines] line + 1 of the kind 1 / 2 line seen last, 0: the carried string
  const uint8_t *in_t;                 // [n_lines] inside a translation in front of the line
  const Carry *carry;
  const uint8_t *carry_tax, *carry_pid;
  uint32_t n_lines;
};
KJF_HD bool has_header(uint32_t k) { return (k & kKindMask) == kWhole || (k & kKindMask) == kOpens; }
KJF_HD uint64_t src_len(const View &V, uint32_t src, uint32_t carried) { return src ? V.cap_e[src - 1] - V.cap_a[src - 1] : carried; }
KJF_HD uint32_t src_byte(const View &V, uint32_t src, const uint8_t *carried, uint64_t p) { return src ? V.text[V.cap_a[src - 1] + p] : carried[p]; }
// a kind 3 / 4 line in front of which no taxon was seen
KJF_HD bool lacks_taxon(const View &V, uint32_t i) { return has_header(V.kind[i]) && V.tax_src[i] == 0 && V.carry->tax_len == 0; }
struct Out { uint64_t hdr, seq, span; };   // bytes of the header line and of the sequence line ('\n' included; 0: none), bytes filtered
KJF_HD Out line_out(const View &V, uint32_t i) {
  Out o{0, 0, 0};
  const uint32_t k = V.kind[i];
  uint64_t a, e;
  if (has_header(k)) {
    o.hdr = 1 + src_len(V, V.pid_src[i], V.carry->pid_len) + 1 + src_len(V, V.tax_src[i], V.carry->tax_len) + 1;
    a = V.cap_a[i]; e = V.cap_e[i];
  } else if ((k & kKindMask) == kOther && V.in_t[i]) {
    a = V.line_start[i]; e = (uint64_t)V.line_start[i + 1] - 1;
  } else {
    return o;
  }
  o.span = e - a;
  o.seq = count_kept(V.text, a, e) + 1;
  return o;
}

// ---- write ----------------------------------------------------------------------------------------------------------
struct Unit {
  uint64_t off, len, hdr;              // of the output: where the line's bytes start, how many, how many of them are the header line
  uint64_t pid_len, tax_len;
  uint64_t a, e, cursor;               // the span of the sequence line, the kept byte written last
  uint32_t tax_src, pid_src;
  bool fits_hdr, fits_seq;             // an output line is written iff it ends at or in front of out_cap
};
KJF_HD Unit load_unit(const View &V, const uint64_t *line_off, uint32_t i, uint64_t out_cap) {
  Unit U{};
  U.off = line_off[i]; U.len = line_off[i + 1] - U.off;
  if (!U.len) return U;
  if (has_header(V.kind[i])) {
    U.pid_src = V.pid_src[i]; U.tax_src = V.tax_src[i];
    U.pid_len = src_len(V, U.pid_src, V.carry->pid_len); U.tax_len = src_len(V, U.tax_src, V.carry->tax_len);
    U.hdr = 1 + U.pid_len + 1 + U.tax_len + 1;
    U.a = V.cap_a[i]; U.e = V.cap_e[i];
  } else {
    U.a = V.line_start[i]; U.e = (uint64_t)V.line_start[i + 1] - 1;
  }
  U.cursor = kNoPos;
  U.fits_hdr = U.off + U.hdr <= out_cap; U.fits_seq = U.off + U.len <= out_cap;
  return U;
}
// byte p of the unit (p < U.len); the bytes of a sequence line are asked for in rising order
KJF_HD uint32_t unit_byte(const View &V, Unit &U, uint64_t p) {
  if (p < U.hdr) {
    if (p == 0) return '>';
    p -= 1;
    if (p < U.pid_len) return src_byte(V, U.pid_src, V.carry_pid, p);
    if (p == U.pid_len) return '_';
    p -= U.pid_len + 1;
    if (p < U.tax_len) return src_byte(V, U.tax_src, V.carry_tax, p);
    return '\n';
  }
  uint64_t q;
  if (U.cursor == kNoPos) q = nth_kept(V.text, U.a, U.e, p - U.hdr);
  else for (q = U.cursor + 1; q < U.e && !is_kept(V.text[q]); q++) {}
  if (q >= U.e) return '\n';
  U.cursor = q;
  return printed(V.text[q]);
}
// the bytes of chunk c of the output; lo, hi: the lines the chunk's block touches
KJF_HD uint32_t gbk_chunk(uint64_t c, const View &V, const uint64_t *line_off, uint32_t lo, uint32_t hi, uint64_t total, uint64_t out_cap, Chunk *v) {
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
    const uint64_t p = pos - U.off;
    if (!(p < U.hdr ? U.fits_hdr : U.fits_seq)) continue;
    const uint64_t byte = unit_byte(V, U, p);
    if (k < 8) w0 |= byte << (8 * k); else w1 |= byte << (8 * (k - 8));
    m |= 1u << k;
  }
  v->w[0] = (uint32_t)w0; v->w[1] = (uint32_t)(w0 >> 32); v->w[2] = (uint32_t)w1; v->w[3] = (uint32_t)(w1 >> 32);
  return m;
}
// bytes of the whole output lines in front of out_cap
KJF_HD uint64_t written_bytes(const View &V, const uint64_t *line_off, uint64_t out_cap) {
  const uint64_t total = line_off[V.n_lines];
  if (total <= out_cap) return total;
  uint32_t lo = 0, hi = V.n_lines;                            // the first line that ends behind out_cap
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (line_off[mid + 1] <= out_cap) lo = mid + 1; else hi = mid; }
  const Unit U = load_unit(V, line_off, lo, out_cap);
  return U.off + (U.hdr && U.fits_hdr ? U.hdr : 0);
}

// ---- finish ---------------------------------------------------------------------------------------------------------
struct Totals {
  uint64_t kinds[5];                   // lines per kind
  uint64_t records, kept, dropped;     // headers; bytes of the filtered spans that were kept / dropped
  uint32_t no_tax_line;                // line + 1 of the first line that lacks a taxon, kNone: none
  uint32_t fin_tax, fin_pid;           // the scans over every line of the block
  uint32_t advance;                    // 1: the carried state took this block in
  uint64_t fin_ev;
};
// the info of a call, and the carried state behind it: it advances only when the whole text was written
KJF_HD kaiju_gpu_gbk_info finish(const View &V, const uint64_t *line_off, uint64_t out_cap, Totals &T, Carry &C) {
  kaiju_gpu_gbk_info o{};
  const bool bad = T.no_tax_line != kNone;
  o.n_lines = V.n_lines;
  for (uint32_t k = 0; k < 5; k++) o.lines_kind[k] = T.kinds[k];
  if (bad) {
    o.no_taxon_line = T.no_tax_line;
  } else {
    o.text_bytes = line_off[V.n_lines];
    o.written_bytes = written_bytes(V, line_off, out_cap);
    o.n_records = T.records; o.letters_kept = T.kept; o.letters_dropped = T.dropped;
    o.overflow = o.text_bytes > out_cap ? 1u : 0u;
  }
  T.advance = !bad && !o.overflow;
  if (T.advance) {
    if (T.fin_tax) C.tax_len = V.cap_e[T.fin_tax - 1] - V.cap_a[T.fin_tax - 1];
    if (T.fin_pid) C.pid_len = V.cap_e[T.fin_pid - 1] - V.cap_a[T.fin_pid - 1];
    C.in_t = inside(T.fin_ev, C);
  }
  return o;
}

}  // namespace kjg

#endif  // KJ_GBK_H
