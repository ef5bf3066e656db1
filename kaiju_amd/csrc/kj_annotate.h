// kj_annotate.h — kaiju-addTaxonNames on a text of output lines: the per-lane logic, for the device (annotate.hip) and for
// the host (tests/emu/annotate_emu.cpp drives the same functions pass by pass).  What kj_format_names.h does for records, this
// does for lines that exist already: those of an earlier run, of kaiju -v, of kaijux / kaijup, of the reference's own kaiju.
//
// The rules are those of kaiju-addTaxonNames.cpp:133-228 of the reference (getline, find('\t') twice, find_first_not_of of
// the digits, stoul), observed on the unmodified tool:
//   lines     a line ends at '\n'; the last one may lack it and gets one in the output; a line of length 0 gives nothing.
//             Every other byte, '\r' and NUL included, is a byte of the line
//   byte 0    not 'C': the line is copied unchanged, or - with drop - left out.  Only byte 0 is looked at
//   id        t2 = the second tab of the line; the id is the run of [0-9] directly behind it, whatever follows the run
//             ("7abc", "7 8", "7\r", "7\t..." of kaiju -v all read 7; "007" reads 7)
//   unchanged fewer than two tabs, an empty run ("+7", " 7"), a value above 2^64 - 1 (by value: thirty zeros and a 7 is 7), an
//             id that is no node, a node without a name of its own.  Such a 'C' line is kept under drop
//   else      line "\t" annotation "\n", the annotation that of kj_format_names.h (name, path, ranks); it may be empty (the
//             root in path mode)
//
// Passes (every one works on independent units; the units of a pass may run in any order):
//   lines   that of kj_ingest.h as it is: tiles of 4096 bytes, 16 per lane; line_start[0 .. n_lines], n_lines
//   len     one lane per line: the second tab by 16-byte chunks, the digit run, kjn::annotation_of; olen[line] (0: no line),
//           aslot[line] (kjn::kNone: copied unchanged), the counts of the info
//   offsets kjl::launch_offsets over olen[]: out_off[0 .. n_lines].  Lines may be empty, so out_off[] rises but not strictly
//           (kjn::find_last_start / the search of kjl::write_blocks take the last line that starts at a byte)
//   write   kjl::write_blocks: per lane 16 aligned bytes of the output, one aligned store, made byte by byte as in
//           kjn::format_chunk: body bytes from the text, a tab, the annotation through kjn::locate / kjn::entry_byte, a
//           newline.  Lines are written whole or not at all; nothing at or behind out_cap is touched.  (A second path that
//           copied a chunk lying wholly inside one body with two aligned 16-byte loads and a funnel shift was built and
//           measured: not faster, taken out again - DESIGN.md 3.12.)
//   finish  kaiju_gpu_annotate_info
//
// Sizes: a text is at most kji::kMaxBytes bytes, so positions and line lengths fit 32 bits (line_start[] is the 32-bit array
// of kj_ingest.h).  A line of nearly 2^32 bytes plus its annotation does not, so olen[] and out_off[] are 64 bit.
#ifndef KJ_ANNOTATE_H
#define KJ_ANNOTATE_H

#include "kj_format_names.h"
#include "kj_ingest.h"

namespace kja {

using kjf::Chunk;
using kjf::kChunk;
using kjn::Tab;
using kjn::kNone;

static_assert(kji::kChunk == kjf::kChunk && kji::kTileBytes == kjf::kBlockBytes, "the chunks of the input are those of the output");

// why a line has no annotation (kWhyNone: it has one)
enum { kWhyNone = 0, kWhyBadId = 1, kWhyUnknown = 2, kWhyUnnamed = 3, kWhyDropped = 4, kWhyEmpty = 5, kWhyOther = 6, kWhyCount = 7 };

constexpr uint64_t kMaxTenth = 1844674407370955161ull;   // (2^64 - 1) / 10; 2^64 - 1 ends in 5

// ---- len ----------------------------------------------------------------------------------------------------------
// the position of the second '\t' in text[a, e), or e: 16 aligned bytes at a time (text: the contract of kji::load_chunk)
KJF_HD uint64_t second_tab(const uint8_t *text, uint64_t a, uint64_t e) {
  uint32_t seen = 0;
  for (uint64_t c = a / kChunk; c * kChunk < e; c++) {
    uint32_t m = kji::eq_mask(kji::load_chunk(text, c), '\t') & kji::range_mask(c * kChunk, a, e);
    if (seen == 0 && m) { m &= m - 1; seen = 1; }
    if (seen && m) return c * kChunk + kji::ctz16(m);
  }
  return e;
}
// the run of [0-9] at text[p, e): false when it is empty or its value exceeds 2^64 - 1
KJF_HD bool parse_id(const uint8_t *text, uint64_t p, uint64_t e, uint64_t *id) {
  uint64_t acc = 0;
  bool any = false, over = false;
  for (; p < e; p++) {
    const uint32_t d = (uint32_t)text[p] - '0';
    if (d > 9) break;
    any = true;
    if (acc > kMaxTenth || (acc == kMaxTenth && d > 5)) over = true;
    acc = acc * 10 + d;
  }
  *id = acc;
  return any && !over;
}
// bytes the line text[a, a + len) gives in the output (0: none); *aslot: the slot whose annotation it carries (kNone: none)
KJF_HD uint64_t line_out(const uint8_t *text, uint64_t a, uint32_t len, const Tab &T, int drop, uint32_t *aslot, uint32_t *why) {
  *aslot = kNone;
  if (len == 0) { *why = kWhyEmpty; return 0; }
  if (text[a] != 'C') {
    *why = drop ? kWhyDropped : kWhyOther;
    return drop ? 0 : (uint64_t)len + 1;
  }
  const uint64_t e = a + len, t2 = second_tab(text, a, e);
  uint64_t id;
  if (t2 == e || !parse_id(text, t2 + 1, e, &id)) { *why = kWhyBadId; return (uint64_t)len + 1; }
  uint32_t alen, w;
  *aslot = kjn::annotation_of(T, id, &alen, &w);
  *why = w == kjn::kWhyUnknown ? kWhyUnknown : w == kjn::kWhyUnnamed ? kWhyUnnamed : kWhyNone;
  return *aslot == kNone ? (uint64_t)len + 1 : (uint64_t)len + 2 + alen;
}

// ---- write --------------------------------------------------------------------------------------------------------
struct Line {
  uint64_t off, olen;       // where its output starts, bytes of it (0: none)
  uint32_t src, body;       // text[src, src + body): the line without its newline
  uint32_t aslot;
  bool fits;
};
KJF_HD Line load_line(const uint32_t *line_start, const uint64_t *out_off, const uint32_t *aslot, uint32_t r, uint64_t out_cap) {
  Line L;
  const uint64_t next = out_off[r + 1];
  L.off = out_off[r];
  L.olen = next - L.off;
  L.src = line_start[r];
  L.body = kji::line_len(line_start, r);
  L.aslot = aslot[r];
  L.fits = next <= out_cap;
  return L;
}
// the bytes of chunk c of the output; r_lo, r_hi: the lines the chunk's block touches.  Returns the mask of the bytes to write: those of lines that end at or in front of out_cap
KJF_HD uint32_t annotate_chunk(uint64_t c, const uint8_t *text, const uint32_t *line_start, const uint64_t *out_off, const uint32_t *aslot, const Tab &T,
                               uint32_t r_lo, uint32_t r_hi, uint64_t total, uint64_t out_cap, Chunk *v) {
  const uint64_t o = c * kChunk;
  *v = Chunk{{0, 0, 0, 0}};
  if (o >= total) return 0;
  uint32_t r = kjn::find_last_start(out_off, r_lo, r_hi, o);
  Line L = load_line(line_start, out_off, aslot, r, out_cap);
  kjn::Entry E = kjn::make_entry(T, kNone, 0, 0);
  E.end = 0;                                               // (no piece yet)
  uint64_t lo = 0, hi = 0;
  uint32_t m = 0;
  for (uint32_t k = 0; k < kChunk; k++) {
    const uint64_t pos = o + k;
    if (pos >= total) break;
    while (pos - L.off >= L.olen) { L = load_line(line_start, out_off, aslot, ++r, out_cap); E.end = 0; }
    if (!L.fits) continue;
    const uint64_t p = pos - L.off;
    uint32_t byte;
    if (p < L.body) byte = text[(uint64_t)L.src + p];
    else if (p + 1 == L.olen) byte = '\n';
    else if (p == L.body) byte = '\t';
    else {
      const uint32_t q = (uint32_t)(p - L.body - 1);
      if (q >= E.end || q < E.start) E = kjn::locate(T, L.aslot, q);
      byte = kjn::entry_byte(T, E, q);
    }
    if (k < 8) lo |= (uint64_t)byte << (8 * k); else hi |= (uint64_t)byte << (8 * (k - 8));
    m |= 1u << k;
  }
  v->w[0] = (uint32_t)lo; v->w[1] = (uint32_t)(lo >> 32); v->w[2] = (uint32_t)hi; v->w[3] = (uint32_t)(hi >> 32);
  return m;
}

// ---- finish -------------------------------------------------------------------------------------------------------
// count[]: lines per kWhy..
KJF_HD kaiju_gpu_annotate_info make_info(uint64_t total, uint32_t n_lines, const uint32_t *count, uint64_t out_cap) {
  kaiju_gpu_annotate_info o;
  o.text_bytes = total;
  o.n_lines = n_lines;
  o.n_c_lines = count[kWhyNone] + count[kWhyBadId] + count[kWhyUnknown] + count[kWhyUnnamed];
  o.n_annotated = count[kWhyNone];
  o.n_bad_id = count[kWhyBadId];
  o.n_unknown_taxon = count[kWhyUnknown];
  o.n_unnamed_taxon = count[kWhyUnnamed];
  o.n_dropped = count[kWhyDropped];
  o.n_empty = count[kWhyEmpty];
  o.overflow = total > out_cap ? 1u : 0u;
  o.reserved = 0;
  return o;
}
// an out_cap that cannot overflow: every line gains at most a tab and an annotation, the last one a newline
KJF_HD uint64_t bound(uint64_t bytes, uint64_t n_lines, uint64_t max_annotation) { return bytes + 1 + n_lines * (1 + max_annotation); }

}  // namespace kja

// what format_names.hip offers annotate.hip: the tables of `names` as they lie on its device
#if defined(__HIPCC__)
const kjn::Tab *kj_fn_tab(const kaiju_gpu_taxon_names *names);
#endif

#endif  // KJ_ANNOTATE_H
