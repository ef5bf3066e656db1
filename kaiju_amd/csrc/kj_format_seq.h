// kj_format_seq.h — hit records to the lines of kaijux / kaijup: the per-lane and per-team logic, for the device
// (format_seq.hip) and for the host (tests/emu/format_seq_emu.cpp drives the same functions unit by unit).
//
// The rules are those of stage 4 of csrc/host/kaiju_main.cpp for kaijux / kaijup (its xmode branch), byte for byte.  For
// record r with hit h, mate lengths l1, l2 from off[] and m = min_fragment_length:
//   decision  kjf::decide, through kjf::record_line, on the compact record {lca = h.n_ids ? 1 : 0, best = h.best, info = h.n_ids}:
//             E-value table, query_len, protein input and the pair rule as in the three-column passes
//   C line    "C\t" name "\t" best "\t" ids "\t" peptides "\n"
//   ids       the first min(n_ids, 21) of h.taxid[] - sequence numbers, the index was loaded with KAIJU_GPU_IDS_SEQUENCE - in
//             ascending numeric order, ties by index, none removed; each as the name of that database sequence (the table of
//             kaiju_gpu_index_upload_seq_names) followed by ','.  A number that is no sequence contributes the ',' alone
//   peptides  nothing without -v (Job::pep == NULL); with it the text_len letters k_vb_pack packed, cut at text_cap and then
//             counted as truncated, as in kj_format_verbose.h
//   U line    "U\t" name "\t0\n" for a GATED read, "U\t" name "\n" for any other
//   gated     nucleotide rule: l1 < 3m, for pairs l1 < 3m && l2 < 3m.  kaijup rule: l1 < m, or the read has no fragment: no
//             maximal run of ASCII letters of non-zero BLOSUM62 diagonal (either case) that is at least m long and, in Greedy
//             mode, sums to at least min_score on that diagonal; the end of the read ends a run like any other byte
//   name      names_text[names[r].pos, + names[r].len), cut at the end of the text as kjf::name_of does
//
// Passes (every one works on independent units; the units of a pass may run in any order):
//   lengths   a team of kTeam lanes per record.  Lane i holds sequence number i and the length of its name; one round over the
//             values of the team (a shuffle per step on the device) gives it the bytes in front of its name inside the ids
//             column and the column's length.  Out: the length of the line, the code of the record (kCodeU / kCodeGated /
//             kCodeC), counts of 'C' lines, inexact and truncated records.  The fragment scan of the kaijup rule runs only for
//             a record the decision left unclassified with l1 >= m: the team strides the letters kTeam at a time, a segmented
//             scan over the lanes gives every letter the length and the sum of the run that ends in it, and the last lane's
//             run is the carry into the next stride (the strides of one read follow each other; the lanes of a stride are
//             independent).  Runs only grow, so a read has a fragment iff some letter's run qualifies.  A 'U' record that
//             needs no scan costs its team one step
//   offsets   64-bit exclusive prefix sum of the line lengths in blocks of kScanBlock: line_off[0 .. n]
//   middle    best, the tab and the ids column with its tab of every 'C' record whose line fits, every lane its own name and
//             comma, into the SHADOW of the output (kj_format_verbose.h)
//   write     per 16 aligned bytes of the output: the record by a search in line_off[], then byte by byte from the name, the
//             shadow, the peptides or constants.  A line is written iff it ends at or in front of out_cap; whole chunks leave
//             as one 16-byte store, no byte at or behind out_cap is touched
//   finish    kaiju_gpu_format_verbose_info (the struct of the -v passes: the same fields mean the same here)
#ifndef KJ_FORMAT_SEQ_H
#define KJ_FORMAT_SEQ_H

#include "kj_format_verbose.h"

namespace kjq {

using kjf::Chunk;
using kjf::kBlockBytes;
using kjf::kBlockLanes;
using kjf::kChunk;
using kjf::kScanBlock;
using kjv::Hdr;
using kjv::kMaxIds;
using kjv::kMaxPrefix;
using kjv::kTeam;

constexpr uint32_t kMaxSeqName = kMaxPrefix;             // longest name the table may hold: 21 of them, their commas and the
                                                         // rest of a middle fit 32 bits
static_assert(((uint64_t)kMaxSeqName + 1) * kMaxIds + 64 < (1ull << 32), "the ids column in 32 bits");
constexpr uint64_t kCodeU = 0, kCodeGated = 1, kCodeC = 2;

// BLOSUM62 diagonal of A .. Z, four bits each, 0: no amino acid (B J O U X Z)
constexpr uint64_t diag_pack(uint32_t from, uint32_t to) {
  constexpr uint8_t d[26] = {4, 0, 9, 6, 5, 6, 6, 8, 4, 0, 5, 4, 5, 6, 0, 7, 5, 5, 4, 5, 0, 4, 11, 0, 7, 0};   // the table of kaiju_main.cpp
  uint64_t v = 0;
  for (uint32_t k = from; k < to; k++) v |= (uint64_t)d[k] << (4 * (k - from));
  return v;
}
constexpr uint64_t kDiagLo = diag_pack(0, 16), kDiagHi = diag_pack(16, 26);
static_assert(kDiagLo == 0x7065450486656904ull && kDiagHi == 0x070b405455ull, "A .. P, Q .. Z");
KJF_HD uint32_t diag_of(uint32_t byte) {
  const uint32_t c = byte & ~32u;
  if (c < 'A' || c > 'Z') return 0;
  const uint32_t k = c - 'A';
  return (uint32_t)((k < 16 ? kDiagLo >> (4 * k) : kDiagHi >> (4 * (k - 16))) & 15u);
}

// what the passes read and write; device pointers on the device, host pointers in the emulation
struct Job {
  kjf::Params P;
  const double *pw;
  const kaiju_gpu_hit *hits;
  const uint64_t *off;
  const uint8_t *seqs;                 // the reads off[] points into: the kaijup rule only
  const uint64_t *text_pos;            // n: where the peptides of a record lie in pep          } looked at only
  const uint32_t *text_len;            // n                                                     } with pep != NULL
  const uint32_t *trunc;               // n or NULL: records whose peptides were cut before they got here
  const uint8_t *pep;                  // NULL: no peptide column (without -v)
  uint32_t text_cap;
  uint32_t u_rule;                     // KAIJU_GPU_U_RULE_*
  uint32_t min_frag, min_score, greedy;
  const uint8_t *names_text;
  uint64_t names_bytes;
  const kaiju_gpu_name_span *names;
  const uint8_t *sn_blob;              // the sequence-name table of the index
  const uint64_t *sn_off;
  const uint32_t *sn_len;
  uint32_t nseq;
  uint8_t *out;
  uint64_t out_cap;
  kaiju_gpu_format_verbose_info *info;
  uint64_t *llen, *line_off, *code;    // n + 1 each
  uint8_t *shadow;                     // out_cap bytes
  uint64_t *oblk, *oblk_base;
  Hdr *hdr;
};

// ---- lengths ----------------------------------------------------------------------------------------
struct Head {                          // what every lane of a team knows of its record
  uint32_t classified;
  uint32_t best, n_ids, pep_len, truncated, inexact;
  uint64_t l1, l2;
  kaiju_gpu_name_span name;
};
KJF_HD Head record_head(const Job &J, uint32_t r) {
  Head h{};
  const uint64_t a = J.off[2 * (uint64_t)r], b = J.off[2 * (uint64_t)r + 1], c = J.off[2 * (uint64_t)r + 2];
  h.l1 = b - a; h.l2 = c - b;
  h.name = kjf::name_of(J.names, r, J.names_bytes);
  const uint32_t ni = J.hits[r].n_ids;
  h.inexact = (J.hits[r].flags & KAIJU_HIT_INEXACT) ? 1u : 0u;
  // (the decision through the very function the three-column passes take it from, on the record stage 4 makes of the hit.
  //  Its lca, n_ids ? 1 : 0, is written as the constant 1: info = n_ids = 0 makes the record unclassified by itself, and only
  //  whether the answer is 0 is looked at, so nothing depends on a value that comes back through the gate)
  const kaiju_gpu_compact rec{1ull, J.hits[r].best, ni};
  const uint64_t off3[3] = {0, h.l1, h.l1 + h.l2};
  uint64_t t;
  (void)kjf::record_line(&rec, off3, &h.name, 0, J.names_bytes, J.P, J.pw, &t);
  h.classified = t ? 1u : 0u;
  if (!t) return h;
  h.best = rec.best;
  h.n_ids = ni < kMaxIds ? ni : kMaxIds;
  if (J.pep) {
    const uint32_t tl = J.text_len[r];
    h.pep_len = tl < J.text_cap ? tl : J.text_cap;
    h.truncated = (tl > J.text_cap || (J.trunc && J.trunc[r])) ? 1u : 0u;
  }
  return h;
}
struct Lane {                          // what lane i of a team holds
  uint64_t id;
  uint32_t piece;                      // bytes of name i and its comma, 0: there is no id i
  uint32_t iseq, name_len;             // name_len 0: nothing but the comma
};
KJF_HD Lane load_lane(const Job &J, uint32_t r, uint32_t i, const Head &h) {
  Lane L{0, 0, 0, 0};
  if (i < h.n_ids) {
    L.id = J.hits[r].taxid[i];
    const uint32_t q = (uint32_t)L.id;                   // (kaiju_gpu_index_seq_name takes 32 bits of it)
    if (q < J.nseq) { L.iseq = q; L.name_len = J.sn_len[q]; }
    L.piece = L.name_len + 1;
  }
  return L;
}
// X: how a lane sees lane k of its team (the device hands `mine` to a shuffle, the emulation reads lane k's row).
// The bytes of the ids column in front of this lane's name, and the column's length
template <class X>
KJF_HD void round_ids(const X &x, const Lane &me, uint32_t i, uint32_t *id_off, uint32_t *ids_len) {
  uint32_t o = 0, t = 0;
#pragma unroll
  for (uint32_t k = 0; k < kMaxIds; k++) {
    const uint64_t v = x.id(me.id, k);
    const uint32_t l = x.piece(me.piece, k);
    t += l;
    if (v < me.id || (v == me.id && k < i)) o += l;
  }
  *id_off = o; *ids_len = t;
}
// best, its tab, the ids column and its tab
KJF_HD uint64_t mid_len(const Head &h, uint32_t ids_len) { return (uint64_t)kjf::digits_u64(h.best) + 1 + ids_len + 1; }
KJF_HD uint64_t line_len_u(const Head &h, bool gated) { return (uint64_t)h.name.len + (gated ? 5 : 3); }
KJF_HD uint64_t line_len_c(const Head &h, uint32_t ids_len) { return 2 + (uint64_t)h.name.len + 1 + mid_len(h, ids_len) + h.pep_len + 1; }

// the 'U' line of an unclassified record.  *scan: the answer needs the fragment scan (gated = it finds no fragment)
KJF_HD bool u_gated(const Job &J, const Head &h, bool *scan) {
  *scan = false;
  if (J.u_rule != KAIJU_GPU_U_RULE_PROTEIN) {
    const uint64_t m3 = 3ull * J.min_frag;
    return J.P.paired ? (h.l1 < m3 && h.l2 < m3) : h.l1 < m3;
  }
  if (h.l1 < J.min_frag) return true;
  if (J.min_frag == 0 && (!J.greedy || J.min_score == 0)) return false;   // (the empty run at the end of the read qualifies)
  *scan = true;
  return false;
}
// the fragment scan: the run that ends in a letter, as far as a lane knows it
struct Seg { uint32_t len, sum, brk; };      // brk: a byte that ends runs lies at or in front of this lane, in this stride
KJF_HD uint32_t frag_letter(const Job &J, uint32_t r, uint64_t p, uint64_t l1) { return p < l1 ? diag_of(J.seqs[J.off[2 * (uint64_t)r] + p]) : 0; }
KJF_HD Seg frag_init(uint32_t d) { return Seg{d ? 1u : 0u, d, d ? 0u : 1u}; }
// step `delta` (1, 2, 4, 8, 16) of the segmented scan; up: the Seg of lane i - delta (of lane i itself where i < delta)
KJF_HD Seg frag_round(const Seg &me, const Seg &up, uint32_t i, uint32_t delta) {
  Seg s = me;
  if (i >= delta && !me.brk) { s.len += up.len; s.sum += up.sum; s.brk = up.brk; }
  return s;
}
// behind the last step: the run that reaches back to the start of the stride goes on from the carry
KJF_HD Seg frag_close(const Seg &me, const Seg &carry) {
  Seg s = me;
  if (!me.brk) { s.len += carry.len; s.sum += carry.sum; }
  return s;
}
KJF_HD bool frag_hit(const Job &J, uint32_t d, const Seg &s) { return d != 0 && s.len >= J.min_frag && (!J.greedy || s.sum >= J.min_score); }
KJF_HD uint64_t frag_steps(uint64_t l1) { return (l1 + kTeam - 1) / kTeam; }

// ---- middle -----------------------------------------------------------------------------------------
// the piece of lane i; mid: where `best` of the record starts in the shadow
KJF_HD void mid_lane(const Job &J, const Head &h, const Lane &me, uint32_t i, uint32_t id_off, uint32_t ids_len, uint8_t *mid) {
  const uint32_t db = kjf::digits_u64(h.best);
  const uint32_t ids0 = db + 1;
  if (i == 0) {
    kjv::put_number(mid, h.best, db); mid[db] = '\t';
    mid[ids0 + ids_len] = '\t';
  }
  if (me.piece) {
    uint8_t *d = mid + ids0 + id_off;
    const uint8_t *s = J.sn_blob + (me.name_len ? J.sn_off[me.iseq] : 0);
    for (uint32_t p = 0; p < me.name_len; p++) d[p] = s[p];
    d[me.name_len] = ',';
  }
}

// ---- write ------------------------------------------------------------------------------------------
struct SLine {
  uint64_t off, len;
  uint64_t tab;                        // 2 + name_len: where the byte behind the name lies
  uint64_t pep0;                       // where the peptides start in the line ('C' lines)
  uint64_t pep_at;                     // ... and in Job::pep
  uint32_t name_pos;
  bool c, fits;
};
KJF_HD SLine load_sline(const Job &J, uint32_t r) {
  SLine L;
  const uint64_t next = J.line_off[r + 1];
  const kaiju_gpu_name_span s = kjf::name_of(J.names, r, J.names_bytes);
  L.off = J.line_off[r];
  L.len = next - L.off;
  L.tab = 2 + (uint64_t)s.len;
  L.name_pos = s.pos;
  L.c = J.code[r] == kCodeC;
  L.fits = next <= J.out_cap;
  L.pep0 = L.len - 1; L.pep_at = 0;
  if (L.c && J.pep) {
    const uint32_t tl = J.text_len[r];
    L.pep0 = L.len - 1 - (tl < J.text_cap ? tl : J.text_cap);
    L.pep_at = J.text_pos[r];
  }
  return L;
}
// byte p of the line (p < L.len)
KJF_HD uint32_t sline_byte(const Job &J, const SLine &L, uint64_t p) {
  if (p == 0) return L.c ? 'C' : 'U';
  if (p == 1) return '\t';
  if (p < L.tab) return J.names_text[(uint64_t)L.name_pos + (p - 2)];
  if (p == L.len - 1) return '\n';
  if (p == L.tab) return '\t';
  if (!L.c) return '0';
  if (p < L.pep0) return J.shadow[L.off + p];
  return J.pep[L.pep_at + (p - L.pep0)];
}
// the bytes of chunk c of the output; r_lo, r_hi: kjf::block_records of the chunk's block.  Returns the mask of the bytes to
// write: those of lines that end at or in front of out_cap
KJF_HD uint32_t format_schunk(const Job &J, uint64_t c, uint32_t r_lo, uint32_t r_hi, uint64_t total, Chunk *v) {
  const uint64_t o = c * kChunk;
  *v = Chunk{{0, 0, 0, 0}};
  if (o >= total) return 0;
  uint32_t r = kjf::find_record(J.line_off, r_lo, r_hi, o);
  SLine L = load_sline(J, r);
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < kChunk; k++) {
    const uint64_t pos = o + k;
    if (pos >= total) break;
    if (pos - L.off >= L.len) L = load_sline(J, ++r);
    if (L.fits) {
      v->w[k >> 2] |= sline_byte(J, L, pos - L.off) << (8 * (k & 3));
      m |= 1u << k;
    }
  }
  return m;
}

// ---- finish: kjv::make_info and kjv::written_bytes ----------------------------------------------------

}  // namespace kjq

// what format_seq.hip offers capi_text.hip
#if defined(__HIPCC__)
// J: the inputs of kjq::Job (everything up to nseq) set; the arrays of the passes are filled in here.  Queues init, lengths and
// offsets on `stream`; grows st.mem, and leaves in st.total the device address of the size of the whole text.  Returns 0, or a
// kaiju_gpu_status with *err set.
int kj_fs_lengths(kjl::Lines &st, hipStream_t stream, kjq::Job &J, uint32_t n, const char **err);
// queues middle, write and finish behind the kj_fs_lengths of the same J and n; the shadow (out_cap bytes) grows on demand.
// st.written: the device address of the number of bytes written (= text_bytes unless it overflows)
int kj_fs_write(kjl::Lines &st, hipStream_t stream, kjq::Job &J, uint32_t n, void *d_out, uint64_t out_cap, kaiju_gpu_format_verbose_info *d_info,
                const char **err);
#endif

#endif  // KJ_FORMAT_SEQ_H
