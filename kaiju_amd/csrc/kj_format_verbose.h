// kj_format_verbose.h — hit records and matches to the seven-column lines of kaiju -v: the per-lane and per-team logic, for the
// device (format_verbose.hip) and for the host (tests/emu/format_verbose_emu.cpp drives the same functions unit by unit).
//
// The rules are those of stage 4 of csrc/host/kaiju_main.cpp for kaiju / kaiju-multi with -v, byte for byte.  For record r:
//   decision  kjf::decide (kj_format.h) on the compact record k_lca makes of the hit: E-value table, query_len, protein input
//             and the pair rule as there.  Taxon 0: "U\t" name "\t0\n", the line without -v
//   line      "C\t" name "\t" taxon "\t" best "\t" ids "\t" accs "\t" peptides "\n"
//   ids       the first n_ids (at most 21) of taxid[] of the hit in ascending numeric order, each in decimal and followed
//             by ',' (the iteration order of the reference's std::set<uint64_t>, ConsumerThread.cpp:527-536)
//   accs      of each of the first min(n_acc, 20) sequence numbers acc_iseq[q] the name of that database sequence up to, not
//             including, its last '_' (a name without '_' and a number that is no sequence contribute nothing, a name that
//             starts with its only '_' the empty string); the set of these strings in std::string order (bytes compared as
//             unsigned, a proper prefix first), each distinct string once and followed by ',' (ConsumerThread.cpp:822-824, 532).
//             The device never compares strings: acc_rank[iseq] (kaiju_accession_ranks, host) is the position of the prefix
//             among the sorted distinct prefixes of the whole index, equal strings share a rank, kNoRank = no '_'
//   peptides  the text_len letters of column 7 as k_vb_pack packs them (the commas are in them); text_len above text_cap is
//             cut at text_cap and the record counted as truncated (classified records only, as stage 4 warns)
//   name      names_text[names[r].pos, + names[r].len), cut at the end of the text as kjf::name_of does
//   numbers   kjf::digits_u64 and to_bcd: no division by a variable
//
// Passes (every one works on independent units; the units of a pass may run in any order):
//   lengths   a team of kTeam lanes per record.  Lane i holds id i and accession rank i; every lane walks the values of the
//             team (a shuffle per step on the device) and so knows the bytes in front of its piece inside its column - the
//             lengths of the ids that sort in front of its own, ties broken by index; the lengths of the KEPT prefixes (no
//             equal rank at a lower index) of smaller rank - and the length of the column.  Out: the taxon, the length of
//             the line, counts of 'C' lines, inexact and truncated records.  A 'U' record costs its team one step
//   offsets   64-bit exclusive prefix sum of the line lengths in blocks of kScanBlock: line_off[0 .. n]
//   middle    columns 3 to 6 of every 'C' record whose line fits, rendered once by its team, every lane its own piece, into
//             the SHADOW: a scratch text in which a byte lies where it lies in the output.  The write pass copies the middle
//             of a line from the same offset it writes to (source and destination aligned alike), no second table of offsets
//             and no second prefix sum exist
//   write     per 16 aligned bytes of the output (kj_format.h): the record by a search in line_off[], then byte by byte through
//             "C\t" name "\t" | the shadow | the peptides | "\n" (or "U\t" name "\t0\n").  A line is written iff it ends at or
//             in front of out_cap; whole chunks leave as one 16-byte store, no byte at or behind out_cap is touched
//   finish    kaiju_gpu_format_verbose_info
#ifndef KJ_FORMAT_VERBOSE_H
#define KJ_FORMAT_VERBOSE_H

#include "kj_format.h"

namespace kjv {

using kjf::Chunk;
using kjf::kBlockBytes;
using kjf::kBlockLanes;
using kjf::kChunk;
using kjf::kScanBlock;

constexpr uint32_t kTeam = 32;                           // lanes per record: two records per wavefront
constexpr uint32_t kMaxIds = KAIJU_GPU_MAX_IDS;          // 21
constexpr uint32_t kMaxAcc = KAIJU_GPU_MAX_ACC;          // 20
constexpr uint32_t kNoRank = 0xffffffffu;
constexpr uint32_t kMaxPrefix = 1u << 24;                // longest prefix an accession table may hold (20 of them fit 32 bits)
static_assert(kMaxIds <= kTeam && kMaxAcc <= kTeam, "a lane per id and per accession");

struct Hdr { uint64_t written; uint32_t n, n_classified, n_inexact, n_truncated; };

// what the passes read and write; device pointers on the device, host pointers in the emulation
struct Job {
  kjf::Params P;
  const double *pw;
  const kaiju_gpu_hit *hits;
  const kaiju_gpu_compact *recs;
  const uint64_t *off;
  const uint32_t *n_acc, *acc_iseq;    // n, n x kMaxAcc
  const uint64_t *text_pos;            // n: where the peptides of a record lie in pep
  const uint32_t *text_len;            // n
  const uint32_t *trunc;               // n or NULL: records whose peptides were cut before they got here
  const uint8_t *pep;
  uint32_t text_cap;
  const uint8_t *names_text;
  uint64_t names_bytes;
  const kaiju_gpu_name_span *names;
  const uint8_t *acc_blob;             // the accession table of the index
  const uint64_t *acc_off;
  const uint32_t *acc_len, *acc_rank;
  uint32_t nseq;
  uint8_t *out;
  uint64_t out_cap;
  kaiju_gpu_format_verbose_info *info;
  uint64_t *llen, *line_off, *tax;     // n + 1 each
  uint8_t *shadow;                     // out_cap bytes
  uint64_t *oblk, *oblk_base;
  Hdr *hdr;
};

// ---- lengths ----------------------------------------------------------------------------------------
struct Head {                          // what every lane of a team knows of its record
  uint64_t taxon;                      // 0: a 'U' line; nothing else is looked at then
  uint32_t best, n_ids, n_acc, pep_len, truncated;
  kaiju_gpu_name_span name;
};
KJF_HD Head record_head(const Job &J, uint32_t r) {
  Head h{};
  // (the decision through the very function the three-column passes take it from)
  uint64_t t;
  (void)kjf::record_line(J.recs, J.off, J.names, r, J.names_bytes, J.P, J.pw, &t);
  h.taxon = t;
  h.name = kjf::name_of(J.names, r, J.names_bytes);
  if (!t) return h;
  h.best = J.recs[r].best;
  const uint32_t ni = J.hits[r].n_ids, na = J.n_acc[r], tl = J.text_len[r];
  h.n_ids = ni < kMaxIds ? ni : kMaxIds;
  h.n_acc = na < kMaxAcc ? na : kMaxAcc;
  h.pep_len = tl < J.text_cap ? tl : J.text_cap;
  h.truncated = (tl > J.text_cap || (J.trunc && J.trunc[r])) ? 1u : 0u;
  return h;
}
struct Lane {                          // what lane i of a team holds
  uint64_t id;
  uint32_t id_len;                     // digits + 1 of id i, 0: there is no id i
  uint32_t rank, acc_len, iseq;        // of accession i: its rank (kNoRank: nothing to print), prefix length + 1, sequence
};
KJF_HD Lane load_lane(const Job &J, uint32_t r, uint32_t i, const Head &h) {
  Lane L{0, 0, kNoRank, 0, 0};
  if (i < h.n_ids) { L.id = J.hits[r].taxid[i]; L.id_len = kjf::digits_u64(L.id) + 1; }
  if (i < h.n_acc) {
    const uint32_t q = J.acc_iseq[(uint64_t)r * kMaxAcc + i];
    if (q < J.nseq) {
      L.iseq = q;
      L.rank = J.acc_rank[q];
      L.acc_len = L.rank == kNoRank ? 0 : J.acc_len[q] + 1;
    }
  }
  return L;
}
// X: how a lane sees lane k of its team.  x.id(mine, k) is lane k's Lane::id and so on; the device hands `mine` to a shuffle,
// the emulation reads lane k's value from the team's row.
// First round: the bytes of column 5 in front of this lane's id, the column's length, and what this lane's prefix adds to
// column 6 (*klen, 0: not kept)
template <class X>
KJF_HD void round_ids(const X &x, const Lane &me, uint32_t i, uint32_t *id_off, uint32_t *ids_len, uint32_t *klen) {
  uint32_t o = 0, t = 0;
#pragma unroll
  for (uint32_t k = 0; k < kMaxIds; k++) {
    const uint64_t v = x.id(me.id, k);
    const uint32_t l = x.id_len(me.id_len, k);
    t += l;
    if (v < me.id || (v == me.id && k < i)) o += l;
  }
  bool dup = false;
#pragma unroll
  for (uint32_t k = 0; k < kMaxAcc; k++) {
    const uint32_t rk = x.rank(me.rank, k);
    if (k < i && rk == me.rank) dup = true;
  }
  *id_off = o; *ids_len = t;
  *klen = (me.rank != kNoRank && !dup) ? me.acc_len : 0;
}
// Second round: the bytes of column 6 in front of this lane's prefix, the column's length
template <class X>
KJF_HD void round_accs(const X &x, const Lane &me, uint32_t klen, uint32_t *acc_off, uint32_t *accs_len) {
  uint32_t o = 0, t = 0;
#pragma unroll
  for (uint32_t k = 0; k < kMaxAcc; k++) {
    const uint32_t l = x.klen(klen, k);
    const uint32_t rk = x.rank(me.rank, k);
    t += l;
    if (rk < me.rank) o += l;
  }
  *acc_off = o; *accs_len = t;
}
// columns 3 to 6 with the tab behind each
KJF_HD uint64_t mid_len(const Head &h, uint32_t ids_len, uint32_t accs_len) {
  return (uint64_t)kjf::digits_u64(h.taxon) + 1 + kjf::digits_u64(h.best) + 1 + ids_len + 1 + accs_len + 1;
}
KJF_HD uint64_t line_len_u(const Head &h) { return (uint64_t)h.name.len + 5; }
KJF_HD uint64_t line_len_c(const Head &h, uint32_t ids_len, uint32_t accs_len) {
  return 2 + (uint64_t)h.name.len + 1 + mid_len(h, ids_len, accs_len) + h.pep_len + 1;
}

// ---- middle -----------------------------------------------------------------------------------------
KJF_HD void put_number(uint8_t *dst, uint64_t v, uint32_t digits) {
  const kjf::Bcd b = kjf::to_bcd(v);
  for (uint32_t p = 0; p < digits; p++) dst[p] = (uint8_t)('0' + kjf::bcd_digit(b, digits - 1 - p));
}
// the piece of lane i; mid: where column 3 of the record starts in the shadow
KJF_HD void mid_lane(const Job &J, const Head &h, const Lane &me, uint32_t i, uint32_t id_off, uint32_t ids_len, uint32_t klen,
                     uint32_t acc_off, uint32_t accs_len, uint8_t *mid) {
  const uint32_t dt = kjf::digits_u64(h.taxon), db = kjf::digits_u64(h.best);
  const uint32_t ids0 = dt + 1 + db + 1, accs0 = ids0 + ids_len + 1;
  if (i == 0) {
    put_number(mid, h.taxon, dt); mid[dt] = '\t';
    put_number(mid + dt + 1, h.best, db); mid[dt + 1 + db] = '\t';
    mid[ids0 + ids_len] = '\t';
    mid[accs0 + accs_len] = '\t';
  }
  if (me.id_len) {
    uint8_t *d = mid + ids0 + id_off;
    put_number(d, me.id, me.id_len - 1);
    d[me.id_len - 1] = ',';
  }
  if (klen) {
    uint8_t *d = mid + accs0 + acc_off;
    const uint8_t *s = J.acc_blob + J.acc_off[me.iseq];
    for (uint32_t p = 0; p + 1 < klen; p++) d[p] = s[p];
    d[klen - 1] = ',';
  }
}

// ---- write ------------------------------------------------------------------------------------------
struct VLine {
  uint64_t off, len;
  uint64_t tab;                        // 2 + name_len: where the tab behind the name lies
  uint64_t pep0;                       // where the peptides start in the line ('C' lines)
  uint64_t pep_at;                     // ... and in Job::pep
  uint32_t name_pos;
  bool c, fits;
};
KJF_HD VLine load_vline(const Job &J, uint32_t r) {
  VLine L;
  const uint64_t next = J.line_off[r + 1];
  const kaiju_gpu_name_span s = kjf::name_of(J.names, r, J.names_bytes);
  L.off = J.line_off[r];
  L.len = next - L.off;
  L.tab = 2 + (uint64_t)s.len;
  L.name_pos = s.pos;
  L.c = J.tax[r] != 0;
  L.fits = next <= J.out_cap;
  L.pep0 = 0; L.pep_at = 0;
  if (L.c) {
    const uint32_t tl = J.text_len[r];
    L.pep0 = L.len - 1 - (tl < J.text_cap ? tl : J.text_cap);
    L.pep_at = J.text_pos[r];
  }
  return L;
}
// byte p of the line (p < L.len)
KJF_HD uint32_t vline_byte(const Job &J, const VLine &L, uint64_t p) {
  if (p == 0) return L.c ? 'C' : 'U';
  if (p == 1) return '\t';
  if (p < L.tab) return J.names_text[(uint64_t)L.name_pos + (p - 2)];
  if (p == L.tab) return '\t';
  if (p == L.len - 1) return '\n';
  if (!L.c) return '0';
  if (p < L.pep0) return J.shadow[L.off + p];
  return J.pep[L.pep_at + (p - L.pep0)];
}
// the bytes of chunk c of the output; r_lo, r_hi: kjf::block_records of the chunk's block.  Returns the mask of the bytes to
// write: those of lines that end at or in front of out_cap
KJF_HD uint32_t format_vchunk(const Job &J, uint64_t c, uint32_t r_lo, uint32_t r_hi, uint64_t total, Chunk *v) {
  const uint64_t o = c * kChunk;
  *v = Chunk{{0, 0, 0, 0}};
  if (o >= total) return 0;
  uint32_t r = kjf::find_record(J.line_off, r_lo, r_hi, o);
  VLine L = load_vline(J, r);
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < kChunk; k++) {
    const uint64_t pos = o + k;
    if (pos >= total) break;
    if (pos - L.off >= L.len) L = load_vline(J, ++r);
    if (L.fits) {
      v->w[k >> 2] |= vline_byte(J, L, pos - L.off) << (8 * (k & 3));
      m |= 1u << k;
    }
  }
  return m;
}

// ---- finish -----------------------------------------------------------------------------------------
KJF_HD kaiju_gpu_format_verbose_info make_info(uint64_t total, const Hdr &h, uint64_t out_cap) {
  kaiju_gpu_format_verbose_info o;
  o.text_bytes = total;
  o.n_records = h.n;
  o.n_classified = h.n_classified;
  o.overflow = total > out_cap ? 1u : 0u;
  o.n_inexact = h.n_inexact;
  o.n_truncated = h.n_truncated;
  o.reserved = 0;
  return o;
}
// bytes of the whole lines that fit: line_off[k] of the largest k with line_off[k] <= out_cap
KJF_HD uint64_t written_bytes(const uint64_t *line_off, uint32_t n, uint64_t out_cap) {
  const uint64_t total = line_off[n];
  return total <= out_cap ? total : line_off[kjf::find_record(line_off, 0, n + 1, out_cap)];
}

}  // namespace kjv

// what format_verbose.hip offers capi_text.hip
#if defined(__HIPCC__)
// J: the inputs of kjv::Job (everything up to nseq) set; the arrays of the passes are filled in here.  Queues init, lengths and
// offsets on `stream`; grows st.mem, and leaves in st.total the device address of the size of the whole text.  Returns 0, or a
// kaiju_gpu_status with *err set.
int kj_fv_lengths(kjl::Lines &st, hipStream_t stream, kjv::Job &J, uint32_t n, const char **err);
// queues middle, write and finish behind the kj_fv_lengths of the same J and n; the shadow (out_cap bytes) grows on demand.
// st.written: the device address of the number of bytes written (= text_bytes unless it overflows)
int kj_fv_write(kjl::Lines &st, hipStream_t stream, kjv::Job &J, uint32_t n, void *d_out, uint64_t out_cap, kaiju_gpu_format_verbose_info *d_info,
                const char **err);
#endif

#endif  // KJ_FORMAT_VERBOSE_H
