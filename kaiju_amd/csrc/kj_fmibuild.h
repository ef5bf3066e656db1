// kj_fmibuild.h - the stages of the index builder behind the suffix sort: BWT of the file, sequence ranks, replication to
// `copies` rows, suffix-array samples, index1 / index2 checkpoints and the byte coding - the per-lane logic, for the device
// (fmibuild.hip) and for the host (tests/emu/fmibuild_emu.cpp drives the same functions through loops shaped like the grids).
//
// What is on the device when the sort (kj_sufsort.h) ends: the text T[0, tlen), SA[0, nsuf) and rank[0, tlen), the inverse of
// the whole row order - rank[p] of a letter is its row (nseq + k with SA[k] = p), rank[p] of a terminator its sequence number.
// Rows 0 .. nseq-1 of the file's own index are the terminator suffixes in file order, row nseq + k is suffix SA[k].
//
// Passes (definitions; the header comment of mkfmi.cpp has the file format):
//   BWT of the file   B[rank[p]] = p ? T[p-1] : 0 for every p: gathered by row for the letters (B[nseq + k] = T[SA[k] - 1]),
//                     scattered for the nseq terminators, whose pass also writes the sequence starts start[rank[p] + 1] = p + 1
//   sequence ranks    rows k with B[nseq + k] == 0 are whole sequences in sorted order; the ord-th of them (inclusive scan of the
//                     flags) starts at p = SA[k], which is sequence i = p ? rank[p-1] + 1 : 0 of the file:
//                     read_of_rank[r0 + ord] = i, rank_of[i] = r0 + ord (r0 empty sequences sort first; the host numbers them)
//   replication       bwt[j] = B[j / copies]
//   samples           q < min(nsamp, ncheck): row k = first + (q << e), r = k / copies, t = k % copies, p = SA[r - nseq],
//                     i = the sequence of p (bounded binary search over the starts),
//                     val = ((rank_of[i] * copies + t) << pbits) + (p - start[i]), big-endian in nbytes
//   checkpoints       per piece of 65 536 rows: 256 lanes count the 21 letters of their 256-row block; the exclusive scan over
//                     the lanes is the piece's index2 rows, the total the raw index1 count (running sums, C[], tails: host)
//   byte coding       per 256-row block, in place: a row j < 128 gets startLcode[c] + min(equal letters before it, top), a row
//                     j >= 128 the equal letters after it, whatever the length of a short last block (the host loop's rule)
//
// Scratch: fb_scratch_bytes.  The driver frees the sort's second key buffer, second value buffer, active list and tile counts
// (16 bytes per suffix) when the sort ends and keeps text, rank[], SA and the first key buffer (the flags and their scan live
// there); what it allocates then is B (tlen), bwt (tlen * copies, only when copies > 1), the samples, index2, the piece counts
// and three arrays of nseq entries.
#ifndef KJ_FMIBUILD_H
#define KJ_FMIBUILD_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KJ_FB_HD __host__ __device__ inline
#else
#define KJ_FB_HD inline
#endif

enum {
  KJ_FB_BLOCK = 256,            // rows per index2 checkpoint and per coding block
  KJ_FB_PIECE = 65536,          // rows per index1 checkpoint
  KJ_FB_ALEN = 21,              // letters, the terminator included
  KJ_FB_SYM_BITS = 5,
  KJ_FB_THREADS = 256,          // lanes per workgroup of every kernel
  KJ_FB_REP_BYTES = 8,          // output bytes per lane of the replication pass
  KJ_FB_PAD = 256,              // the byte arrays are allocated to a multiple of this (whole-word loads of a last block)
  KJ_FB_SEARCH_STEPS = 32,      // bound of the binary search over the sequence starts
  KJ_FB_STAGE_BWT = 1, KJ_FB_STAGE_RANKS = 2, KJ_FB_STAGE_SAMPLES = 4, KJ_FB_STAGE_CHECKPOINTS = 8, KJ_FB_STAGE_RECODE = 16,
  KJ_FB_STAGES_ALL = 31
};

KJ_FB_HD int fb_bits_needed(uint64_t k) { int i = 0; while (i < 64 && (k >> i)) ++i; return i; }   // suffixArray.c:57
KJ_FB_HD uint64_t fb_round_up(uint64_t n, uint64_t to) { return (n + to - 1) / to * to; }

// the numbers every stage shares, on the host and on the device (init_suffixArray suffixArray.c:140-180, fmicommon.h:77-94)
struct FbPlan {
  uint64_t tlen, nseq, nsuf, copies, otlen, onseq;   // the file's own index, and what the output describes
  uint64_t first, nsamp, nfill;                      // first sampled row, samples that exist, samples that are written
  uint64_t nblk, npieces;                            // 256-row blocks, 65 536-row pieces of the output
  int64_t ncheck;                                    // the header's number of samples
  int32_t chpt_exp, sbits, pbits, nbytes, N1, N2;
};
KJ_FB_HD FbPlan fb_make_plan(uint64_t tlen, uint64_t nseq, uint64_t maxlen, uint64_t copies, int chpt_exp) {
  FbPlan P;
  P.tlen = tlen; P.nseq = nseq; P.nsuf = tlen - nseq; P.copies = copies < 1 ? 1 : copies;
  P.otlen = tlen * P.copies; P.onseq = nseq * P.copies;
  P.chpt_exp = chpt_exp;
  P.sbits = fb_bits_needed(P.onseq); P.pbits = fb_bits_needed(maxlen);
  P.nbytes = (7 + P.sbits + P.pbits) / 8;
  P.ncheck = (int64_t)(P.otlen >> chpt_exp) - (int64_t)(P.onseq >> chpt_exp);
  const uint64_t step = 1ull << chpt_exp;
  P.first = ((P.onseq + step - 1) >> chpt_exp) << chpt_exp;
  P.nsamp = P.first < P.otlen ? ((P.otlen - 1 - P.first) >> chpt_exp) + 1 : 0;
  const uint64_t nc = P.ncheck > 0 ? (uint64_t)P.ncheck : 0;
  P.nfill = P.nsamp < nc ? P.nsamp : nc;             // mkfmi only carries ncheck entries over
  P.nblk = (P.otlen + KJ_FB_BLOCK - 1) / KJ_FB_BLOCK;
  P.npieces = (P.otlen + KJ_FB_PIECE - 1) / KJ_FB_PIECE;
  const int64_t bwtlen = (int64_t)P.otlen;
  P.N1 = (int32_t)(((bwtlen - 1) >> 16) + 2);
  if (((int64_t)P.N1 << 16) == bwtlen) P.N1 -= 1;
  P.N2 = (int32_t)(((bwtlen - 1) >> 8) + 2);
  if (((int64_t)P.N1 << 8) == bwtlen) P.N2 -= 1;      // (N1, not N2: the reference's expression)
  return P;
}
KJ_FB_HD uint64_t fb_samples_bytes(const FbPlan &P) { return (P.ncheck > 0 ? (uint64_t)P.ncheck : 0) * (uint64_t)P.nbytes; }

// device memory the stages allocate when the sort has ended (see the header comment for what they keep and free of the sort's)
KJ_FB_HD uint64_t fb_scratch_bytes(uint64_t tlen, uint64_t nseq, uint64_t copies, int chpt_exp) {
  const FbPlan P = fb_make_plan(tlen, nseq, tlen, copies, chpt_exp);      // (no sequence is longer than the text: nbytes from above)
  return fb_round_up(tlen, KJ_FB_PAD) + (P.copies > 1 ? fb_round_up(P.otlen, KJ_FB_PAD) : 0) + fb_round_up(fb_samples_bytes(P), KJ_FB_PAD) +
         2 * (uint64_t)KJ_FB_ALEN * P.nblk + 4 * (uint64_t)KJ_FB_ALEN * P.npieces + 3 * 4 * nseq + 8 * 256;
}
// ... of which the sort's scratch no longer holds (second key buffer 8, second value buffer 4, active list 4 per suffix)
KJ_FB_HD uint64_t fb_sort_bytes_freed(uint64_t nsuf) { return 16 * (nsuf ? nsuf : 1); }

// ---- BWT of the file -----------------------------------------------------------------------------------------------------
KJ_FB_HD uint8_t fb_bwt_of(const uint8_t *T, uint64_t p) { return p ? T[p - 1] : (uint8_t)0; }
// the sequence that starts at p (p > 0: the position in front is a terminator, whose rank is its sequence number)
KJ_FB_HD uint32_t fb_seq_starting_at(const uint32_t *rank, uint64_t p) { return p ? rank[p - 1] + 1u : 0u; }
// a terminator at p: its row of B, and the start of the sequence behind it
KJ_FB_HD void fb_terminator(const uint8_t *T, const uint32_t *rank, uint64_t p, uint64_t nseq, uint8_t *B, uint32_t *starts) {
  const uint64_t s = rank[p];
  if (s >= nseq) return;                             // (never: the sort gave every terminator its sequence number)
  B[s] = fb_bwt_of(T, p);                            // the last letter of the sequence, 0 for an empty one
  if (s + 1 < nseq) starts[s + 1] = (uint32_t)(p + 1);
  if (s == 0) starts[0] = 0;
}

// ---- sequence ranks ---------------------------------------------------------------------------------------------------
// row nseq + k holds a whole sequence; incl = inclusive scan of the flags at k
KJ_FB_HD void fb_seq_rank(const uint32_t *SA, const uint32_t *rank, uint64_t k, uint32_t incl, uint64_t r0, uint64_t nseq, uint32_t *read_of_rank,
                          uint32_t *rank_of) {
  const uint64_t r = r0 + incl - 1;
  const uint32_t i = fb_seq_starting_at(rank, SA[k]);
  if (r < nseq && i < nseq) { read_of_rank[r] = i; rank_of[i] = (uint32_t)r; }
}

// ---- replication: one lane, KJ_FB_REP_BYTES output rows from row j0 on, as one little-endian word --------------------------
KJ_FB_HD uint64_t fb_replicate(const uint8_t *B, uint64_t j0, uint64_t otlen, uint64_t copies) {
  uint64_t r = j0 / copies, t = j0 % copies, w = 0;
#pragma unroll
  for (int i = 0; i < KJ_FB_REP_BYTES; i++) {
    if (j0 + i < otlen) w |= (uint64_t)B[r] << (8 * i);
    if (++t == copies) { t = 0; r++; }
  }
  return w;
}

// ---- samples ----------------------------------------------------------------------------------------------------------
// the last i with starts[i] <= p (starts ascending, starts[0] = 0)
KJ_FB_HD uint32_t fb_seq_search(const uint32_t *starts, uint32_t nseq, uint32_t p) {
  uint32_t lo = 0, hi = nseq;
  for (int s = 0; s < KJ_FB_SEARCH_STEPS && hi - lo > 1; s++) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (starts[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}
KJ_FB_HD void fb_sample(const FbPlan &P, uint64_t q, const uint32_t *SA, const uint32_t *starts, const uint32_t *rank_of, uint8_t *out) {
  const uint64_t k = P.first + (q << P.chpt_exp);
  const uint64_t r = k / P.copies, t = k % P.copies;   // row of the file's own index, copy
  if (r < P.nseq || r - P.nseq >= P.nsuf) return;      // (never: first >= onseq and k < otlen)
  const uint32_t p = SA[r - P.nseq];
  const uint32_t i = fb_seq_search(starts, (uint32_t)P.nseq, p);
  uint64_t val = (((uint64_t)rank_of[i] * P.copies + t) << P.pbits) + (uint64_t)(p - starts[i]);
  uint8_t *c = out + q * (uint64_t)P.nbytes;
  for (int n = P.nbytes; n-- > 0;) { c[n] = (uint8_t)val; val >>= 8; }
}

// ---- checkpoints: one lane counts the letters of rows [lo, hi) of its block into cnt[a * stride] (zeroed by the caller);
//      bwt + lo is aligned to 8 and the array allocated to a multiple of KJ_FB_PAD -------------------------------------------
KJ_FB_HD void fb_count_block(const uint8_t *bwt, uint64_t lo, uint64_t hi, uint32_t *cnt, int stride) {
  const uint64_t *w = reinterpret_cast<const uint64_t *>(bwt + lo);
  for (uint64_t at = lo; at < hi; at += 8) {
    uint64_t v = *w++;
    for (int i = 0; i < 8 && at + i < hi; i++, v >>= 8) {
      const uint32_t c = (uint32_t)(v & 0xffu);
      if (c < KJ_FB_ALEN) cnt[c * stride]++;
    }
  }
}

// ---- byte coding (FMIrecode, compactfmi.c:399-440) ---------------------------------------------------------------------------
// One wavefront per block of 256 rows, lane l holds rows 4 l .. 4 l + 3 as one word.  bit[i][b] = the lanes whose row 4 l + i has
// bit b of its letter set, valid[i] = the lanes whose row 4 l + i exists (a short last block).
struct FbBallots { uint64_t bit[4][KJ_FB_SYM_BITS]; uint64_t valid[4]; };
KJ_FB_HD uint64_t fb_match(const FbBallots &B, int slot, uint32_t c) {          // the lanes whose row `slot` holds letter c
  uint64_t m = B.valid[slot];
#pragma unroll
  for (int b = 0; b < KJ_FB_SYM_BITS; b++) m &= ((c >> b) & 1u) ? B.bit[slot][b] : ~B.bit[slot][b];
  return m;
}
KJ_FB_HD uint8_t fb_code(const int *startLcode, uint32_t c, int n) {
  const int mx = startLcode[c + 1] - startLcode[c] - 1;
  if (n > mx) n = mx;
  return (uint8_t)(startLcode[c] + n);
}
KJ_FB_HD uint32_t fb_recode_lane(const FbBallots &B, int lane, uint32_t word, int nvalid, const int *startLcode) {
  const uint64_t below = (1ull << lane) - 1;
  uint32_t out = word;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int row = 4 * lane + i;
    const uint32_t c = (word >> (8 * i)) & 0xffu;
    if (row >= nvalid || c >= KJ_FB_ALEN) continue;
    int before = 0, total = 0;
#pragma unroll
    for (int i2 = 0; i2 < 4; i2++) {
      const uint64_t m = fb_match(B, i2, c);
      total += __builtin_popcountll(m);
      before += __builtin_popcountll(m & below);
      if (i2 < i) before += (int)((m >> lane) & 1u);
    }
    const int n = row < KJ_FB_BLOCK / 2 ? before : total - before - 1;      // rows j < 128 are first-half rows, whatever nvalid is
    out = (out & ~(0xffu << (8 * i))) | ((uint32_t)fb_code(startLcode, c, n) << (8 * i));
  }
  return out;
}

// ---- the driver (fmibuild.hip; host side, linked into libkaiju_mkfmi_gpu.so only) ------------------------------------------
#ifdef __cplusplus
#include <functional>
#include <string>
struct kaiju_fmi_build_stats;
// host buffers the driver fills (sized by the plan): read_of_rank[r0, nseq) - the caller numbers the r0 empty sequences -,
// samples[ncheck * nbytes], bwt[otlen] (coded, or raw with recode = 0), piece_counts[npieces * 21] (raw letter counts of the
// pieces), index2[nblk * 21] (the rows of the blocks that exist; the caller writes the tail rows)
struct FbHostOut { uint32_t *read_of_rank; uint8_t *samples; uint8_t *bwt; uint32_t *piece_counts; uint16_t *index2; };
// Sorts the text on the device and runs the five passes there.  r0: the number of empty sequences.  prepare() is called once the
// size check has passed and points FbHostOut at the host buffers; finish() is called with the piece counts when the checkpoint
// pass has ended and index2's rows are down, and returns startLcode[22]; mark() (may be empty) is told when the sort has ended.
// Blocking.  Status codes of mkfmi.h; err gets the message.
int kj_fmibuild_device(const uint8_t *text, const FbPlan &P, uint64_t r0, int device_id, int recode,
                       const std::function<void(FbHostOut &)> &prepare,
                       const std::function<void(const uint32_t *piece_counts, int *startLcode)> &finish,
                       const std::function<void(const char *)> &mark, kaiju_fmi_build_stats *stats, std::string &err);
#endif

#endif
