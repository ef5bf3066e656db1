// fmibuild_emu.cpp - the per-lane functions of kaiju_amd/csrc/kj_fmibuild.h driven on the host through loops shaped like the grids
// of fmibuild.hip, pass by pass: a serial loop stands in for the scans, a loop over 64 lanes for the ballots.  Test
// infrastructure (tests/test_fmibuild_emu.py, tests/tools/fmibuild_san.cpp).  The inputs are what the device holds when the sort
// has ended - the text, SA and rank[], made here as the inverse of the row order - and the code table, which is the host's.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_fmibuild.h"
#include "../../kaiju_amd/csrc/kj_sufsort.h"

namespace {
enum { V_SA = 1, V_RANK_TOTAL = 2, V_RANK_TWICE = 4, V_STARTS = 8, V_PLAN = 16 };
}

extern "C" void fmibuild_emu_constants(uint64_t *out) {
  out[0] = KJ_FB_BLOCK; out[1] = KJ_FB_PIECE; out[2] = KJ_FB_ALEN; out[3] = KJ_FB_THREADS; out[4] = KJ_FB_REP_BYTES; out[5] = KJ_FB_SEARCH_STEPS;
  out[6] = KJ_FB_STAGES_ALL; out[7] = KJ_FB_PAD;
}
extern "C" uint64_t fmibuild_emu_scratch_bytes(uint64_t tlen, uint64_t nseq, uint64_t copies, int chpt_exp) { return fb_scratch_bytes(tlen, nseq, copies, chpt_exp); }
extern "C" uint64_t fmibuild_emu_sort_bytes_freed(uint64_t nsuf) { return fb_sort_bytes_freed(nsuf); }
// plan[0..11]: otlen, onseq, first, nsamp, nfill, nblk, npieces, ncheck, sbits, pbits, nbytes, N1, N2
extern "C" void fmibuild_emu_plan(uint64_t tlen, uint64_t nseq, uint64_t maxlen, uint64_t copies, int chpt_exp, int64_t *plan) {
  const FbPlan P = fb_make_plan(tlen, nseq, maxlen, copies, chpt_exp);
  const int64_t v[13] = {(int64_t)P.otlen, (int64_t)P.onseq, (int64_t)P.first, (int64_t)P.nsamp, (int64_t)P.nfill, (int64_t)P.nblk, (int64_t)P.npieces,
                         P.ncheck, P.sbits, P.pbits, P.nbytes, P.N1, P.N2};
  for (int k = 0; k < 13; k++) plan[k] = v[k];
}

// text[0, tlen) with its suffix array sa[0, nsuf); startLcode[22]: the host's table.  Out: read_of_rank[nseq] (the entries of the
// empty sequences in front, as the host numbers them), samples[ncheck * nbytes], bwt[tlen * copies] (coded with recode != 0),
// piece_counts[npieces * 21], index2_rows[nblk * 21].  Returns the violations seen (0 = none).
extern "C" uint32_t fmibuild_emu(const uint8_t *text, uint64_t tlen, const uint32_t *sa, uint64_t copies, int chpt_exp, const int *startLcode, int recode,
                                 uint32_t *read_of_rank, uint8_t *samples, uint8_t *bwt_out, uint32_t *piece_counts, uint16_t *index2_rows) {
  uint32_t bad = 0;
  // ---- what the sort leaves: padded text, rank[] ----
  std::vector<uint8_t> T((size_t)ss_text_alloc(tlen), 0);
  memcpy(T.data(), text, (size_t)tlen);
  uint64_t nseq = 0, maxlen = 0, run = 0, r0 = 0;
  for (uint64_t p = 0; p < tlen; p++) { if (T[p]) run++; else { nseq++; maxlen = std::max(maxlen, run); r0 += run == 0; run = 0; } }
  const uint64_t nsuf = tlen - nseq;
  std::vector<uint32_t> rank((size_t)tlen, 0);
  { uint32_t s = 0; for (uint64_t p = 0; p < tlen; p++) if (!T[p]) rank[(size_t)p] = s++; }
  for (uint64_t k = 0; k < nsuf; k++) { if (sa[k] >= tlen || !T[sa[k]]) return V_SA; rank[sa[k]] = (uint32_t)(nseq + k); }
  const FbPlan P = fb_make_plan(tlen, nseq, maxlen, copies, chpt_exp);
  if (P.nsuf != nsuf || P.otlen != tlen * P.copies) return V_PLAN;
  const uint64_t otlen = P.otlen;

  // ---- BWT of the file: rows by k, terminators by words of four text bytes ----
  std::vector<uint8_t> B((size_t)fb_round_up(tlen, KJ_FB_PAD), 0xee);
  std::vector<uint32_t> starts((size_t)nseq, 0), rank_of((size_t)nseq, 0), ror((size_t)nseq, 0xffffffffu);
  for (uint64_t k = 0; k < nsuf; k++) B[(size_t)(nseq + k)] = fb_bwt_of(T.data(), sa[k]);
  for (uint64_t g = 0; g < (tlen + 3) / 4; g++) {
    uint32_t w;
    memcpy(&w, T.data() + g * 4, 4);
    for (int j = 0; j < 4; j++) {
      const uint64_t p = g * 4 + j;
      if (p < tlen && ((w >> (8 * j)) & 0xffu) == 0) fb_terminator(T.data(), rank.data(), p, nseq, B.data(), starts.data());
    }
  }
  for (uint64_t i = 0, b = 0, p = 0; p < tlen; p++) if (!T[p]) { if (starts[(size_t)i] != b) bad |= V_STARTS; i++; b = p + 1; }

  // ---- sequence ranks: flags, inclusive scan, ranks ----
  std::vector<uint32_t> flags((size_t)nsuf, 0);
  for (uint64_t k = 0; k < nsuf; k++) flags[(size_t)k] = B[(size_t)(nseq + k)] == 0 ? 1u : 0u;
  for (uint64_t k = 1; k < nsuf; k++) flags[(size_t)k] += flags[(size_t)k - 1];
  for (uint64_t k = 0; k < nsuf; k++) if (B[(size_t)(nseq + k)] == 0) {
    const uint64_t r = r0 + flags[(size_t)k] - 1;
    if (r < nseq && ror[(size_t)r] != 0xffffffffu) bad |= V_RANK_TWICE;
    fb_seq_rank(sa, rank.data(), k, flags[(size_t)k], r0, nseq, ror.data(), rank_of.data());
  }
  if (r0 + (nsuf ? flags[(size_t)nsuf - 1] : 0u) != nseq) bad |= V_RANK_TOTAL;
  { uint32_t r = 0; for (uint64_t i = 0, b = 0, p = 0; p < tlen; p++) if (!T[p]) { if (p == b) ror[r++] = (uint32_t)i; i++; b = p + 1; } }   // the host's part
  for (uint64_t r = 0; r < nseq; r++) read_of_rank[r] = ror[(size_t)r];

  // ---- replication by words of eight rows, samples ----
  std::vector<uint64_t> bwt64((size_t)(fb_round_up(otlen, KJ_FB_PAD) / 8), 0xeeeeeeeeeeeeeeeeull);
  uint8_t *bwt = reinterpret_cast<uint8_t *>(bwt64.data());
  if (P.copies > 1) { for (uint64_t g = 0; g < (otlen + KJ_FB_REP_BYTES - 1) / KJ_FB_REP_BYTES; g++) bwt64[(size_t)g] = fb_replicate(B.data(), g * KJ_FB_REP_BYTES, otlen, P.copies); }
  else memcpy(bwt, B.data(), (size_t)tlen);
  if (fb_samples_bytes(P)) memset(samples, 0, (size_t)fb_samples_bytes(P));
  for (uint64_t q = 0; q < P.nfill; q++) fb_sample(P, q, sa, starts.data(), rank_of.data(), samples);

  // ---- checkpoints: a workgroup per piece, a lane per block ----
  std::vector<uint32_t> cnt((size_t)KJ_FB_ALEN * KJ_FB_THREADS);
  for (uint64_t R = 0; R < P.npieces; R++) {
    std::fill(cnt.begin(), cnt.end(), 0u);
    for (int t = 0; t < KJ_FB_THREADS; t++) {
      const uint64_t lo = R * KJ_FB_PIECE + (uint64_t)t * KJ_FB_BLOCK, hi = std::min<uint64_t>(lo + KJ_FB_BLOCK, otlen);
      if (lo < otlen) fb_count_block(bwt, lo, hi, cnt.data() + t, KJ_FB_THREADS);
    }
    for (int a = 0; a < KJ_FB_ALEN; a++) {
      uint32_t excl = 0;
      for (int t = 0; t < KJ_FB_THREADS; t++) {
        const uint64_t lo = R * KJ_FB_PIECE + (uint64_t)t * KJ_FB_BLOCK;
        if (lo < otlen) index2_rows[(R * KJ_FB_THREADS + t) * KJ_FB_ALEN + a] = (uint16_t)excl;
        excl += cnt[(size_t)a * KJ_FB_THREADS + t];
      }
      piece_counts[R * KJ_FB_ALEN + a] = excl;
    }
  }

  // ---- byte coding: a wavefront per block ----
  if (recode) {
    uint32_t *bwt32 = reinterpret_cast<uint32_t *>(bwt);
    for (uint64_t blk = 0; blk < P.nblk; blk++) {
      const uint64_t left = otlen - blk * KJ_FB_BLOCK;
      const int nvalid = left < KJ_FB_BLOCK ? (int)left : (int)KJ_FB_BLOCK;
      uint32_t word[64];
      FbBallots bal;
      memset(&bal, 0, sizeof bal);
      for (int lane = 0; lane < 64; lane++) {
        word[lane] = bwt32[blk * 64 + lane];
        for (int i = 0; i < 4; i++) {
          if (4 * lane + i < nvalid) bal.valid[i] |= 1ull << lane;
          for (int b = 0; b < KJ_FB_SYM_BITS; b++) if ((word[lane] >> (8 * i + b)) & 1u) bal.bit[i][b] |= 1ull << lane;
        }
      }
      for (int lane = 0; lane < 64; lane++) bwt32[blk * 64 + lane] = fb_recode_lane(bal, lane, word[lane], nvalid, startLcode);
    }
  }
  memcpy(bwt_out, bwt, (size_t)otlen);
  return bad;
}
