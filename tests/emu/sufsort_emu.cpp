// sufsort_emu.cpp - the per-lane functions of kaiju_amd/csrc/kj_sufsort.h driven through the whole round loop on the host, pass
// by pass as sufsort.hip runs them; std::stable_sort stands in for the radix sort, a serial loop for the scans.  Test
// infrastructure (tests/test_sufsort_emu.py).  On the way it checks what the device cannot: the invariant of the load
// rank[p + h], that the rank of a final suffix never changes and that the active set only shrinks.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_sufsort.h"

namespace {
enum { V_LETTER_COUNT = 1, V_KEY_COUNT = 2, V_LOAD_INVARIANT = 4, V_FINAL_RANK_CHANGED = 8, V_ACTIVE_GREW = 16, V_FINAL_ACTIVE = 32,
       V_ROUND_BOUND = 64, V_RANK_RANGE = 128, V_ROW_TAKEN = 256 };
}

extern "C" void sufsort_emu_constants(uint64_t *out) {
  out[0] = KJ_SS_K; out[1] = KJ_SS_TILE; out[2] = KJ_SS_LANE_BYTES; out[3] = KJ_SS_STATS_ROUNDS;
  out[4] = ss_tlen_ok(0xefffffffull) ? 1 : 0; out[5] = ss_tlen_ok(0xf0000000ull) ? 1 : 0;
}
extern "C" uint64_t sufsort_emu_scratch_bytes(uint64_t tlen, uint64_t nsuf) { return ss_scratch_bytes(tlen, nsuf); }

// sa_out: room for the letters of the text; active_out: 64 entries (active[r] = suffixes not final in front of round r + 1).
// Returns the violations seen (0 = none).
extern "C" uint32_t sufsort_emu(const uint8_t *text, uint64_t tlen, uint32_t *sa_out, uint64_t *n_out, uint32_t *rounds_out, uint64_t *active_out) {
  uint32_t bad = 0;
  std::vector<uint8_t> T((size_t)ss_text_alloc(tlen), 0);
  memcpy(T.data(), text, (size_t)tlen);
  const uint64_t nlanes = (tlen + KJ_SS_LANE_BYTES - 1) / KJ_SS_LANE_BYTES;
  uint64_t nseq = 0, maxlen = 0, run = 0;
  std::vector<uint64_t> next_term((size_t)tlen + 1, tlen);
  for (uint64_t p = 0; p < tlen; p++) { if (T[p]) run++; else { nseq++; maxlen = std::max(maxlen, run); run = 0; } }
  for (uint64_t p = tlen; p-- > 0;) next_term[p] = T[p] ? next_term[p + 1] : p;
  const uint64_t nsuf = tlen - nseq;
  *n_out = nsuf; *rounds_out = 0;
  for (int r = 0; r < 64; r++) active_out[r] = 0;
  if (nsuf == 0) return 0;

  // ---- round 1: keys lane by lane ----
  std::vector<uint32_t> rank((size_t)tlen, 0);
  std::vector<uint64_t> keys; std::vector<uint32_t> vals;
  uint64_t counted = 0;
  for (uint64_t g = 0; g < nlanes; g++) {
    uint64_t w[4];
    memcpy(w, T.data() + g * KJ_SS_LANE_BYTES, 32);
    uint64_t k[KJ_SS_LANE_BYTES];
    const uint32_t letters = ss_lane_keys(w, k);
    if ((uint32_t)__builtin_popcount(letters) != ss_lane_letters(w[0], w[1])) bad |= V_LETTER_COUNT;
    counted += ss_lane_letters(w[0], w[1]);
    for (int j = 0; j < KJ_SS_LANE_BYTES; j++) {
      const uint64_t p = g * KJ_SS_LANE_BYTES + j;
      if ((letters >> j) & 1u) { keys.push_back(k[j]); vals.push_back((uint32_t)p); }
      else if (p < tlen) rank[(size_t)p] = (uint32_t)(p - keys.size());
    }
  }
  if (counted != nsuf || keys.size() != nsuf) return bad | V_KEY_COUNT;

  std::vector<uint8_t> is_final((size_t)tlen, 0);
  std::vector<uint32_t> act;
  std::vector<uint64_t> items;
  std::vector<uint32_t> order;
  uint64_t m = nsuf, h = 0;
  uint32_t rounds = 0;
  for (;;) {
    const bool first = rounds == 0;
    if (rounds < 64) active_out[rounds] = m;
    if (!first) {
      if (!ss_round_allowed(h, maxlen)) return bad | V_ROUND_BOUND;
      keys.resize((size_t)m); vals.resize((size_t)m);
      for (uint64_t i = 0; i < m; i++) {
        const uint32_t p = act[(size_t)i];
        if (is_final[p]) bad |= V_FINAL_ACTIVE;
        if ((uint64_t)p + h >= tlen || next_term[p] < (uint64_t)p + h) bad |= V_LOAD_INVARIANT;
        keys[(size_t)i] = ss_round_key(rank.data(), p, h, tlen);
        vals[(size_t)i] = p;
      }
    }
    // the sort: stable, by the bits the device sorts by
    order.resize((size_t)m);
    for (uint64_t i = 0; i < m; i++) order[(size_t)i] = (uint32_t)i;
    const uint64_t mask = first ? (1ull << KJ_SS_KEY_BITS) - 1 : ~0ull;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return (keys[a] & mask) < (keys[b] & mask); });
    std::vector<uint64_t> sk((size_t)m); std::vector<uint32_t> sv((size_t)m);
    for (uint64_t i = 0; i < m; i++) { sk[(size_t)i] = keys[order[(size_t)i]]; sv[(size_t)i] = vals[order[(size_t)i]]; }
    // heads, scan
    items.resize((size_t)m);
    for (uint64_t i = 0; i < m; i++) {
      const uint64_t k = sk[(size_t)i], kp = i ? sk[(size_t)i - 1] : 0;
      items[(size_t)i] = first ? ss_scan_item((uint32_t)i, false, ss_head_first(i, kp, k)) : ss_scan_item((uint32_t)i, ss_head_old(i, kp, k), ss_head_new(i, kp, k));
    }
    for (uint64_t i = 1; i < m; i++) items[(size_t)i] = SsScanMax()(items[(size_t)i - 1], items[(size_t)i]);
    // ranks, flags, compaction
    std::vector<uint32_t> next_act;
    for (uint64_t i = 0; i < m; i++) {
      const uint64_t s = items[(size_t)i], sn = i + 1 < m ? items[(size_t)i + 1] : 0;
      const uint32_t p = sv[(size_t)i];
      const uint32_t r = first ? ss_rank_first((uint32_t)nseq, s) : ss_rank_round(sk[(size_t)i], s);
      if (is_final[p] && rank[p] != r) bad |= V_FINAL_RANK_CHANGED;
      if (r < nseq || r - nseq >= nsuf) bad |= V_RANK_RANGE;
      rank[p] = r;
      if (ss_is_final(i, m, s, sn)) is_final[p] = 1; else next_act.push_back(p);
    }
    rounds++;
    h = first ? (uint64_t)KJ_SS_K : 2 * h;
    if (next_act.size() > m) bad |= V_ACTIVE_GREW;
    act.swap(next_act);
    m = act.size();
    if (m == 0) break;
  }
  *rounds_out = rounds;
  std::vector<uint8_t> taken((size_t)nsuf, 0);
  for (uint64_t p = 0; p < tlen; p++) if (T[p]) {
    const uint64_t row = (uint64_t)rank[(size_t)p] - nseq;
    if (row >= nsuf) { bad |= V_RANK_RANGE; continue; }
    if (taken[(size_t)row]) bad |= V_ROW_TAKEN;
    taken[(size_t)row] = 1;
    sa_out[row] = (uint32_t)p;
  }
  return bad;
}
