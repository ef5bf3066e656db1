// sufsort_wide_emu.cpp - the wide (64-bit) per-lane functions of kaiju_amd/csrc/kj_sufsort.h driven through the whole round
// loop on the host, pass by pass as the wide instantiation of sufsort.hip runs them: a round sorts twice, stable both times,
// by rank[p + h] and then by rank[p]; std::stable_sort stands in for the radix sort, a serial loop for the scans.  Every rank
// is rank_bias higher than the definition's, as on the device.  Test infrastructure (tests/test_sufsort_wide_emu.py,
// tests/tools/sufsort_wide_san.cpp).  It checks what the device cannot: the invariant of the load rank[p + h], that the rank of
// a final suffix never changes and that the active set only shrinks.  Behind it: the single functions with arguments of the
// caller's, for values beyond 2^32 that no text of a test's size reaches.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_sufsort.h"

namespace {
enum { V_LETTER_COUNT = 1, V_KEY_COUNT = 2, V_LOAD_INVARIANT = 4, V_FINAL_RANK_CHANGED = 8, V_ACTIVE_GREW = 16, V_FINAL_ACTIVE = 32,
       V_ROUND_BOUND = 64, V_RANK_RANGE = 128, V_ROW_TAKEN = 256, V_BOUND = 512 };

// stable, by the low `bits` bits of the keys, as the radix sort: keys and vals reordered together
void sort_pairs(std::vector<uint64_t> &keys, std::vector<uint64_t> &vals, int bits) {
  const size_t m = keys.size();
  const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
  std::vector<size_t> order(m);
  for (size_t i = 0; i < m; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return (keys[a] & mask) < (keys[b] & mask); });
  std::vector<uint64_t> sk(m), sv(m);
  for (size_t i = 0; i < m; i++) { sk[i] = keys[order[i]]; sv[i] = vals[order[i]]; }
  keys.swap(sk); vals.swap(sv);
}
int bits_of(uint64_t v) { int b = 0; while (v >> b) ++b; return b; }
}  // namespace

// sa_out: room for the letters of the text; active_out: 64 entries (active[r] = suffixes not final in front of round r + 1).
// Returns the violations seen (0 = none).
extern "C" uint32_t sufsort_wide_emu(const uint8_t *text, uint64_t tlen, uint64_t rank_bias, uint64_t *sa_out, uint64_t *n_out, uint32_t *rounds_out,
                                     uint64_t *active_out) {
  uint32_t bad = 0;
  *n_out = 0; *rounds_out = 0;
  for (int r = 0; r < 64; r++) active_out[r] = 0;
  if (tlen >= (1ull << 40) || rank_bias >= (1ull << 40) || !ss_tlen_ok_wide(tlen + rank_bias)) return V_BOUND;
  std::vector<uint8_t> T((size_t)ss_text_alloc(tlen), 0);
  memcpy(T.data(), text, (size_t)tlen);
  const uint64_t nlanes = (tlen + KJ_SS_LANE_BYTES - 1) / KJ_SS_LANE_BYTES;
  uint64_t nseq = 0, maxlen = 0, run = 0;
  std::vector<uint64_t> next_term((size_t)tlen + 1, tlen);
  for (uint64_t p = 0; p < tlen; p++) { if (T[p]) run++; else { nseq++; maxlen = std::max(maxlen, run); run = 0; } }
  for (uint64_t p = tlen; p-- > 0;) next_term[p] = T[p] ? next_term[p + 1] : p;
  const uint64_t nsuf = tlen - nseq, first_rank = rank_bias + nseq;
  const int round_bits = bits_of(rank_bias + tlen);
  *n_out = nsuf;
  if (nsuf == 0) return 0;

  // ---- round 1: keys lane by lane; a tile's base is the letters in front of it ----
  std::vector<uint64_t> rank((size_t)tlen, 0);
  std::vector<uint64_t> keys, vals;
  uint64_t counted = 0, tile_base = 0;
  uint32_t in_tile = 0;
  for (uint64_t g = 0; g < nlanes; g++) {
    uint64_t w[4];
    memcpy(w, T.data() + g * KJ_SS_LANE_BYTES, 32);
    uint64_t k[KJ_SS_LANE_BYTES];
    const uint32_t letters = ss_lane_keys(w, k);
    if ((uint32_t)__builtin_popcount(letters) != ss_lane_letters(w[0], w[1])) bad |= V_LETTER_COUNT;
    if (g % KJ_SS_BLOCK == 0) { tile_base = counted; in_tile = 0; }
    const uint32_t cnt = ss_lane_letters(w[0], w[1]);
    uint64_t o = ss_lane_base(tile_base, in_tile, cnt, cnt);          // (the inclusive count of the lane minus its own)
    if (o != keys.size()) bad |= V_LETTER_COUNT;
    counted += cnt; in_tile += cnt;
    for (int j = 0; j < KJ_SS_LANE_BYTES; j++) {
      const uint64_t p = g * KJ_SS_LANE_BYTES + j;
      if ((letters >> j) & 1u) { keys.push_back(k[j]); vals.push_back(p); o++; }
      else if (p < tlen) rank[(size_t)p] = rank_bias + (p - o);
    }
  }
  if (counted != nsuf || keys.size() != nsuf) return bad | V_KEY_COUNT;

  std::vector<uint8_t> is_final((size_t)tlen, 0);
  std::vector<uint64_t> act;
  std::vector<SsScanItemW> items;
  uint64_t m = nsuf, h = 0;
  uint32_t rounds = 0;
  for (;;) {
    const bool first = rounds == 0;
    if (rounds < 64) active_out[rounds] = m;
    if (first) {
      sort_pairs(keys, vals, KJ_SS_KEY_BITS);
    } else {
      if (!ss_round_allowed(h, maxlen)) return bad | V_ROUND_BOUND;
      keys.resize((size_t)m); vals.resize((size_t)m);
      for (uint64_t i = 0; i < m; i++) {                      // k_ss_round_keys: rank[p + h]
        const uint64_t p = act[(size_t)i];
        if (is_final[(size_t)p]) bad |= V_FINAL_ACTIVE;
        if (p + h >= tlen || next_term[(size_t)p] < p + h) bad |= V_LOAD_INVARIANT;
        keys[(size_t)i] = ss_rank_ahead(rank.data(), p, h, tlen);
        vals[(size_t)i] = p;
      }
      sort_pairs(keys, vals, round_bits);
      for (uint64_t i = 0; i < m; i++) keys[(size_t)i] = rank[(size_t)vals[(size_t)i]];      // k_ss_round_keys_hi: rank[p]
      sort_pairs(keys, vals, round_bits);
    }
    // heads, scan
    items.resize((size_t)m);
    for (uint64_t i = 0; i < m; i++) {
      const uint64_t k = keys[(size_t)i], kp = i ? keys[(size_t)i - 1] : 0;
      if (first) {
        items[(size_t)i] = ss_scan_item_wide(i, false, ss_head_first(i, kp, k));
      } else {
        const SsKeyW key = {k, ss_rank_ahead(rank.data(), vals[(size_t)i], h, tlen)}, prev = {kp, i ? ss_rank_ahead(rank.data(), vals[(size_t)i - 1], h, tlen) : 0};
        const SsKeyW whole = ss_round_key(rank.data(), vals[(size_t)i], h, tlen);
        if (whole.hi != key.hi || whole.lo != key.lo) bad |= V_KEY_COUNT;       // the sorted key buffer still holds rank[p]
        items[(size_t)i] = ss_scan_item_wide(i, ss_head_old(i, prev, key), ss_head_new(i, prev, key));
      }
    }
    for (uint64_t i = 1; i < m; i++) items[(size_t)i] = SsScanMaxW()(items[(size_t)i - 1], items[(size_t)i]);
    // ranks, flags, compaction
    std::vector<uint64_t> next_act;
    for (uint64_t i = 0; i < m; i++) {
      const SsScanItemW s = items[(size_t)i], sn = i + 1 < m ? items[(size_t)i + 1] : SsScanItemW();
      const uint64_t p = vals[(size_t)i];
      const SsKeyW key = {keys[(size_t)i], 0};
      const uint64_t r = first ? ss_rank_first(first_rank, s) : ss_rank_round(key, s);
      if (is_final[(size_t)p] && rank[(size_t)p] != r) bad |= V_FINAL_RANK_CHANGED;
      if (r < first_rank || r - first_rank >= nsuf) bad |= V_RANK_RANGE;
      rank[(size_t)p] = r;
      if (ss_is_final(i, m, s, sn)) is_final[(size_t)p] = 1; else next_act.push_back(p);
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
    const uint64_t row = rank[(size_t)p] - first_rank;
    if (row >= nsuf) { bad |= V_RANK_RANGE; continue; }
    if (taken[(size_t)row]) bad |= V_ROW_TAKEN;
    taken[(size_t)row] = 1;
    sa_out[row] = p;
  }
  return bad;
}

// ---- the single functions ---------------------------------------------------------------------------------------------------
// rank[p] = r_p and rank[p + h] = r_ph through an array of two entries and a pointer moved back by p entries (h = 1);
// out = {hi, lo, the ahead load alone, the ahead load with tlen = p + 1: outside the text}
extern "C" void sufsort_wide_emu_round_key(uint64_t r_p, uint64_t r_ph, uint64_t p, uint64_t *out) {
  const uint64_t two[2] = {r_p, r_ph};
  const uint64_t *rank = reinterpret_cast<const uint64_t *>(reinterpret_cast<uintptr_t>(two) - (uintptr_t)p * 8u);
  const SsKeyW k = ss_round_key(rank, p, 1, p + 2);
  out[0] = k.hi; out[1] = k.lo; out[2] = ss_rank_ahead(rank, p, 1, p + 2); out[3] = ss_rank_ahead(rank, p, 1, p + 1);
}
// bit 0: head of the old order, bit 1: of the new one
extern "C" uint32_t sufsort_wide_emu_heads(uint64_t i, uint64_t prev_hi, uint64_t prev_lo, uint64_t hi, uint64_t lo) {
  const SsKeyW prev = {prev_hi, prev_lo}, key = {hi, lo};
  return (ss_head_old(i, prev, key) ? 1u : 0u) | (ss_head_new(i, prev, key) ? 2u : 0u);
}
extern "C" void sufsort_wide_emu_scan(uint64_t a_old, uint64_t a_new, uint64_t b_old, uint64_t b_new, uint64_t *out) {
  const SsScanItemW a = {a_old, a_new}, b = {b_old, b_new}, s = SsScanMaxW()(a, b);
  out[0] = s.old_head; out[1] = s.new_head;
}
extern "C" void sufsort_wide_emu_scan_item(uint64_t i, int head_old, int head_new, uint64_t *out) {
  const SsScanItemW s = ss_scan_item_wide(i, head_old != 0, head_new != 0);
  out[0] = s.old_head; out[1] = s.new_head;
}
extern "C" uint64_t sufsort_wide_emu_rank_first(uint64_t first_rank, uint64_t new_head) {
  const SsScanItemW s = {0, new_head};
  return ss_rank_first(first_rank, s);
}
extern "C" uint64_t sufsort_wide_emu_rank_round(uint64_t old_rank, uint64_t old_head, uint64_t new_head) {
  const SsKeyW k = {old_rank, 0};
  const SsScanItemW s = {old_head, new_head};
  return ss_rank_round(k, s);
}
extern "C" int sufsort_wide_emu_is_final(uint64_t i, uint64_t n, uint64_t new_head, uint64_t new_head_next) {
  const SsScanItemW s = {0, new_head}, sn = {0, new_head_next};
  return ss_is_final(i, n, s, sn) ? 1 : 0;
}
extern "C" uint64_t sufsort_wide_emu_lane_base(uint64_t tile_base, uint32_t before, uint32_t inc, uint32_t cnt) { return ss_lane_base(tile_base, before, inc, cnt); }
extern "C" int sufsort_wide_emu_tlen_ok_wide(uint64_t v) { return ss_tlen_ok_wide(v) ? 1 : 0; }
extern "C" int sufsort_wide_emu_tlen_ok(uint64_t v) { return ss_tlen_ok(v) ? 1 : 0; }
extern "C" uint64_t sufsort_wide_emu_scratch_bytes_wide(uint64_t tlen, uint64_t nsuf) { return ss_scratch_bytes_wide(tlen, nsuf); }
extern "C" uint64_t sufsort_wide_emu_scratch_bytes(uint64_t tlen, uint64_t nsuf) { return ss_scratch_bytes(tlen, nsuf); }
