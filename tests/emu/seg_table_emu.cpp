// seg_table_emu.cpp — TEST INFRASTRUCTURE ONLY.
//
// The window-probability table of s_Trim (kj_core.h: seg_prob_lookup; host_tables.cpp: seg_prob_table) on the host: every
// entry against seg_prob_of_counts, the paths that must not use it, and the SEG regions of a peptide with one lane.  Built
// twice by tests/test_seg_prob_table.py: as it is, and with -DKJ_SEG_NO_TABLE (direct evaluation of every window).  No index:
// SEG looks at the identity of letters only, so the peptides are coded by a fixed alphabet.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../kaiju_amd/csrc/host_tables.h"
#include "../../kaiju_amd/csrc/kj_core.h"

using namespace kj;

namespace kj { unsigned long long kj_seg_hist[4][64]; }   // (this library is built with -DKJ_SEG_HIST)

namespace {
struct State {
  SegTables st;
  std::vector<double> lnfact;
  bool ok = false;
} g;

uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
uint64_t rng_next(uint64_t &x) {                 // splitmix64
  uint64_t z = (x += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
void pack(const int *cnt, uint64_t &c0, uint64_t &c1) {
  c0 = c1 = 0;
  for (int a = 0; a < 20; a++)
    if (a < 10) c0 += (uint64_t)cnt[a] << (6 * a); else c1 += (uint64_t)cnt[a] << (6 * (a - 10));
}
// slots seg_prob_lookup looks at before it finds `key` in the table (0: not there)
uint32_t probes_of(const SegProbTable &t, uint64_t key) {
  uint32_t slot = (uint32_t)key & t.mask;
  for (uint32_t n = 1; n <= t.mask + 1; n++, slot = (slot + 1u) & t.mask) {
    if (t.slots[slot].key == key) return n;
    if (t.slots[slot].key == 0) return 0;
  }
  return 0;
}
struct Walk {
  SegCtx cx;
  uint64_t seed;
  uint64_t entries = 0, mismatches = 0, missing = 0;
  uint32_t max_probe = 0;
  std::vector<uint64_t> keys;
};
// every partition of `remaining` into parts <= maxpart, at most 20 in all; its parts dealt to the 20 letters at random
void walk(int remaining, int maxpart, int *sv, int n, int l, Walk &w) {
  if (remaining == 0) {
    int cnt[20] = {0};
    int order[20];
    for (int a = 0; a < 20; a++) order[a] = a;
    for (int a = 19; a > 0; a--) { const int b = (int)(rng_next(w.seed) % (uint64_t)(a + 1)); std::swap(order[a], order[b]); }
    for (int k = 0; k < n; k++) cnt[order[k]] = sv[k];
    uint64_t c0, c1;
    pack(cnt, c0, c1);
    const double direct = seg_prob_of_counts(w.cx, c0, c1, l);
    double got = 0.;
    w.entries++;
    if (!seg_prob_lookup(w.cx, c0, c1, got)) w.missing++;
    else if (bits(got) != bits(direct)) w.mismatches++;
    const uint64_t key = seg_counts_key(w.cx.tab_T, c0, c1);
    w.keys.push_back(key);
    const uint32_t pr = probes_of(seg_prob_table(), key);
    if (pr > w.max_probe) w.max_probe = pr;
    return;
  }
  if (n == 20) return;
  for (int p = remaining < maxpart ? remaining : maxpart; p >= 1; p--) {
    sv[n] = p;
    walk(remaining - p, p, sv, n + 1, l, w);
  }
}
// the context of the lookups: the process-wide table, whatever KJ_SEG_NO_TABLE left in SegTables
SegCtx table_ctx() {
  const SegProbTable &t = seg_prob_table();
  SegTables st = g.st;
  st.ptab = t.slots.data(); st.ptab_T = t.T; st.ptab_mask = t.mask; st.ptab_probe = t.probe; st.ptab_max = (uint32_t)kSegTabMax;
  return seg_ctx(st, st.ent_g, st.lnfact);
}
}  // namespace

extern "C" {

// 0, or -1 with the message of build_seg_tables
int ste_open(char *err, int errlen) {
  std::string msg;
  const int rc = build_seg_tables(g.lnfact, g.st, msg);
  if (rc) { snprintf(err, (size_t)errlen, "%s", msg.c_str()); return -1; }
  g.ok = true;
  return 0;
}
// out[0] kSegTabMax, [1] entries, [2] slots, [3] recorded probe bound, [4] 1: SegTables points at the table (0: KJ_SEG_NO_TABLE),
// [5] occupied slots
void ste_info(uint64_t *out) {
  const SegProbTable &t = seg_prob_table();
  out[0] = (uint64_t)kSegTabMax; out[1] = t.entries; out[2] = t.slots.size(); out[3] = t.probe; out[4] = g.st.ptab ? 1 : 0;
  uint64_t occ = 0;
  for (const SegProbEntry &e : t.slots) occ += e.key != 0;
  out[5] = occ;
}
// every partition of every l <= kSegTabMax into at most 20 parts, parts dealt to the letters by `seed`:
// out[0] partitions, [1] lookups whose bit pattern differs from seg_prob_of_counts, [2] lookups that found nothing,
// [3] distinct keys, [4] the longest probe sequence of any of them
void ste_check_entries(uint64_t seed, uint64_t *out) {
  Walk w{table_ctx(), seed};
  int sv[20];
  for (int l = 1; l <= kSegTabMax; l++) walk(l, l, sv, 0, l, w);
  std::sort(w.keys.begin(), w.keys.end());
  out[0] = w.entries; out[1] = w.mismatches; out[2] = w.missing;
  out[3] = (uint64_t)(std::unique(w.keys.begin(), w.keys.end()) - w.keys.begin());
  out[4] = w.max_probe;
}
// A window given by its 20 counts: out[0] 1: seg_prob_lookup finds it in the table, [1] 1: what it found has the bit pattern of
// seg_prob_of_counts
void ste_window(const int *cnt, uint64_t *out) {
  const SegCtx cx = table_ctx();
  uint64_t c0, c1;
  pack(cnt, c0, c1);
  int l = 0;
  for (int a = 0; a < 20; a++) l += cnt[a];
  double got = 0.;
  out[0] = seg_prob_lookup(cx, c0, c1, got) ? 1 : 0;
  out[1] = out[0] && bits(got) == bits(seg_prob_of_counts(cx, c0, c1, l)) ? 1 : 0;
}
// SEG regions of an ASCII peptide by one lane (the table as this library was built: on, or off with KJ_SEG_NO_TABLE).
// use_prefix 0: seg_trim without prefix counts (every window counts its letters: never the table).  drop (20 counts or NULL):
// the entry of that multiset is taken out of a copy of the table first - a key that is absent although its window length is
// covered.  Returns the number of merged regions or -1 (scan lists overflowed); hist[4 * 64] receives the counters of the call
// (kj_core.h: KJ_SEG_HISTO)
int ste_seg(const char *aa, int len, int use_prefix, const int *drop, int32_t *left, int32_t *right, uint64_t *hist) {
  static const char kLetters[21] = "ACDEFGHIKLMNPQRSTVWY";
  std::vector<uint8_t> codes((size_t)len + 1, 0);
  for (int i = 0; i < len; i++) {
    const char *p = strchr(kLetters, aa[i]);
    if (!p || !aa[i]) return -2;
    codes[(size_t)i] = (uint8_t)(p - kLetters + 1);
  }
  static thread_local uint64_t pref[2 * (kSegPacked + 1)];
  CoopSerial coop;
  coop.prefix = use_prefix ? pref : nullptr;
  SegCtx cx = seg_ctx(g.st, g.st.ent_g, g.st.lnfact);
  std::vector<SegProbEntry> copy;
  if (drop && cx.tab) {
    const SegProbTable &t = seg_prob_table();
    uint64_t c0, c1;
    pack(drop, c0, c1);
    const uint64_t key = seg_counts_key(t.T, c0, c1);
    copy = t.slots;
    for (SegProbEntry &e : copy) if (e.key == key) e.key = ~0ull;       // (a tombstone: the probe sequences of the others stay whole)
    cx.tab = copy.data();
  }
  int32_t work[2 * kSegMaxRegions];
  std::vector<uint8_t> cls((size_t)len + 1);
  bool ov = false;
  memset(kj_seg_hist, 0, sizeof kj_seg_hist);
  const int n = seg_regions(cx, coop, codes.data(), len, left, right, ov, work, cls.data(), [] {});
  if (hist) for (int h = 0; h < 4; h++) for (int v = 0; v < 64; v++) hist[h * 64 + v] = kj_seg_hist[h][v];
  return ov ? -1 : n;
}

}  // extern "C"
