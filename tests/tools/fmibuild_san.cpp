// fmibuild_san.cpp — the stages behind the suffix sort as a program of its own for the sanitizers: the host emulation of the
// kernels (tests/emu/fmibuild_emu.cpp over kaiju_amd/csrc/kj_fmibuild.h) and the host stages (kaiju_fmi_arrays_host of
// kaiju_amd/csrc/mkfmi.cpp) on texts at the edges of blocks and pieces; the two must agree.
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan tests/tools/fmibuild_san.cpp tests/emu/fmibuild_emu.cpp kaiju_amd/csrc/mkfmi.cpp -lpthread -o fmibuild_san
//   fmibuild_san
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../kaiju_amd/csrc/mkfmi.h"

extern "C" uint32_t fmibuild_emu(const uint8_t *text, uint64_t tlen, const uint32_t *sa, uint64_t copies, int chpt_exp, const int *startLcode, int recode,
                                 uint32_t *read_of_rank, uint8_t *samples, uint8_t *bwt_out, uint32_t *piece_counts, uint16_t *index2_rows);

namespace {

std::vector<uint8_t> iid(uint64_t n, uint32_t seed, uint32_t term_every) {
  std::vector<uint8_t> t(n);
  uint32_t x = seed * 2654435761u + 12345u;
  for (uint64_t p = 0; p < n; p++) {
    x = x * 1664525u + 1013904223u;
    t[p] = (x >> 8) % term_every == 0 ? 0 : (uint8_t)(1 + (x >> 16) % 20);
  }
  t[n - 1] = 0;
  return t;
}

// positions of the letters by (symbols up to and including the terminator, position)
std::vector<uint32_t> naive_sa(const std::vector<uint8_t> &t) {
  std::vector<uint32_t> sa;
  for (uint32_t p = 0; p < t.size(); p++) if (t[p]) sa.push_back(p);
  std::sort(sa.begin(), sa.end(), [&](uint32_t a, uint32_t b) {
    for (uint32_t i = 0;; i++) {
      const uint8_t x = t[a + i], y = t[b + i];
      if (x != y) return x < y;
      if (!x) return a < b;
    }
  });
  return sa;
}

int run(const char *name, const std::vector<uint8_t> &t, uint64_t copies, int e, int recode) {
  kaiju_fmi_arrays a;
  memset(&a, 0, sizeof a);
  if (kaiju_fmi_arrays_sizes(t.data(), t.size(), copies, e, &a) != 0) { printf("%s: sizes: %s\n", name, kaiju_build_fmi_error()); return 1; }
  std::vector<uint32_t> ror(a.nseq), e_ror(a.nseq);
  std::vector<uint8_t> smp(a.n_samples_bytes), e_smp(a.n_samples_bytes), bwt(a.bwtlen), e_bwt(a.bwtlen);
  std::vector<int64_t> i1(a.n_index1);
  std::vector<uint16_t> i2(a.n_index2);
  a.read_of_rank = ror.data(); a.samples = smp.data(); a.bwt = bwt.data(); a.index1 = i1.data(); a.index2 = i2.data();
  if (kaiju_fmi_arrays_host(t.data(), t.size(), copies, e, 2, recode, &a) != 0) { printf("%s: host: %s\n", name, kaiju_build_fmi_error()); return 1; }
  const uint64_t nblk = (a.bwtlen + 255) >> 8, npieces = (a.bwtlen + 65535) >> 16;
  std::vector<uint32_t> pc(npieces * 21);
  std::vector<uint16_t> rows(nblk * 21);
  const std::vector<uint32_t> sa = naive_sa(t);
  const uint32_t bad = fmibuild_emu(t.data(), t.size(), sa.data(), copies, e, a.startLcode, recode, e_ror.data(), e_smp.data(), e_bwt.data(), pc.data(), rows.data());
  int wrong = bad != 0;
  wrong |= ror != e_ror ? 2 : 0;
  wrong |= smp != e_smp ? 4 : 0;
  wrong |= bwt != e_bwt ? 8 : 0;
  const uint64_t keep = std::min<uint64_t>(nblk, (uint64_t)a.N2 - 1);
  wrong |= memcmp(rows.data(), i2.data(), keep * 21 * 2) != 0 ? 16 : 0;
  uint64_t sum = 0;
  for (uint32_t c : pc) sum += c;
  wrong |= sum != a.bwtlen ? 32 : 0;
  if (wrong) printf("%s copies %lu e %d recode %d: emulation and host stages differ (%d, violations %#x)\n", name, (unsigned long)copies, e, recode, wrong, bad);
  return wrong != 0;
}

}  // namespace

int main() {
  struct Case { std::string name; std::vector<uint8_t> t; };
  std::vector<Case> cases;
  cases.push_back({"len_1", std::vector<uint8_t>(1, 0)});
  cases.push_back({"terminators_only", std::vector<uint8_t>(37, 0)});
  cases.push_back({"one_letter_75", [] { std::vector<uint8_t> t(76, 20); t[75] = 0; return t; }()});
  cases.push_back({"identical_40x300", [] { std::vector<uint8_t> t; for (int s = 0; s < 40; s++) { t.insert(t.end(), 300, 1); t.push_back(0); } return t; }()});
  cases.push_back({"empties", {1, 0, 2, 0, 1, 0, 20, 0, 1, 0, 0, 2, 0, 20, 0, 20, 0}});
  for (uint64_t n : {2, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097}) cases.push_back({"iid_" + std::to_string(n), iid(n, (uint32_t)n, 40)});
  cases.push_back({"iid_65537", iid(65537, 7, 40)});
  int failed = 0, runs = 0;
  for (const Case &c : cases) {
    const bool edge = c.name == "iid_4095" || c.name == "iid_4096" || c.name == "iid_4097";
    for (uint64_t copies : {1, 3, 7, 16, 17}) {
      if (copies > 7 && !edge) continue;
      if (copies > 1 && c.t.size() > 5000) continue;
      for (int e : {0, 2, 3, 5}) {
        if ((e == 2 || e == 5) && copies > 7) continue;
        for (int recode = 0; recode < 2; recode++) { failed += run(c.name.c_str(), c.t, copies, e, recode); runs++; }
      }
    }
  }
  printf("fmibuild_san: %d runs, %s\n", runs, failed ? "FAILED" : "ok");
  return failed ? 1 : 0;
}
