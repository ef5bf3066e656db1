// sufsort_wide_san.cpp — the wide suffix sort's host emulation (tests/emu/sufsort_wide_emu.cpp over the wide functions of
// kaiju_amd/csrc/kj_sufsort.h) as a program of its own for the sanitizers, on three texts of tests/sufsort_inputs.py -
// family_30x900, term_inside_key, ends_at_tlen_17 - with rank_bias 0 and 2^32 + 12345, against the naive order.
//   g++ -std=c++17 -fsanitize=address,undefined -static-libasan -static-libubsan tests/tools/sufsort_wide_san.cpp tests/emu/sufsort_wide_emu.cpp -o sufsort_wide_san
//   sufsort_wide_san
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

extern "C" uint32_t sufsort_wide_emu(const uint8_t *text, uint64_t tlen, uint64_t rank_bias, uint64_t *sa_out, uint64_t *n_out, uint32_t *rounds_out,
                                     uint64_t *active_out);

namespace {

std::vector<uint8_t> encode(const std::vector<std::string> &seqs) {
  const std::string alphabet = "*ACDEFGHIKLMNPQRSTVWY";
  std::vector<uint8_t> t;
  for (const std::string &s : seqs) {
    for (char c : s) t.push_back((uint8_t)alphabet.find(c));
    t.push_back(0);
  }
  return t;
}

// 30 sequences of 900 letters that differ from one another in a letter or two (the texts of the Python tests come from numpy's
// generator; the shape is what counts here)
std::vector<uint8_t> family() {
  uint32_t x = 77u * 2654435761u + 12345u;
  auto next = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
  std::vector<uint8_t> base(900);
  for (uint8_t &b : base) b = (uint8_t)(1 + next() % 20);
  std::vector<uint8_t> t;
  for (int i = 0; i < 30; i++) {
    std::vector<uint8_t> s = base;
    const uint32_t at = next() % 900;
    s[at] = (uint8_t)(s[at] % 20 + 1);
    t.insert(t.end(), s.begin(), s.end());
    t.push_back(0);
  }
  return t;
}

// positions of the letters by (symbols up to and including the terminator, position)
std::vector<uint64_t> naive_sa(const std::vector<uint8_t> &t) {
  std::vector<uint64_t> sa;
  for (uint64_t p = 0; p < t.size(); p++) if (t[p]) sa.push_back(p);
  std::sort(sa.begin(), sa.end(), [&](uint64_t a, uint64_t b) {
    for (uint64_t i = 0;; i++) {
      const uint8_t x = t[a + i], y = t[b + i];
      if (x != y) return x < y;
      if (!x) return a < b;
    }
  });
  return sa;
}

int run(const char *name, const std::vector<uint8_t> &t, uint64_t bias) {
  const std::vector<uint64_t> want = naive_sa(t);
  std::vector<uint64_t> sa(std::max<size_t>(1, want.size()), ~0ull);
  uint64_t n = 0, active[64];
  uint32_t rounds = 0;
  const uint32_t bad = sufsort_wide_emu(t.data(), t.size(), bias, sa.data(), &n, &rounds, active);
  sa.resize((size_t)n);
  const bool wrong = bad != 0 || sa != want;
  printf("%s bias %llu: %llu suffixes, %u rounds, violations %#x%s\n", name, (unsigned long long)bias, (unsigned long long)n, rounds, bad, wrong ? " WRONG" : "");
  return wrong ? 1 : 0;
}

}  // namespace

int main() {
  struct Case { const char *name; std::vector<uint8_t> t; };
  const Case cases[] = {
      {"family_30x900", family()},
      {"term_inside_key", encode({"ACDEFGHIKLM", "ACDEFGHIKLM", "ACDEFGHIKLMN", "ACDEFGHIKLMNA", "ACDEFGHIKLMN"})},
      {"ends_at_tlen_17", encode({"ACDEFGHIKLMNPQRS"})},
  };
  int failed = 0, runs = 0;
  for (const Case &c : cases)
    for (uint64_t bias : {0ull, (1ull << 32) + 12345ull}) { failed += run(c.name, c.t, bias); runs++; }
  printf("sufsort_wide_san: %d runs, %s\n", runs, failed ? "FAILED" : "ok");
  return failed ? 1 : 0;
}
