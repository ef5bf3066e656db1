// kj_rowtax_plan.h — which row -> taxon table an index with 64-bit positions gets: one pure function from the size of the index,
// the free HBM and the two environment variables to {none | full | every 2^s-th row}.
//
// capi.hip's loader calls it where it used to test `bwtlen * 4 + 8 GB <= 70 % of the free HBM` inline; the CPU suite holds the
// table of decisions (tests/test_row_tax_sampled_emu.py).  Plain C++17: no HIP, no device types.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace kj {

constexpr uint64_t kRowTaxContextReserve = 8ull << 30;   // HBM left for the classification contexts (a constant: INTEGRATION.md)
constexpr uint32_t kRowTaxMaxShift = 3;

struct RowTaxPlan {
  enum Kind : uint32_t { None = 0, Full = 1, Sampled = 2 };
  Kind kind = None;
  uint32_t shift = 0;              // Sampled: 1 .. kRowTaxMaxShift and < chpt_exp; 0 otherwise
  uint64_t bytes = 0;              // of the table planned (what the text arrays behind it cannot have)
  bool shift_ignored = false;      // env_shift held a value outside 0 .. 3 or >= chpt_exp: the loader says so once
};

// bytes of the table for shift s (s = 0: the full one, DevIndex::row_tax; the slack: the many-rows locate reads 16 bytes at a time)
inline uint64_t row_tax_bytes(uint64_t bwtlen, uint32_t s) { return s == 0 ? bwtlen * 4 + 64 : ((bwtlen >> s) + 1) * 4 + 64; }

// env_row_tax / env_shift: the values of KAIJU_GPU_ROW_TAX / KAIJU_GPU_ROW_TAX_SHIFT, nullptr = not set.
//   KAIJU_GPU_ROW_TAX=0         none
//   KAIJU_GPU_ROW_TAX_SHIFT=s   s forced (0: the full table) - unless ROW_TAX=0
//   KAIJU_GPU_ROW_TAX=1         the full table (no shift given)
//   neither                     the smallest s in 0 .. min(3, chpt_exp - 1) whose table, the temporaries of the build
//                               (nseq * 20 + 64) and the contexts' reserve fit in 70 % of free_bytes; s = 0 is the test the
//                               loader has always made, so an index that got the full table keeps it
inline RowTaxPlan plan_row_tax(uint64_t bwtlen, uint32_t nseq, uint32_t chpt_exp, uint64_t free_bytes, const char *env_row_tax,
                               const char *env_shift) {
  RowTaxPlan r;
  auto pick = [&](uint32_t s) {
    r.kind = s == 0 ? RowTaxPlan::Full : RowTaxPlan::Sampled;
    r.shift = s;
    r.bytes = row_tax_bytes(bwtlen, s);
  };
  if (env_row_tax && atoi(env_row_tax) == 0) return r;
  if (env_shift) {
    char *end = nullptr;
    const long v = strtol(env_shift, &end, 10);
    if (end != env_shift && *end == 0 && v >= 0 && v <= (long)kRowTaxMaxShift && (v == 0 || (uint64_t)v < chpt_exp)) { pick((uint32_t)v); return r; }
    r.shift_ignored = true;
  }
  if (env_row_tax) { pick(0); return r; }
  const uint64_t tmp = (uint64_t)nseq * 20 + 64;
  const uint32_t s_max = chpt_exp == 0 ? 0u : (chpt_exp - 1 < kRowTaxMaxShift ? chpt_exp - 1 : kRowTaxMaxShift);
  for (uint32_t s = 0; s <= s_max; s++)
    if ((double)(row_tax_bytes(bwtlen, s) + tmp + kRowTaxContextReserve) <= 0.7 * (double)free_bytes) { pick(s); return r; }
  return r;
}

}  // namespace kj
