// locate_sampled_emu.cpp — TEST INFRASTRUCTURE ONLY.
//
// The locate of a wide index on the host (kaiju_amd/csrc/kj_core.h: mem_locate_read, mem_locate_read_team), over records that
// hold given suffix-array intervals as pending matches - what kaiju_gpu_locate_intervals does with the device's kernels:
//   0  mem_locate_read<true>                       the row -> taxon table of every row (k_mem_locate<true>)
//   1  mem_locate_read_team<true, 4>, TeamSerial   the walk to the suffix array's sample (k_mem_locate_wide)
//   2  mem_locate_read_team<true, 4, true>         the walk to the SAMPLED row -> taxon table (k_mem_locate_sampled)
//   3  mem_locate_read<true, true>                 the many-rows instantiation on the full table (k_mem_locate_list<true>)
// and the two pure host functions of the feature: plan_row_tax (kj_rowtax_plan.h) and the locate of plan_flow (kj_flow.h).
// tests/test_row_tax_sampled_emu.py builds it as a library; with -DLSE_MAIN it is a program of its own (the sanitizer build).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kaiju_gpu.h"
#include "../../kaiju_amd/csrc/host_index.h"
#include "../../kaiju_amd/csrc/kj_core.h"
#include "../../kaiju_amd/csrc/kj_flow.h"
#include "../../kaiju_amd/csrc/kj_rowtax_plan.h"

using namespace kj;

struct LseIndex {
  FmiFile file;
  PackedIndex packed;
};

extern "C" {

// environment: KAIJU_GPU_FORCE_WIDE (the tests: 16), KAIJU_EMU_ROW_TAX_SHIFT, KAIJU_EMU_NO_ROW_TAX
void *lse_load(const char *path, char *err, int errlen) {
  LseIndex *ix = new LseIndex();
  std::string msg;
  int rc = ix->file.load(path, msg);
  if (rc == 0) rc = ix->packed.build(ix->file.view(), msg);
  if (rc == 0 && !ix->packed.wide) { rc = -1; msg = "the sampled row -> taxon table is for wide indexes: set KAIJU_GPU_FORCE_WIDE"; }
  if (rc == 0) ix->packed.build_text_wide(1);
  if (rc != 0) { snprintf(err, (size_t)errlen, "%s", msg.c_str()); delete ix; return nullptr; }
  return ix;
}
void lse_free(void *h) { delete (LseIndex *)h; }
// out: [0] bwtlen, [1] rts_shift, [2] 1 = row_tax, [3] 1 = row_tax_s, [4] entries of that table (slack included), [5] n_dense
void lse_info(void *h, uint64_t *out) {
  const PackedIndex &pk = ((LseIndex *)h)->packed;
  const DevIndex d = pk.host_view();
  out[0] = d.bwtlen; out[1] = d.rts_shift; out[2] = d.row_tax != nullptr; out[3] = d.row_tax_s != nullptr;
  out[4] = pk.row_seq.size(); out[5] = d.n_dense;
}
const uint32_t *lse_table(void *h) { const DevIndex d = ((LseIndex *)h)->packed.host_view(); return d.row_tax ? d.row_tax : d.row_tax_s; }
const uint64_t *lse_tax_of_dense(void *h) { return ((LseIndex *)h)->packed.host_view().tax_of_dense; }

// records as kaiju_gpu_locate_intervals builds them; -> 0, -1 (bad argument), -2 (the index lacks the table `which` wants).
// steps (may be null; locators 1 and 2): the LF steps the walks of every record took
int lse_locate(void *h, int which, const uint64_t *lo, const uint32_t *len, const uint32_t *first, uint32_t n, uint32_t max_match_ids,
               kaiju_gpu_hit *out, uint64_t *steps) {
  DevIndex d = ((LseIndex *)h)->packed.host_view();
  if ((which == 0 || which == 3) && !d.row_tax) return -2;
  if (which == 2 && !d.row_tax_s) return -2;
  if (which == 1) { d.row_tax = nullptr; d.row_tax_s = nullptr; d.rts_shift = 0; }      // (the walk to sa_iseq, whatever the index holds)
  Params p{};
  p.mode = 0; p.m = 11; p.max_matches_SI = 20; p.max_match_ids = max_match_ids;
  static_assert(sizeof(Hit) == sizeof(kaiju_gpu_hit), "one record");
  for (uint32_t r = 0; r < n; r++) {
    const uint32_t k = first[r + 1] - first[r];
    if (first[r + 1] < first[r] || k > KAIJU_GPU_LOCATE_MAX_INTERVALS) return -1;
    Hit rec;
    memset(&rec, 0, sizeof rec);
    for (uint32_t q = 0; q < k; q++) {
      const uint64_t l0 = lo[first[r] + q], ln = len[first[r] + q];
      if (ln == 0 || l0 >= d.bwtlen || ln > d.bwtlen - l0 || ln >= kLocWideMaxLen) return -1;
      rec.taxid[q] = l0 | ln << kLocWideShift;
    }
    rec.n_ids = k; rec.flags = kHitLocPending;
    switch (which) {
      case 0: mem_locate_read<true>(d, p, &rec); break;
      case 1: { TeamSerial<4> tm; mem_locate_read_team<true, 4>(d, p, &rec, tm); if (steps) steps[r] = tm.lf_steps; break; }
      case 2: { TeamSerial<4> tm; mem_locate_read_team<true, 4, true>(d, p, &rec, tm); if (steps) steps[r] = tm.lf_steps; break; }
      case 3: mem_locate_read<true, true>(d, p, &rec); break;
      default: return -1;
    }
    memcpy(out + r, &rec, sizeof rec);
  }
  return 0;
}

// plan_row_tax; env_*: nullptr = not set.  out: [0] kind (0 none, 1 full, 2 sampled), [1] shift, [2] bytes, [3] shift_ignored
void lse_plan_row_tax(uint64_t bwtlen, uint32_t nseq, uint32_t chpt_exp, uint64_t free_bytes, const char *env_row_tax, const char *env_shift,
                      uint64_t *out) {
  const RowTaxPlan r = plan_row_tax(bwtlen, nseq, chpt_exp, free_bytes, env_row_tax, env_shift);
  out[0] = r.kind; out[1] = r.shift; out[2] = r.bytes; out[3] = r.shift_ignored;
}
// the loader's rule before plan_row_tax existed, written out again: the full table iff this holds
int lse_inline_rule(uint64_t bwtlen, uint32_t nseq, uint64_t free_bytes) {
  const uint64_t tmp = (uint64_t)nseq * 20 + 64, rt_est = bwtlen * 4 + 64;
  return (double)(rt_est + tmp + (8ull << 30)) <= 0.7 * (double)free_bytes ? 1 : 0;
}

// plan_flow's answer for a wide index as the device builds it (a six-letter k-mer table), 1000 reads of 150 nt.
// out: [0] locate, [1] fused, [2] lane, [3] mem_verbose
void lse_flow(int row_tax, int row_tax_sampled, int mode, int verbose, int records16, uint64_t *out) {
  FlowIndex ix{true, false, 0u, true, 6u, true, row_tax != 0};
  ix.row_tax_sampled = row_tax_sampled != 0;
  FlowSwitches sw;
  sw.p = Params{};
  sw.p.mode = mode; sw.p.m = 11; sw.p.seed_length = 7; sw.p.seg = 1; sw.p.max_matches_SI = 20; sw.p.max_match_ids = 20;
  sw.verbose = verbose != 0;
  sw.blocks_retry = mode ? 4 : 16;
  sw.greedy2 = flow_greedy2(ix, sw.p.seed_length);
  const FlowPlan f = plan_flow(ix, sw, FlowCall{1000u, false, 150u, 150000ull, records16 != 0});
  out[0] = (uint64_t)f.locate; out[1] = f.fused; out[2] = (uint64_t)f.lane; out[3] = f.mem_verbose;
}

}  // extern "C"

#ifdef LSE_MAIN
// locate_sampled_emu <fmi> <cases> <shift>: the cases (u32 n, u32 n_intervals, first[n + 1] u32, len[] u32, lo[] u64) through
// locators 0, 1, 3 on the full table and 1, 2 on the sampled one, max_match_ids 20 and 3; prints a digest of every run, which the
// test compares with the library's.  Exit status 0 unless something could not be loaded or run
static uint64_t digest(const std::vector<kaiju_gpu_hit> &v) {
  uint64_t h = 1469598103934665603ull;
  const uint8_t *b = reinterpret_cast<const uint8_t *>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(kaiju_gpu_hit); i++) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s <fmi> <cases> <shift>\n", argv[0]); return 2; }
  FILE *fp = fopen(argv[2], "rb");
  if (!fp) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  uint32_t head[2] = {0, 0};
  bool ok = fread(head, 4, 2, fp) == 2;
  std::vector<uint32_t> first((size_t)head[0] + 1), len(head[1]);
  std::vector<uint64_t> lo(head[1]);
  ok = ok && fread(first.data(), 4, first.size(), fp) == first.size() && fread(len.data(), 4, len.size(), fp) == len.size() &&
       fread(lo.data(), 8, lo.size(), fp) == lo.size();
  fclose(fp);
  if (!ok) { fprintf(stderr, "short read of %s\n", argv[2]); return 2; }
  setenv("KAIJU_GPU_FORCE_WIDE", "16", 1);
  char err[512];
  for (int pass = 0; pass < 2; pass++) {
    if (pass) setenv("KAIJU_EMU_ROW_TAX_SHIFT", argv[3], 1); else unsetenv("KAIJU_EMU_ROW_TAX_SHIFT");
    void *h = lse_load(argv[1], err, (int)sizeof err);
    if (!h) { fprintf(stderr, "%s\n", err); return 2; }
    uint64_t info[6];
    lse_info(h, info);
    for (int which = 0; which < 4; which++) {
      if (pass == 0 ? which == 2 : (which == 0 || which == 3)) continue;
      for (uint32_t cap : {20u, 3u}) {
        std::vector<kaiju_gpu_hit> out(head[0]);
        const int rc = lse_locate(h, which, lo.data(), len.data(), first.data(), head[0], cap, out.data(), nullptr);
        if (rc) { fprintf(stderr, "lse_locate(%d) = %d\n", which, rc); return 2; }
        printf("%u %d %u %016llx\n", (unsigned)info[1], which, cap, (unsigned long long)digest(out));
      }
    }
    lse_free(h);
  }
  return 0;
}
#endif
