// kj_flow.h — which kernels a classification call runs: one pure function from (index, switches, call) to a plan.
//
// capi.hip's launch_batch executes the plan on the device; tests/emu/kernel_emu.cpp's emu_classify takes the same plan for
// its sequential lanes, so the CPU suite hands the oracle the lane the product would run for those parameters.
// tests/test_flow_plan.py holds the table of flows.  Plain C++17: no HIP, no device types.
#pragma once
#include <algorithm>
#include <cstdint>

#include "kj_core.h"

namespace kj {

constexpr int kBlock = 256;        // threads per block of the search lanes
constexpr int kFragBlock = 64;     // ... of the one-lane-per-read stage 1 (k_fragments, k_fragments_protein)

// what the index offers
struct FlowIndex {
  bool blocks64;
  bool kline;  uint32_t kline_k;   // k-mer lines (narrow, second-generation lanes)
  bool kmer64; uint32_t kmer_k;    // k-mer table with 64-bit positions
  bool wide;                       // mb_base: 64-bit positions
  bool row_tax;                    // the row -> taxon table
  bool row_tax_sampled = false;    // ... of every 2^s-th row only (wide indexes, DevIndex::row_tax_s)
};
inline FlowIndex flow_index(const DevIndex &d) {
  return FlowIndex{d.blocks64 != nullptr, d.kline != nullptr, d.kline_k, d.kmer64 != nullptr, d.kmer_k, d.mb_base != nullptr,
                   d.row_tax != nullptr, d.row_tax_s != nullptr};
}

// the parameters and the switches of a context
struct FlowSwitches {
  Params p;
  bool verbose = false, verbose_v1 = false, mem_v1 = false, stage1_old = false, stage1_lane = false;
  bool lazy_seg = true, fused_post = true, exact_pass = true;
  bool greedy2 = false, greedy3 = false, count_ops = false;
  int blocks_retry = 16;           // blocks of the retry pass as the context has them (kaiju_gpu_create: 16 in MEM mode, 4 in Greedy, or
                                   // KAIJU_GPU_RETRY_BLOCKS); in MEM mode the plan halves them until the pass's scratch fits 1 GB
};

// the call
struct FlowCall {
  uint32_t n;
  bool paired;
  uint32_t max_read_len;           // as given: 0 = 1024; tripled for protein reads
  uint64_t seq_bytes;
  bool records16;                  // the 16-byte records (LCA on the device) are wanted too
};

// Greedy mode: the index and the seed length allow greedy_lane2 (a context asks this once, at creation)
inline bool flow_greedy2(const FlowIndex &ix, uint32_t seed_length) {
  const bool g_wide = ix.wide;
  const uint32_t g_k = g_wide ? ix.kmer_k : ix.kline_k;
  return ix.blocks64 && (g_wide ? ix.kmer64 : ix.kline) && g_k >= 2 && g_k <= seed_length && seed_length >= 3;
}

enum class FlowStatus : uint32_t { Ok, ProteinPaired, ProteinTooLong, TooManyFragSlots };
enum class FlowStage1 : uint32_t { Protein, Old, Fast, FastTrig, Long, LongTrig, Team };
enum class FlowSeg : uint32_t { Off, Eager, Lazy };
// (the first-generation lanes have one instantiation each, which also serves -v)
enum class FlowLane : uint32_t { MemV1, MemWideV1, Mem2, MemWide2, GreedyV1, Greedy2, Greedy2Wide, Greedy3 };
enum class FlowInst : uint32_t { Plain, Counting, XOrder, Verbose };
// who turns the matches the lanes found into ids
enum class FlowLocate : uint32_t { InLane, RowTax, RowTaxWide, Team, WideWalk, Fused, SampledWide };

struct FlowPlan {
  FlowStatus status = FlowStatus::Ok;
  bool run = false;                // n > 0: kernels are launched at all (the events of a call are recorded either way)
  FlowStage1 stage1 = FlowStage1::Old;
  FlowSeg seg = FlowSeg::Off;
  bool seg_apply = false;          // eager SEG in MEM mode: k_seg_apply behind k_seg
  FlowLane lane = FlowLane::MemV1;
  FlowInst inst = FlowInst::Plain;         // of the main search
  FlowInst inst_second = FlowInst::Plain;  // of the search of the lazily SEGged reads, unless ...
  bool mem_second = false;                 // ... k_mem_second runs it
  uint32_t flags_lane = 0, flags_second = 0;   // Params::flags added for those two searches (kParamDeferLocate, kParamLazySeg)
  bool fused = false;              // k_mem_post1 / _post2 finish the records
  bool trigcheck = false;          // lazy SEG without the fused pass: k_trigcheck lists the reads
  bool mem_verbose = false;        // k_mem_verbose writes columns 6 / 7 from the records
  FlowLocate locate = FlowLocate::InLane;
  bool exact_pass = false;
  bool lca = false;                // k_lca behind everything
  bool clear_out = false;          // d_out is zeroed in front of stage 1
  // sizes
  uint32_t max_read_len = 0;       // defaulted, tripled for protein reads
  uint64_t max_pair = 0, pep_bytes = 0, n_frag_slots = 0, seg_cap = 0, max_frag = 0;
  uint32_t si_cap_retry = 0, per_lane = 0;
  int blocks_retry = 0;
};

inline bool flow_lane_wide(FlowLane l) { return l == FlowLane::MemWideV1 || l == FlowLane::MemWide2 || l == FlowLane::Greedy2Wide; }

inline FlowPlan plan_flow(const FlowIndex &ix, const FlowSwitches &sw, const FlowCall &call) {
  FlowPlan f;
  const Params &p = sw.p;
  const uint32_t n = call.n;
  uint32_t max_read_len = call.max_read_len;
  if (max_read_len == 0) max_read_len = 1024;
  const bool protein = (p.flags & kParamProtein) != 0;
  if (protein) {
    // a protein read is its own (single) frame: fragments are up to max_read_len long, not a third of it
    if (call.paired) { f.status = FlowStatus::ProteinPaired; return f; }
    if (max_read_len > 0x10000000u) { f.status = FlowStatus::ProteinTooLong; return f; }
    max_read_len *= 3;
  }
  const uint64_t max_pair = (uint64_t)max_read_len * (call.paired ? 2 : 1);
  f.run = n > 0;
  f.max_read_len = max_read_len;
  f.max_pair = max_pair;
  f.pep_bytes = 2 * call.seq_bytes + kPepPerRead * n + 32 + 256;   // pep_base() + window over-read slack
  f.n_frag_slots = 2 * ((2 * call.seq_bytes) / (p.m + 1) + 7ull * n) + 8;
  if (f.n_frag_slots >= 0xffffffffull) { f.status = FlowStatus::TooManyFragSlots; return f; }
  // SEG work list: at most one entry per original fragment
  f.seg_cap = p.seg ? std::min<uint64_t>(f.n_frag_slots / 2 + 8, 0x00ffffffull) : 1;
  f.max_frag = protein ? max_read_len / 3 : max_read_len / 3 + 2;     // (max_read_len was tripled for protein reads)
  // every (fragment, end position) can yield at most one match
  f.si_cap_retry = (uint32_t)std::min<uint64_t>(2 * max_pair + 64, 1u << 24);
  f.blocks_retry = sw.blocks_retry;
  if (p.mode == 0)
    while (f.blocks_retry > 1 && (uint64_t)f.blocks_retry * kBlock * f.si_cap_retry * sizeof(SIEntry) > (1ull << 30)) f.blocks_retry /= 2;
  // LDS staging area per lane of the old stage 1: all frame strings of a read (or pair), rounded to 16 bytes
  f.per_lane = (uint32_t)((2 * max_pair + 12 + 15) & ~15ull);
  if ((uint64_t)f.per_lane * kFragBlock > 60000) f.per_lane = 0;        // long reads: write in place

  // which stage 1 / SEG flow: the fast stage 1 serves mates up to kS1MaxLenLong nucleotides (two instantiations); in MEM mode on
  // the second-generation lanes SEG is then looked at lazily (kj_core.h: kParamLazySeg), everywhere else stage 1 detects the
  // SEG trigger itself
  const bool mem_narrow2 = ix.blocks64 && ix.kline && ix.kline_k >= 2 && ix.kline_k <= p.m;
  const bool mem_wide2 = ix.blocks64 && ix.wide && ix.kmer64 && ix.kmer_k >= 2 && ix.kmer_k <= p.m;
  // kaiju -v in MEM mode: the VERBOSE instantiations of those lanes + k_mem_verbose - where a match's place in its read fits the
  // 16 + 16 bits of the lanes' notes (reads of 196 000 nt and more: the first-generation lanes, which also serve -v in Greedy
  // mode, the retry pass and the exact pass)
  const bool vb_v2 = sw.verbose && !sw.verbose_v1 && max_read_len / 3 + 4 < 65536 && 2 * max_pair / (p.m + 1) + 8 < 65536;
  const bool mem_v2 = p.mode == 0 && (mem_narrow2 || mem_wide2) && !sw.mem_v1 && (!sw.verbose || vb_v2);
  const bool fast1 = !protein && !sw.stage1_old && max_read_len <= kS1MaxLenLong && p.m >= 1 && p.m <= 64;
  const bool long1 = max_read_len > kS1MaxLen;              // (192 .. 287 nt: the instantiation with six units per frame string)
  const bool lazy = fast1 && mem_v2 && p.seg && sw.lazy_seg;
  const bool trig1 = fast1 && p.seg && !lazy;
  // the fused post-search pass (k_mem_post1 / _post2): narrow MEM lanes with the row -> taxon table, SEG lazily or not at all
  // (an eager SEG pass may send ANY read to the exact pass: nothing is final before that)
  f.fused = p.mode == 0 && mem_v2 && mem_narrow2 && ix.row_tax && (lazy || !p.seg) && sw.fused_post && n > 0 && !sw.verbose;
  // unused id slots read as 0.  Not with the 16-byte records as the output on the fused path: the lanes write the header of every
  // record and the entries they announce in it, k_mem_post1 / _post2 read nothing else - d_hits is scratch there (1.84 GB less to
  // write per 10 M reads)
  f.clear_out = n > 0 && !(f.fused && call.records16);
  if (protein) f.stage1 = FlowStage1::Protein;
  else if (fast1 && trig1 && long1) f.stage1 = FlowStage1::LongTrig;
  else if (fast1 && long1) f.stage1 = FlowStage1::Long;
  else if (fast1 && trig1) f.stage1 = FlowStage1::FastTrig;
  else if (fast1 && !sw.stage1_lane && !call.paired) f.stage1 = FlowStage1::Team;     // (pairs: the team kernel was slower)
  else if (fast1) f.stage1 = FlowStage1::Fast;
  else f.stage1 = FlowStage1::Old;
  f.seg = !p.seg ? FlowSeg::Off : lazy ? FlowSeg::Lazy : FlowSeg::Eager;
  f.seg_apply = f.seg == FlowSeg::Eager && p.mode == 0;
  f.trigcheck = lazy && !f.fused;
  // the exact pass (kj_core.h: BigSeg; kernels in exact_pass.hip): reads with a fragment whose SEG regions did not fit a SegRec
  // are classified again behind the retry pass, with region lists of any length
  f.exact_pass = n > 0 && p.seg && sw.exact_pass;
  f.lca = call.records16 && !f.fused && n > 0;

  bool defer;      // the second-generation lanes leave the best matches of every read in its hit record; k_mem_locate* behind the
                   // searches turn them into ids
  bool narrow;
  if (p.mode == 0) {
    const bool xo = (p.flags & kParamXOrder) != 0;
    defer = mem_v2;
    narrow = mem_narrow2;
    if (mem_v2) {
      // the second-generation lane that serves this index (narrow: below 2^32 rows; wide: 64-bit positions)
      f.lane = mem_narrow2 ? FlowLane::Mem2 : FlowLane::MemWide2;
      f.inst = sw.verbose ? FlowInst::Verbose : sw.count_ops ? FlowInst::Counting : xo ? FlowInst::XOrder : FlowInst::Plain;
      f.inst_second = sw.verbose ? FlowInst::Verbose : xo ? FlowInst::XOrder : FlowInst::Plain;
      f.mem_second = lazy && !sw.verbose && mem_narrow2 && !xo;
      f.flags_lane = f.flags_second = kParamDeferLocate;
      if (lazy) f.flags_lane |= kParamLazySeg;
    } else f.lane = !ix.wide ? FlowLane::MemV1 : FlowLane::MemWideV1;
  } else {
    // (-v: the VERBOSE instantiation of the second-generation lane unless verbose_v1 - fragment positions must fit the 16 bits
    //  of a GBestV's substitution positions, as in the lane itself)
    const bool vb_g2 = sw.verbose && !sw.verbose_v1 && max_read_len / 3 + 4 < 65536;
    const bool use_g2 = sw.greedy2 && (!sw.verbose || vb_g2);
    const bool use_g3 = use_g2 && sw.greedy3 && !sw.verbose;
    defer = use_g2;       // (greedy_lane2 leaves every read's best matches to k_mem_locate*)
    narrow = !ix.wide;
    if (use_g3) { f.lane = FlowLane::Greedy3; f.inst = sw.count_ops ? FlowInst::Counting : FlowInst::Plain; }
    else if (use_g2) {
      f.lane = ix.wide ? FlowLane::Greedy2Wide : FlowLane::Greedy2;
      f.inst = sw.verbose ? FlowInst::Verbose : sw.count_ops ? FlowInst::Counting : FlowInst::Plain;
    } else f.lane = FlowLane::GreedyV1;
    if (use_g2) f.flags_lane = kParamDeferLocate;
  }
  // columns 6 / 7 of the reads whose matches wait in their records (the retry pass writes its reads' own)
  f.mem_verbose = defer && sw.verbose;
  if (!defer) f.locate = FlowLocate::InLane;
  else if (f.fused) f.locate = FlowLocate::Fused;
  else if (narrow) f.locate = ix.row_tax ? FlowLocate::RowTax : FlowLocate::Team;
  else f.locate = ix.row_tax ? FlowLocate::RowTaxWide : ix.row_tax_sampled ? FlowLocate::SampledWide : FlowLocate::WideWalk;
  return f;
}

}  // namespace kj
