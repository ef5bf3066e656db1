// exact_pass.h — the exact pass (kj_core.h: BigSeg) as capi.hip launches it; kernels in exact_pass.hip.
//
// Its kernels live in a translation unit of their own on purpose: a second use of stage 1 (build_fragments) in the
// unit of the hot kernels changes how the compiler inlines and schedules k_fragments (seen in the device assembly,
// tests/tools/isa_dump.sh); apart, the kernels of the main pass stay exactly what was measured.
#pragma once
#include <hip/hip_runtime.h>

#include "kj_core.h"

// The counter buffer of a batch (4096 bytes, zeroed in front of every call up to kCntProf): its uint32 slots
enum CounterSlot : uint32_t {
  kCntMainWork = 0,        // work counter of the main search
  kCntRetryWork = 1,       // ... of the retry pass
  kCntRetryLen = 2,        // length of the retry list
  kCntErrFlags = 3,        // error flags: 1 a SegRec overflowed (settled by the exact pass), 2 SEG queue full, 4 region pool of
                           // the exact pass exhausted, 8 more reads than its list holds
  kCntSegQueue = 4,        // fragments in the SEG queue
  kCntExactReads = 5,      // the exact pass: listed reads,
  kCntExactFrags = 6,      // ... fragments of its queue,
  kCntExactWork = 7,       // ... its work counter,
  kCntLaneStats = 8,       // base of six uint64 of the lanes' loop statistics (KAIJU_GPU_PRINT_STATS)
  kCntExactPairs = 20,     // ... (left, right) pairs handed out of its pool
  kCntLazyList = 22,       // lazy SEG: listed reads,
  kCntLazyWork = 23,       // ... work counter of their second search
  kCntLocListMem = 24,     // reads whose matches hold many rows (k_mem_locate_list): MEM,
  kCntLocListGreedy = 25,  // ... Greedy
  kCntTodoList = 26,       // reads k_mem_post1 left to k_mem_post2
  kCntOvfWhy = 40,         // base of eight counts: Greedy reads sent to the retry pass, by reason (KAIJU_GPU_OVF_STATS)
  kCntOpTotals = kj::kOpcOffsetBytes / 4,   // base of the totals of the counting lanes (kOpcN uint64)
  kCntProf = 256           // base of the section profiles of -DKJ_PROF builds (byte 1024 .. 4096)
};

struct ExactPassLaunch {
  kj::DevIndex ix;
  const kj::ConstTables *d_ct;
  kj::SegTables st;
  kj::Params p;
  kj::Batch b;
  kj::SegQueue sq;            // queue and records of the main SEG pass
  uint32_t *cnt;              // counters of the batch (CounterSlot)
  uint32_t *bitmap, *list;    // one bit per read (zeroed); the listed reads
  uint32_t list_cap;
  kj::SegQueue sq2;           // queue of the exact pass (recs unused)
  kj::BigSeg big;
  int32_t *work; uint8_t *cls;    // SEG scratch: per block 4 * cap_ints ints and cls_bytes bytes
  uint32_t seg_blocks, cap_ints, cls_bytes;
  int n_cu;
  // search: scratch of the retry pass (the exact pass runs behind it on the same stream)
  int blocks_search;
  kj::SIEntry *si; uint32_t si_cap;                                                  // MEM
  kj::GItem *g_pool; uint16_t *g_ord; kj::GMatch *g_matches; kj::GBest *g_best; kj::GBestV *g_bestv;   // Greedy
  uint32_t g_pool_cap, g_match_cap;
  kj::VerboseOut vb;
  hipStream_t stream;
};

// collect the reads -> stage 1 -> SEG with lists of any length -> (MEM) split -> search; asynchronous on a.stream
hipError_t kj_launch_exact_pass(const ExactPassLaunch &a);
// step (3) of it alone - k_redo_seg over the queue a.sq2 into a.big (uses st, b, sq2, big, work, cls, seg_blocks, cap_ints,
// cls_bytes, cnt, stream): the diagnostic entry point kaiju_gpu_seg_regions
hipError_t kj_launch_redo_seg(const ExactPassLaunch &a);
