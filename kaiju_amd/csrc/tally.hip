// tally.hip — kaiju2table's reading of texts of output lines (gfx950, wave64): the passes of kj_tally.h as kernels, and the
// entry points kaiju_gpu_tally_* of include/kaiju_gpu.h.  As in annotate.hip the host never learns a count while the passes
// of an add call are queued: every kernel behind the first sizes itself from counts in device memory.
//
// per tree    k_tl_virus          virus[] (one lane per slot)
// per add     k_tl_init           the counters of the call
//             k_tl_lines_count    '\n' per tile                          k_tl_top   prefix sum over the tiles, one block
//             k_tl_lines_fill     line_start[]                                                          (kj_ingest.h: lines)
//             k_tl_plan           by one lane: the lines to count (without `final`: those a '\n' ends), the bytes used
//             k_tl_count          one lane per line: the kind and the slot; the five counts, direct[]  (k_tl_count_table)
//             k_tl_finish         kaiju_gpu_tally_info of the call, the call's counts added to the totals; by one lane
// at result   k_tl_sum            one lane per slot with direct > 0 walks up: summed[]
//             kjl::k_scan_sums / k_scan_top / k_scan_apply <TlSlots>   pos[] = prefix sum of (summed > 0)  (kj_lines.h)
//             k_tl_compact        the entries, dense, in slot order
//
// The count pass is a histogram over skewed keys - in a real sample a handful of taxa hold most of the reads -, and adds
// to one address of global memory go one behind the other.  So a block counts in a table of its own in LDS (kj_tally.h:
// table_place; a lane that finds no room there adds to direct[] for itself) and adds the table to direct[] at its end: a hot
// taxon costs one add to global memory per block.  The five counts are reduced per wavefront.  Every counter in global
// memory is 64 bit, every add to it an atomicAdd on unsigned long long.  Two other ways were built for the measurement in
// DESIGN.md 3.15 and stay selectable when a tally is created, so that the table there can be made again:
// KAIJU_GPU_TALLY_COUNT=lane adds lane by lane (the baseline), =wave groups equal slots inside a wavefront by ballot - the
// first open lane's slot, the lanes that hold it, their leader adds their number - for up to kGroupRounds slots and adds
// lane by lane for the rest.
//
// Every loop is bounded by the data: the hash probe of kjn::find_slot ends at an empty slot (the table is at least half
// empty), the walks of kjt::is_virus / sum_walk end because the loader refuses cycles, the probes of a block's table and
// the grouping rounds are counted, everything else runs over bytes, lines or slots.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "kj_tally.h"
#include "kj_krona.h"
#include "kj_lines.h"

using namespace kjt;
using kjs::OpAdd32;
using kjs::block_scan_excl;

typedef unsigned long long tl_u64;     // what atomicAdd takes
static_assert(sizeof(tl_u64) == sizeof(uint64_t), "64-bit counters");

struct kaiju_gpu_tally {
  const kaiju_gpu_taxon_names *names = nullptr;
  int device = -1;
  uint32_t cap = 0;                            // slots of the tree
  // what lasts from reset to reset, in allocations of its own: no call's scratch ever lies here
  uint64_t *direct = nullptr;                  // [cap]
  uint64_t *totals = nullptr;                  // used, n_lines, the five counts
  uint8_t *virus = nullptr;                    // [cap], per tree
  kjl::Scratch scratch;                        // of an add call: line tables, the call's counters
  kjl::Scratch res;                            // of a result call: summed[], flags, positions
  kjl::Scratch ent;                            // ... and the entries
  kjl::Scratch text, info;                     // device staging of the host form
  void *h_info = nullptr;                      // pinned: an info, or the totals and the number of entries
  void *h_text = nullptr, *h_ent = nullptr;    // pinned staging, grown on demand
  size_t h_text_cap = 0, h_ent_cap = 0;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;                   // behind the last call, on whichever stream it ran
  int count_by = 0;                            // KAIJU_GPU_TALLY_COUNT: kByTable (default), kByLane, kByWave
  bool timed = false;                          // KAIJU_GPU_TALLY_TIMES=1: events between the passes (kaiju_gpu_tally_pass_ms)
  hipEvent_t ev[KAIJU_GPU_TALLY_PASSES + 1] = {};
};

namespace {

constexpr int kTlBlock = 256;
static_assert(kTlBlock == (int)kji::kTileLanes && kTlBlock == kjs::kScanLanes, "one lane per chunk of a tile / element of a scan block");
constexpr int kGroupRounds = 4;        // different slots a wavefront adds through a leader
constexpr int kTotals = 2 + kCounts;   // used, n_lines, the counts
enum { kByTable = 0, kByLane = 1, kByWave = 2 };

struct TlHdr { uint64_t used; uint32_t n_lines, pad; uint64_t count[kCounts]; };

struct TlJob {
  const uint8_t *text;
  uint64_t bytes;
  uint32_t n_tiles;
  uint32_t *tile_cnt, *tile_base;      // n_tiles + 1
  uint32_t *line_start;                // bytes + 2
  TlHdr *hdr;
  kaiju_gpu_tally_info *info;
  const uint64_t *key;
  uint32_t cap_mask;
  const uint8_t *virus;
  uint64_t *direct, *totals;
  int final;
};

struct TlRes {
  const uint64_t *key;
  const uint32_t *parent;
  const uint8_t *virus;
  const uint64_t *direct;
  uint32_t cap;
  uint64_t *summed;                    // cap
  uint32_t *flag;                      // cap
  uint64_t *pos;                       // cap + 1
  uint64_t *blk, *blk_base;
};

struct TlSlots { uint64_t cap; __device__ uint64_t operator()() const { return cap; } };   // elements of the scan

__global__ __launch_bounds__(kTlBlock) void k_tl_virus(const uint64_t *key, const uint32_t *parent, uint32_t cap, uint8_t *virus) {
  const uint32_t vslot = kjn::find_slot(key, cap - 1, kVirusTaxon);
  for (uint32_t s = blockIdx.x * kTlBlock + threadIdx.x; s < cap; s += gridDim.x * kTlBlock)
    virus[s] = key[s] != ~0ull && is_virus(parent, vslot, s) ? 1 : 0;
}

__global__ void k_tl_init(TlHdr *h) {
  if (blockIdx.x || threadIdx.x) return;
  TlHdr z{};
  *h = z;
}

__global__ __launch_bounds__(kTlBlock) void k_tl_lines_count(TlJob J) {
  const uint64_t c = (uint64_t)blockIdx.x * kji::kTileLanes + threadIdx.x;
  uint32_t tot;
  block_scan_excl<uint32_t>(kji::popc16(kji::nl_mask(J.text, J.bytes, c)), 0u, &tot, OpAdd32());
  if (threadIdx.x == 0) J.tile_cnt[blockIdx.x] = tot;
}

// out[i] = in[0] + .. + in[i - 1] for i <= n, by one block
__global__ __launch_bounds__(kTlBlock) void k_tl_top(const uint32_t *in, uint32_t *out, uint32_t n) {
  uint32_t carry = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kTlBlock) {
    const uint32_t i = i0 + threadIdx.x;
    uint32_t tot;
    const uint32_t ex = block_scan_excl<uint32_t>(i < n ? in[i] : 0u, 0u, &tot, OpAdd32());
    if (i < n) out[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) out[n] = carry;
}

// line_start[0] and the sentinel behind the last line are k_tl_plan's
__global__ __launch_bounds__(kTlBlock) void k_tl_lines_fill(TlJob J) {
  const uint64_t c = (uint64_t)blockIdx.x * kji::kTileLanes + threadIdx.x;
  const uint32_t m = kji::nl_mask(J.text, J.bytes, c);
  uint32_t tot;
  const uint32_t ex = block_scan_excl<uint32_t>(kji::popc16(m), 0u, &tot, OpAdd32());
  uint32_t j = J.tile_base[blockIdx.x] + ex;                       // the line that ends at the next '\n'
  for (uint32_t mm = m; mm; mm &= mm - 1, j++) J.line_start[j + 1] = (uint32_t)(c * kji::kChunk + kji::ctz16(mm) + 1);
}

__global__ void k_tl_plan(TlJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t n_nl = J.tile_base[J.n_tiles];
  J.line_start[0] = 0;
  uint32_t sentinel;
  uint64_t used;
  const uint32_t n = lines_counted(J.text, J.bytes, n_nl, J.line_start[n_nl], J.final, &sentinel, &used);
  J.line_start[n] = sentinel;                                      // (a text that ends in '\n': the value the last '\n' gave too)
  J.hdr->n_lines = n;
  J.hdr->used = used;
}

// a line of `kind` (and, for a hit, whether its node is viral) in a lane's five counts
__device__ __forceinline__ void note_line(uint32_t *cnt, uint32_t kind, uint32_t virus) {
  cnt[kCntTotal] += kind != kLineEmpty ? 1u : 0u;
  cnt[kCntUnclassified] += kind == kLineUnclassified ? 1u : 0u;
  cnt[kCntBadId] += kind == kLineBadId ? 1u : 0u;
  cnt[kCntUnknown] += kind == kLineUnknown ? 1u : 0u;
  cnt[kCntVirus] += virus;
}
// the five counts of a lane's lines, reduced over the wavefront: one atomic per wavefront and counter
__device__ __forceinline__ void add_counts(const uint32_t *cnt, uint64_t *count) {
#pragma unroll
  for (int w = 0; w < kCounts; w++) {
    uint32_t v = cnt[w];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(reinterpret_cast<tl_u64 *>(&count[w]), (tl_u64)v);
  }
}

template <bool BY_LANE>
__global__ __launch_bounds__(kTlBlock) void k_tl_count(TlJob J) {
  const uint32_t n = J.hdr->n_lines;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t cnt[kCounts];
#pragma unroll
  for (int w = 0; w < kCounts; w++) cnt[w] = 0;
  // every lane of a wavefront makes the same number of rounds: the ballots below want all of them
  for (uint32_t r0 = blockIdx.x * kTlBlock; r0 < n; r0 += gridDim.x * kTlBlock) {
    const uint32_t r = r0 + threadIdx.x;
    uint32_t slot = kNone, kind = kLineEmpty;
    if (r < n) kind = line_kind(J.text, J.line_start[r], kji::line_len(J.line_start, r), J.key, J.cap_mask, &slot);
    note_line(cnt, kind, slot != kNone ? J.virus[slot] : 0u);
    if (!BY_LANE) {
      for (int round = 0; round < kGroupRounds; round++) {
        const tl_u64 open = __ballot(slot != kNone);
        if (!open) break;
        const uint32_t first = (uint32_t)__ffsll((long long)open) - 1u;
        const uint32_t s = (uint32_t)__shfl((int)slot, (int)first, 64);
        const tl_u64 same = __ballot(slot == s);
        if (lane == first) atomicAdd(reinterpret_cast<tl_u64 *>(&J.direct[s]), (tl_u64)__popcll(same));
        if (slot == s) slot = kNone;
      }
    }
    if (slot != kNone) atomicAdd(reinterpret_cast<tl_u64 *>(&J.direct[slot]), (tl_u64)1);
  }
  add_counts(cnt, J.hdr->count);
}

__global__ __launch_bounds__(kTlBlock) void k_tl_count_table(TlJob J) {
  __shared__ uint32_t s_key[kTableSlots], s_cnt[kTableSlots];          // 16 KiB
  for (uint32_t i = threadIdx.x; i < kTableSlots; i += kTlBlock) { s_key[i] = kNone; s_cnt[i] = 0; }
  __syncthreads();
  const uint32_t n = J.hdr->n_lines;
  uint32_t cnt[kCounts];
#pragma unroll
  for (int w = 0; w < kCounts; w++) cnt[w] = 0;
  for (uint32_t r = blockIdx.x * kTlBlock + threadIdx.x; r < n; r += gridDim.x * kTlBlock) {
    uint32_t slot;
    const uint32_t kind = line_kind(J.text, J.line_start[r], kji::line_len(J.line_start, r), J.key, J.cap_mask, &slot);
    note_line(cnt, kind, slot != kNone ? J.virus[slot] : 0u);
    if (slot == kNone) continue;
    const uint32_t i = table_place(slot, [&](uint32_t at, uint32_t v) { return atomicCAS(&s_key[at], kNone, v); });
    if (i != kNone) atomicAdd(&s_cnt[i], 1u);
    else atomicAdd(reinterpret_cast<tl_u64 *>(&J.direct[slot]), (tl_u64)1);
  }
  __syncthreads();
  // (a text has fewer than 2^32 lines: the 32-bit counts of the table cannot wrap)
  for (uint32_t i = threadIdx.x; i < kTableSlots; i += kTlBlock)
    if (s_cnt[i]) atomicAdd(reinterpret_cast<tl_u64 *>(&J.direct[s_key[i]]), (tl_u64)s_cnt[i]);
  add_counts(cnt, J.hdr->count);
}

__global__ void k_tl_finish(TlJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const TlHdr &H = *J.hdr;
  *J.info = make_info(H.used, H.n_lines, H.count);
  J.totals[0] += H.used;
  J.totals[1] += H.n_lines;
  for (int w = 0; w < kCounts; w++) J.totals[2 + w] += H.count[w];
}

__global__ __launch_bounds__(kTlBlock) void k_tl_sum(TlRes R) {
  for (uint32_t s = blockIdx.x * kTlBlock + threadIdx.x; s < R.cap; s += gridDim.x * kTlBlock) {
    const uint64_t d = R.direct[s];
    if (d) sum_walk(R.parent, R.virus, s, d, [&](uint32_t a, uint64_t v) { atomicAdd(reinterpret_cast<tl_u64 *>(&R.summed[a]), (tl_u64)v); });
  }
}

__global__ __launch_bounds__(kTlBlock) void k_tl_flag(TlRes R) {
  for (uint32_t s = blockIdx.x * kTlBlock + threadIdx.x; s < R.cap; s += gridDim.x * kTlBlock) R.flag[s] = R.summed[s] ? 1u : 0u;
}

// n_ent: room in ent[]
__global__ __launch_bounds__(kTlBlock) void k_tl_compact(TlRes R, kaiju_gpu_tally_entry *ent, uint64_t n_ent) {
  for (uint32_t s = blockIdx.x * kTlBlock + threadIdx.x; s < R.cap; s += gridDim.x * kTlBlock)
    if (R.flag[s] && R.pos[s] < n_ent) ent[R.pos[s]] = make_entry(R.key[s], R.direct[s], R.summed[s], R.virus[s]);
}

// ---- host side: scratch and the queue of passes ----------------------------------------------------------------------
void carve(kjl::Carver &c, TlJob &J, uint64_t bytes) {
  J.n_tiles = (uint32_t)((bytes + kji::kTileBytes - 1) / kji::kTileBytes);
  J.tile_cnt = c.take<uint32_t>((size_t)J.n_tiles + 1);
  J.tile_base = c.take<uint32_t>((size_t)J.n_tiles + 1);
  J.line_start = c.take<uint32_t>(bytes + 2);
  J.hdr = c.take<TlHdr>(1);
}

void carve(kjl::Carver &c, TlRes &R, uint32_t cap) {
  const size_t nblk = (size_t)cap / kjs::kScanLanes + 2;
  R.summed = c.take<uint64_t>(cap);
  R.flag = c.take<uint32_t>(cap);
  R.pos = c.take<uint64_t>((size_t)cap + 1);
  R.blk = c.take<uint64_t>(nblk);
  R.blk_base = c.take<uint64_t>(nblk + 1);
}

// p is device memory of a device other than `device` (what the runtime does not know is taken as it is)
bool on_other_device(const void *p, int device) {
  hipPointerAttribute_t at;
  if (!p) return false;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeDevice && at.device != device;
}

dim3 slot_grid(uint32_t cap) { return dim3((unsigned)std::min<uint64_t>(4096, (uint64_t)cap / kTlBlock + 1)); }

// the calls of a tally run one behind the other, on whichever streams they are queued
bool enter(kaiju_gpu_tally *a, hipStream_t s) { return hipStreamWaitEvent(s, a->done, 0) == hipSuccess; }
bool leave(kaiju_gpu_tally *a, hipStream_t s) { return hipEventRecord(a->done, s) == hipSuccess; }

int launch(kaiju_gpu_tally *a, hipStream_t s, const void *d_text, uint64_t bytes, int final, kaiju_gpu_tally_info *d_info) {
  if (!d_info || (!d_text && bytes)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (bytes > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
  if ((uintptr_t)d_text & (kji::kChunk - 1)) return fail(KAIJU_GPU_ERR_ARG, "the text must be 16-byte aligned");
  if (on_other_device(d_text, a->device) || on_other_device(d_info, a->device)) return fail(KAIJU_GPU_ERR_ARG, "the text or the info lives on another device than the taxon names");
  TlJob J{};
  kjl::Carver measure{nullptr};
  carve(measure, J, bytes);
  const char *err = "";
  if (int rc = a->scratch.reserve(measure.at, 256, "hipMalloc of the tally scratch", &err)) return fail(rc, err);
  kjl::Carver c{static_cast<uint8_t *>(a->scratch.p)};
  carve(c, J, bytes);
  const kjn::Tab &T = *kj_fn_tab(a->names);
  J.text = static_cast<const uint8_t *>(d_text); J.bytes = bytes; J.info = d_info; J.final = final ? 1 : 0;
  J.key = T.key; J.cap_mask = T.cap_mask; J.virus = a->virus; J.direct = a->direct; J.totals = a->totals;

  const dim3 blk(kTlBlock);
  // blocks for the other ways' pass over lines: how many there are is known on the device only
  const dim3 lgrid((unsigned)std::min<uint64_t>(4096, (bytes + 1) / kTlBlock + 1));
  int mark = 0;
  auto passed = [&]() { if (a->timed) (void)hipEventRecord(a->ev[mark++], s); };
  if (!enter(a, s)) return fail(KAIJU_GPU_ERR_HIP, "hipStreamWaitEvent of the tally");
  passed();
  hipLaunchKernelGGL(k_tl_init, dim3(1), dim3(64), 0, s, J.hdr);
  if (J.n_tiles) hipLaunchKernelGGL(k_tl_lines_count, dim3(J.n_tiles), blk, 0, s, J);
  hipLaunchKernelGGL(k_tl_top, dim3(1), blk, 0, s, J.tile_cnt, J.tile_base, J.n_tiles);
  if (J.n_tiles) hipLaunchKernelGGL(k_tl_lines_fill, dim3(J.n_tiles), blk, 0, s, J);
  hipLaunchKernelGGL(k_tl_plan, dim3(1), dim3(64), 0, s, J);
  passed();
  if (a->count_by == kByTable) hipLaunchKernelGGL(k_tl_count_table, dim3(count_blocks(bytes)), blk, 0, s, J);
  else if (a->count_by == kByLane) hipLaunchKernelGGL(k_tl_count<true>, lgrid, blk, 0, s, J);
  else hipLaunchKernelGGL(k_tl_count<false>, lgrid, blk, 0, s, J);
  passed();
  hipLaunchKernelGGL(k_tl_finish, dim3(1), dim3(64), 0, s, J);
  passed();
  if (hipGetLastError() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "a kernel of the tally passes could not be launched");
  if (!leave(a, s)) return fail(KAIJU_GPU_ERR_HIP, "hipEventRecord of the tally");
  return KAIJU_GPU_OK;
}

// pinned host memory of at least `bytes` bytes
int pinned(void **p, size_t *cap, size_t bytes) {
  if (bytes <= *cap) return KAIJU_GPU_OK;
  if (*p) { (void)hipHostFree(*p); *p = nullptr; *cap = 0; }
  const size_t want = bytes + bytes / 8 + 256;
  if (hipHostMalloc(p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return fail(KAIJU_GPU_ERR_NOMEM, "hipHostMalloc of the tally's staging"); }
  *cap = want;
  return KAIJU_GPU_OK;
}

int zero_counts(kaiju_gpu_tally *a) {
  const hipStream_t s = a->stream;
  if (!enter(a, s) || hipMemsetAsync(a->direct, 0, (size_t)a->cap * 8, s) != hipSuccess || hipMemsetAsync(a->totals, 0, kTotals * 8, s) != hipSuccess || !leave(a, s))
    return fail(KAIJU_GPU_ERR_HIP, "hipMemset of the tally's counts");
  return KAIJU_GPU_OK;
}

}  // namespace

extern "C" int kaiju_gpu_tally_create(const kaiju_gpu_taxon_names *names, kaiju_gpu_tally **out) {
  return guarded([&]() -> int {
    if (!names || !out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    *out = nullptr;
    kaiju_gpu_tally *a = new kaiju_gpu_tally();
    a->names = names;
    a->device = kj_fn_device(names);
    const kjn::Tab &T = *kj_fn_tab(names);
    a->cap = T.cap_mask + 1;
    if (hipSetDevice(a->device) != hipSuccess || hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&a->done, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(&a->h_info, sizeof(kaiju_gpu_tally_info) + 8, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&a->direct), (size_t)a->cap * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&a->totals), kTotals * 8) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&a->virus), a->cap) != hipSuccess) {
      (void)hipGetLastError();
      kaiju_gpu_tally_free(a);
      return fail(KAIJU_GPU_ERR_HIP, "hipStreamCreate / hipMalloc of the tally");
    }
    const char *e = getenv("KAIJU_GPU_TALLY_COUNT");
    a->count_by = e && !strcmp(e, "lane") ? kByLane : e && !strcmp(e, "wave") ? kByWave : kByTable;
    e = getenv("KAIJU_GPU_TALLY_TIMES");
    if (e && *e == '1') {
      for (hipEvent_t &ev : a->ev)
        if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); kaiju_gpu_tally_free(a); return fail(KAIJU_GPU_ERR_HIP, "hipEventCreate of the tally"); }
      a->timed = true;
    }
    if (hipEventRecord(a->done, a->stream) != hipSuccess) { kaiju_gpu_tally_free(a); return fail(KAIJU_GPU_ERR_HIP, "hipEventRecord of the tally"); }
    hipLaunchKernelGGL(k_tl_virus, slot_grid(a->cap), dim3(kTlBlock), 0, a->stream, T.key, T.parent, a->cap, a->virus);
    if (hipGetLastError() != hipSuccess) { kaiju_gpu_tally_free(a); return fail(KAIJU_GPU_ERR_HIP, "k_tl_virus could not be launched"); }
    if (int rc = zero_counts(a)) { kaiju_gpu_tally_free(a); return rc; }
    *out = a;
    return KAIJU_GPU_OK;
  });
}

extern "C" void kaiju_gpu_tally_free(kaiju_gpu_tally *a) {
  if (!a) return;
  if (a->device >= 0 && hipSetDevice(a->device) == hipSuccess) {
    if (a->done) { (void)hipEventSynchronize(a->done); (void)hipEventDestroy(a->done); }
    if (a->stream) { (void)hipStreamSynchronize(a->stream); (void)hipStreamDestroy(a->stream); }
    for (hipEvent_t ev : a->ev) if (ev) (void)hipEventDestroy(ev);
    if (a->h_info) (void)hipHostFree(a->h_info);
    if (a->h_text) (void)hipHostFree(a->h_text);
    if (a->h_ent) (void)hipHostFree(a->h_ent);
    if (a->direct) (void)hipFree(a->direct);
    if (a->totals) (void)hipFree(a->totals);
    if (a->virus) (void)hipFree(a->virus);
    a->scratch.release(); a->res.release(); a->ent.release(); a->text.release(); a->info.release();
  }
  delete a;
}

// for krona.hip, which reads the counts where they lie
kj_tally_view kj_tally_view_of(const kaiju_gpu_tally *a) { return kj_tally_view{a->names, a->device, a->direct, a->totals, a->done}; }

extern "C" int kaiju_gpu_tally_reset(kaiju_gpu_tally *a) {
  return guarded([&]() -> int {
    if (!a) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(a->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    return zero_counts(a);
  });
}

extern "C" int kaiju_gpu_tally_add_text_device(kaiju_gpu_tally *a, const void *d_text, uint64_t bytes, int final, kaiju_gpu_tally_info *d_info, void *stream) {
  return guarded([&]() -> int {
    if (!a) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(a->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    return launch(a, stream ? static_cast<hipStream_t>(stream) : a->stream, d_text, bytes, final, d_info);
  });
}

extern "C" int kaiju_gpu_tally_add_text(kaiju_gpu_tally *a, const char *text, uint64_t bytes, int final, kaiju_gpu_tally_info *info) {
  return guarded([&]() -> int {
    if (!a || !info || (!text && bytes)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (bytes > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
    if (hipSetDevice(a->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    const char *err = "";
    int rc;
    if ((rc = a->text.reserve(bytes + kji::kChunk, 256, "hipMalloc of the tally's text", &err))) return fail(rc, err);
    if ((rc = a->info.reserve(sizeof(kaiju_gpu_tally_info), 256, "hipMalloc of the tally's info", &err))) return fail(rc, err);
    if ((rc = pinned(&a->h_text, &a->h_text_cap, bytes))) return rc;
    const hipStream_t s = a->stream;
    if (bytes) memcpy(a->h_text, text, bytes);
    if (bytes && hipMemcpyAsync(a->text.p, a->h_text, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the text");
    kaiju_gpu_tally_info *d_info = static_cast<kaiju_gpu_tally_info *>(a->info.p);
    if ((rc = launch(a, s, a->text.p, bytes, final, d_info))) return rc;
    if (hipMemcpyAsync(a->h_info, d_info, sizeof *info, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, std::string("the tally passes: ") + hipGetErrorString(hipGetLastError()));
    memcpy(info, a->h_info, sizeof *info);
    return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_tally_result(kaiju_gpu_tally *a, kaiju_gpu_tally_entry *entries, uint64_t cap, uint64_t *n_entries, kaiju_gpu_tally_info *totals) {
  return guarded([&]() -> int {
    if (!a || !n_entries || !totals || (!entries && cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(a->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    TlRes R{};
    kjl::Carver measure{nullptr};
    carve(measure, R, a->cap);
    const char *err = "";
    if (int rc = a->res.reserve(measure.at, 256, "hipMalloc of the tally's sums", &err)) return fail(rc, err);
    kjl::Carver c{static_cast<uint8_t *>(a->res.p)};
    carve(c, R, a->cap);
    const kjn::Tab &T = *kj_fn_tab(a->names);
    R.key = T.key; R.parent = T.parent; R.virus = a->virus; R.direct = a->direct; R.cap = a->cap;
    static_assert(sizeof(kaiju_gpu_tally_info) == kTotals * 8, "the totals are an info");

    const hipStream_t s = a->stream;
    const dim3 blk(kTlBlock), grid = slot_grid(a->cap);
    if (!enter(a, s) || hipMemsetAsync(R.summed, 0, (size_t)a->cap * 8, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemset of the tally's sums");
    hipLaunchKernelGGL(k_tl_sum, grid, blk, 0, s, R);
    hipLaunchKernelGGL(k_tl_flag, grid, blk, 0, s, R);
    kjl::launch_offsets(s, dim3((unsigned)std::min<uint64_t>(2048, (uint64_t)a->cap / kjs::kScanLanes + 1)), TlSlots{a->cap}, R.flag, R.blk, R.blk_base, R.pos);
    if (hipGetLastError() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "a kernel of the tally's result could not be launched");
    uint8_t *h = static_cast<uint8_t *>(a->h_info);
    if (hipMemcpyAsync(h, a->totals, sizeof *totals, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(h + sizeof *totals, R.pos + a->cap, 8, hipMemcpyDeviceToHost, s) != hipSuccess || !leave(a, s) || hipStreamSynchronize(s) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, std::string("the tally's result: ") + hipGetErrorString(hipGetLastError()));
    memcpy(totals, h, sizeof *totals);
    uint64_t n;
    memcpy(&n, h + sizeof *totals, 8);
    *n_entries = n;
    if (n > a->cap) return fail(KAIJU_GPU_ERR_HIP, "the tally's result counted more nodes than the tree has");
    if (n > cap) return fail(KAIJU_GPU_ERR_ARG, "more nodes with reads than entries[] holds: " + std::to_string(n));
    if (!n) return KAIJU_GPU_OK;
    const size_t bytes = (size_t)n * sizeof(kaiju_gpu_tally_entry);
    if (int rc = a->ent.reserve(bytes, 256, "hipMalloc of the tally's entries", &err)) return fail(rc, err);
    if (int rc = pinned(&a->h_ent, &a->h_ent_cap, bytes)) return rc;
    if (!enter(a, s)) return fail(KAIJU_GPU_ERR_HIP, "hipStreamWaitEvent of the tally");
    hipLaunchKernelGGL(k_tl_compact, grid, blk, 0, s, R, static_cast<kaiju_gpu_tally_entry *>(a->ent.p), n);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(a->h_ent, a->ent.p, bytes, hipMemcpyDeviceToHost, s) != hipSuccess || !leave(a, s) ||
        hipStreamSynchronize(s) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, "the entries of the tally's result");
    memcpy(entries, a->h_ent, bytes);
    return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_tally_pass_ms(kaiju_gpu_tally *a, float *ms, uint32_t n) {
  return guarded([&]() -> int {
    if (!a || (!ms && n)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (!a->timed) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "the tally was created without KAIJU_GPU_TALLY_TIMES=1");
    if (hipSetDevice(a->device) != hipSuccess || hipEventSynchronize(a->ev[KAIJU_GPU_TALLY_PASSES]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventSynchronize");
    for (uint32_t k = 0; k < n && k < KAIJU_GPU_TALLY_PASSES; k++)
      if (hipEventElapsedTime(&ms[k], a->ev[k], a->ev[k + 1]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventElapsedTime");
    return KAIJU_GPU_OK;
  });
}
