// merge.hip — kaiju-mergeOutputs on two texts of output lines (gfx950, wave64): the passes of kj_merge.h as kernels, and the
// entry points kaiju_gpu_merger_* / kaiju_gpu_merge_* of include/kaiju_gpu.h.  As in annotate.hip the host never learns a count
// while the passes are queued: every kernel behind the first sizes itself from counts in device memory.
//
//   k_mg_init           counters
//   k_mg_lines_count    '\n' per tile                          k_mg_top   prefix sum over the tiles, one block
//   k_mg_lines_fill     line_start[], the number of lines                (kj_ingest.h: lines; the three once per text)
//   k_mg_plan           by one lane: the pairs to look at, the bytes used, whether text 2 goes on
//   k_mg_pair           one lane per pair: rec[], atomicMin of the first pair that stops.  The walks in the tree are here
//   k_mg_count          the pairs in front of the stop: olen[], the counters.  (Which pairs those are is known only once every
//                       lane of k_mg_pair is through: this cannot sit in that pass)
//   kjl::k_scan_sums / k_scan_top / k_scan_apply <MgCount>   out_off[] = prefix sum of olen[] (kj_lines.h)
//   k_mg_write          per lane 16 aligned bytes of the output: kjl::write_blocks over merge_chunk
//   k_mg_finish         kaiju_gpu_merge_info, by one lane with ordinary stores
// With KAIJU_GPU_MERGE_TIMES=1 a merger records an event between the passes (kaiju_gpu_merge_pass_ms: tests/tools/merge_timing.py).
//
// Every loop is bounded by the data: the hash probe of kjm::find_slot ends at an empty slot (the table is at least half
// empty), the walks of kjm::mlca / anc count down the depth stored with the slot, everything else runs over bytes or lines.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "kj_merge.h"
#include "kj_lines.h"

using namespace kjm;
using kjs::OpAdd32;
using kjs::block_scan_excl;

struct kaiju_gpu_merger {
  int device = -1;
  int conflict = 0, use_score = 0;
  Tree tree{};
  kjl::Lines st;
  kjl::Scratch text1, text2, out, info;        // device staging of the host form
  void *h_info = nullptr;                      // pinned
  void *h_text1 = nullptr, *h_text2 = nullptr, *h_out = nullptr;   // pinned staging of the host form, grown on demand
  size_t h_text1_cap = 0, h_text2_cap = 0, h_out_cap = 0;
  hipStream_t stream = nullptr;
  bool timed = false;                          // KAIJU_GPU_MERGE_TIMES=1: events between the passes (kaiju_gpu_merge_pass_ms)
  hipEvent_t ev[KAIJU_GPU_MERGE_PASSES + 1] = {};
};

namespace {

constexpr int kMgBlock = 256;
static_assert(kMgBlock == (int)kji::kTileLanes && kMgBlock == (int)kjf::kBlockLanes && kMgBlock == kjs::kScanLanes,
              "one lane per chunk of a tile / of a block of output / element of a scan block");

struct MgHdr {
  uint64_t written, used1, used2;
  uint32_t n_lines[2];
  uint32_t n_look;                     // pairs k_mg_pair looks at
  uint32_t stop;                       // the first pair that stops (kNoStop: none)
  uint32_t n_out;                      // pairs written: min(n_look, stop)
  uint32_t more_in_2;
  uint32_t count[kKindCount];
};

struct MgText {
  const uint8_t *text;
  uint64_t bytes;
  uint32_t n_tiles;
  uint32_t *tile_cnt, *tile_base;      // n_tiles + 1
  uint32_t *line_start;                // bytes + 2
};

struct MgJob {
  MgText t[2];
  uint8_t *out;
  uint64_t out_cap;
  kaiju_gpu_merge_info *info;
  Rec *rec;                            // pair_cap
  uint64_t *olen, *out_off;            // pair_cap, pair_cap + 1
  uint64_t *oblk, *oblk_base;          // per block of kScanLanes pairs (+ 1)
  MgHdr *hdr;
  int final, conflict, use_score;
};

struct MgCount { const MgHdr *hdr; __device__ uint64_t operator()() const { return hdr->n_out; } };   // elements of the scan

__global__ void k_mg_init(MgHdr *h) {
  if (blockIdx.x || threadIdx.x) return;
  MgHdr z{};
  z.stop = kNoStop;
  *h = z;
}

__global__ __launch_bounds__(kMgBlock) void k_mg_lines_count(MgText X) {
  const uint64_t c = (uint64_t)blockIdx.x * kji::kTileLanes + threadIdx.x;
  uint32_t tot;
  block_scan_excl<uint32_t>(kji::popc16(kji::nl_mask(X.text, X.bytes, c)), 0u, &tot, OpAdd32());
  if (threadIdx.x == 0) X.tile_cnt[blockIdx.x] = tot;
}

// out[i] = in[0] + .. + in[i - 1] for i <= n, by one block
__global__ __launch_bounds__(kMgBlock) void k_mg_top(const uint32_t *in, uint32_t *out, uint32_t n) {
  uint32_t carry = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kMgBlock) {
    const uint32_t i = i0 + threadIdx.x;
    uint32_t tot;
    const uint32_t ex = block_scan_excl<uint32_t>(i < n ? in[i] : 0u, 0u, &tot, OpAdd32());
    if (i < n) out[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) out[n] = carry;
}

// line_start[0] and the sentinel behind the last line are k_mg_plan's
__global__ __launch_bounds__(kMgBlock) void k_mg_lines_fill(MgText X) {
  const uint64_t c = (uint64_t)blockIdx.x * kji::kTileLanes + threadIdx.x;
  const uint32_t m = kji::nl_mask(X.text, X.bytes, c);
  uint32_t tot;
  const uint32_t ex = block_scan_excl<uint32_t>(kji::popc16(m), 0u, &tot, OpAdd32());
  uint32_t j = X.tile_base[blockIdx.x] + ex;                       // the line that ends at the next '\n'
  for (uint32_t mm = m; mm; mm &= mm - 1, j++) X.line_start[j + 1] = (uint32_t)(c * kChunk + kji::ctz16(mm) + 1);
}

__global__ void k_mg_plan(MgJob J) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t n[2];
  for (int k = 0; k < 2; k++) {
    const MgText &X = J.t[k];
    const uint32_t n_nl = X.tile_base[X.n_tiles];
    X.line_start[0] = 0;
    uint32_t sentinel;
    n[k] = merge_line_count(X.text, X.bytes, n_nl, X.line_start[n_nl], J.final, &sentinel);
    X.line_start[n[k]] = sentinel;                                 // (a text that ends in '\n': the value the last '\n' gave too)
    J.hdr->n_lines[k] = n[k];
  }
  const uint32_t n_pairs = n[0] < n[1] ? n[0] : n[1];
  J.hdr->n_look = pairs_looked_at(n[0], n[1], J.final, J.t[0].bytes, J.t[1].bytes);
  J.hdr->used1 = J.final ? J.t[0].bytes : J.t[0].line_start[n_pairs];
  J.hdr->used2 = J.final ? J.t[1].bytes : J.t[1].line_start[n_pairs];
  J.hdr->more_in_2 = J.final && n[1] > n[0] && kji::line_len(J.t[1].line_start, n[0]) != 0 ? 1u : 0u;
}

__global__ __launch_bounds__(kMgBlock) void k_mg_pair(MgJob J, Tree T) {
  const uint32_t n = J.hdr->n_look, n2 = J.hdr->n_lines[1];
  uint32_t stop = kNoStop;
  for (uint32_t r = blockIdx.x * kMgBlock + threadIdx.x; r < n; r += gridDim.x * kMgBlock) {
    const uint32_t *l1 = J.t[0].line_start, *l2 = J.t[1].line_start;
    const bool have2 = r < n2;
    const uint64_t a2 = have2 ? l2[r] : 0, e2 = have2 ? (uint64_t)l2[r + 1] - 1 : 0;
    const Rec R = resolve_pair(J.t[0].text, l1[r], (uint64_t)l1[r + 1] - 1, J.t[1].text, a2, e2, have2, T, J.conflict, J.use_score);
    J.rec[r] = R;
    if (rec_why(R) && r < stop) stop = r;
  }
  if (stop != kNoStop) atomicMin(&J.hdr->stop, stop);
}

__global__ __launch_bounds__(kMgBlock) void k_mg_count(MgJob J) {
  const uint32_t look = J.hdr->n_look, stop = J.hdr->stop;
  const uint32_t n = look < stop ? look : stop;
  uint32_t cnt[kKindCount];
#pragma unroll
  for (int w = 0; w < kKindCount; w++) cnt[w] = 0;
  for (uint32_t r = blockIdx.x * kMgBlock + threadIdx.x; r < n; r += gridDim.x * kMgBlock) {
    const Rec R = J.rec[r];
    J.olen[r] = rec_olen(R);
#pragma unroll
    for (int w = 0; w < kKindCount; w++) cnt[w] += rec_kind(R) == (uint32_t)w ? 1u : 0u;
  }
#pragma unroll
  for (int w = 0; w < kKindCount; w++) {
    uint32_t v = cnt[w];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&J.hdr->count[w], v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) J.hdr->n_out = n;
}

__global__ __launch_bounds__(kMgBlock) void k_mg_write(MgJob J) {
  kjl::write_blocks(J.out_off, J.hdr->n_out, J.out, J.out_cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) {
    return merge_chunk(c, J.t[0].text, J.t[1].text, J.rec, J.out_off, lo, hi, total, J.out_cap, v);
  });
}

__global__ void k_mg_finish(MgJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const MgHdr &H = *J.hdr;
  const uint32_t n = H.n_out;
  const uint64_t total = J.out_off[n];
  // the lines that fit: out_off[0 .. k] with out_off[k] <= out_cap
  J.hdr->written = total <= J.out_cap ? total : J.out_off[kjf::find_record(J.out_off, 0, n + 1, J.out_cap)];
  const uint32_t why = H.stop != kNoStop ? rec_why(J.rec[H.stop]) : (uint32_t)kStopNone;
  *J.info = make_info(total, H.used1, H.used2, H.n_lines[0], H.n_lines[1], n, H.stop, why, H.count, H.more_in_2, J.out_cap);
}

// ---- host side: scratch and the queue of passes ----------------------------------------------------------------------
void carve(kjl::Carver &c, MgJob &J) {
  for (MgText &X : J.t) {
    X.n_tiles = (uint32_t)((X.bytes + kji::kTileBytes - 1) / kji::kTileBytes);
    X.tile_cnt = c.take<uint32_t>((size_t)X.n_tiles + 1);
    X.tile_base = c.take<uint32_t>((size_t)X.n_tiles + 1);
    X.line_start = c.take<uint32_t>(X.bytes + 2);
  }
  const size_t pairs = pair_cap(J.t[0].bytes, J.t[1].bytes), nblk = pairs / kjs::kScanLanes + 2;
  J.rec = c.take<Rec>(pairs);
  J.olen = c.take<uint64_t>(pairs);
  J.out_off = c.take<uint64_t>(pairs + 1);
  J.oblk = c.take<uint64_t>(nblk);
  J.oblk_base = c.take<uint64_t>(nblk + 1);
  J.hdr = c.take<MgHdr>(1);
}

// p is device memory of a device other than `device` (what the runtime does not know is taken as it is)
bool on_other_device(const void *p, int device) {
  hipPointerAttribute_t at;
  if (!p) return false;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeDevice && at.device != device;
}

int launch(kaiju_gpu_merger *a, hipStream_t s, const void *d_text1, uint64_t bytes1, const void *d_text2, uint64_t bytes2, int final, void *d_out,
           uint64_t out_cap, kaiju_gpu_merge_info *d_info) {
  if (!d_info || (!d_text1 && bytes1) || (!d_text2 && bytes2) || (!d_out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (bytes1 > kji::kMaxBytes || bytes2 > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
  if (((uintptr_t)d_text1 | (uintptr_t)d_text2 | (uintptr_t)d_out) & (kChunk - 1)) return fail(KAIJU_GPU_ERR_ARG, "the texts and the output pointer must be 16-byte aligned");
  if (on_other_device(d_text1, a->device) || on_other_device(d_text2, a->device) || on_other_device(d_out, a->device))
    return fail(KAIJU_GPU_ERR_ARG, "a text or the output lives on another device than the merger");
  MgJob J{};
  J.t[0].text = static_cast<const uint8_t *>(d_text1); J.t[0].bytes = bytes1;
  J.t[1].text = static_cast<const uint8_t *>(d_text2); J.t[1].bytes = bytes2;
  kjl::Carver measure{nullptr};
  carve(measure, J);
  const char *err = "";
  if (int rc = a->st.mem.reserve(measure.at, 256, "hipMalloc of the merge scratch", &err)) return fail(rc, err);
  kjl::Carver c{static_cast<uint8_t *>(a->st.mem.p)};
  carve(c, J);
  a->st.total = nullptr;
  a->st.written = &J.hdr->written;
  J.out = static_cast<uint8_t *>(d_out); J.out_cap = out_cap; J.info = d_info;
  J.final = final ? 1 : 0; J.conflict = a->conflict; J.use_score = a->use_score;

  const dim3 blk(kMgBlock);
  const uint64_t pairs = pair_cap(bytes1, bytes2);
  // blocks for the passes over pairs: how many there are is known on the device only
  const dim3 pgrid((unsigned)std::min<uint64_t>(4096, pairs / kMgBlock + 1));
  const dim3 ogrid((unsigned)std::min<uint64_t>(2048, pairs / kjs::kScanLanes + 1));
  const dim3 wgrid((unsigned)std::min<uint64_t>(8192, out_cap / kjf::kBlockBytes + 1));
  int mark = 0;
  auto passed = [&]() { if (a->timed) (void)hipEventRecord(a->ev[mark++], s); };
  passed();
  hipLaunchKernelGGL(k_mg_init, dim3(1), dim3(64), 0, s, J.hdr);
  for (const MgText &X : J.t) {
    if (X.n_tiles) hipLaunchKernelGGL(k_mg_lines_count, dim3(X.n_tiles), blk, 0, s, X);
    hipLaunchKernelGGL(k_mg_top, dim3(1), blk, 0, s, X.tile_cnt, X.tile_base, X.n_tiles);
    if (X.n_tiles) hipLaunchKernelGGL(k_mg_lines_fill, dim3(X.n_tiles), blk, 0, s, X);
  }
  hipLaunchKernelGGL(k_mg_plan, dim3(1), dim3(64), 0, s, J);
  passed();
  hipLaunchKernelGGL(k_mg_pair, pgrid, blk, 0, s, J, a->tree);
  passed();
  hipLaunchKernelGGL(k_mg_count, pgrid, blk, 0, s, J);
  passed();
  kjl::launch_offsets(s, ogrid, MgCount{J.hdr}, J.olen, J.oblk, J.oblk_base, J.out_off);
  passed();
  hipLaunchKernelGGL(k_mg_write, wgrid, blk, 0, s, J);
  passed();
  hipLaunchKernelGGL(k_mg_finish, dim3(1), dim3(64), 0, s, J);
  passed();
  if (hipGetLastError() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "a kernel of the merge passes could not be launched");
  return KAIJU_GPU_OK;
}

// pinned host memory of at least `bytes` bytes
int pinned(void **p, size_t *cap, size_t bytes) {
  if (bytes <= *cap) return KAIJU_GPU_OK;
  if (*p) { (void)hipHostFree(*p); *p = nullptr; *cap = 0; }
  const size_t want = bytes + bytes / 8 + 256;
  if (hipHostMalloc(p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return fail(KAIJU_GPU_ERR_NOMEM, "hipHostMalloc of the merger's staging"); }
  *cap = want;
  return KAIJU_GPU_OK;
}

}  // namespace

extern "C" int kaiju_gpu_merger_create(const kaiju_gpu_taxonomy *tax, int device_id, int conflict, int use_score, kaiju_gpu_merger **out) {
  return guarded([&]() -> int {
    if (!out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (conflict < KAIJU_GPU_MERGE_FIRST || conflict > KAIJU_GPU_MERGE_LOWEST) return fail(KAIJU_GPU_ERR_ARG, "conflict must be KAIJU_GPU_MERGE_FIRST, _SECOND, _LCA or _LOWEST");
    if (conflict == KAIJU_GPU_MERGE_LCA && !tax) return fail(KAIJU_GPU_ERR_ARG, "KAIJU_GPU_MERGE_LCA needs a tree");
    if (tax && tax->device != device_id) return fail(KAIJU_GPU_ERR_ARG, "the tree lives on another device");
    if (int rc = no_device()) return rc;
    kaiju_gpu_merger *a = new kaiju_gpu_merger();
    a->device = device_id;
    a->conflict = conflict;
    a->use_score = use_score ? 1 : 0;
    if (tax) a->tree = Tree{tax->dev.key, tax->dev.parent_slot, tax->dev.depth, tax->dev.cap_mask};
    if (hipSetDevice(a->device) != hipSuccess || hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc(&a->h_info, sizeof(kaiju_gpu_merge_info) + 8, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      kaiju_gpu_merger_free(a);
      return fail(KAIJU_GPU_ERR_HIP, "hipStreamCreate / hipHostMalloc of the merger");
    }
    const char *e = getenv("KAIJU_GPU_MERGE_TIMES");
    if (e && *e == '1') {
      for (hipEvent_t &ev : a->ev)
        if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); kaiju_gpu_merger_free(a); return fail(KAIJU_GPU_ERR_HIP, "hipEventCreate of the merger"); }
      a->timed = true;
    }
    *out = a;
    return KAIJU_GPU_OK;
  });
}

extern "C" void kaiju_gpu_merger_free(kaiju_gpu_merger *a) {
  if (!a) return;
  if (a->device >= 0 && hipSetDevice(a->device) == hipSuccess) {
    if (a->stream) { (void)hipStreamSynchronize(a->stream); (void)hipStreamDestroy(a->stream); }
    for (hipEvent_t ev : a->ev) if (ev) (void)hipEventDestroy(ev);
    if (a->h_info) (void)hipHostFree(a->h_info);
    if (a->h_text1) (void)hipHostFree(a->h_text1);
    if (a->h_text2) (void)hipHostFree(a->h_text2);
    if (a->h_out) (void)hipHostFree(a->h_out);
    a->st.release(); a->text1.release(); a->text2.release(); a->out.release(); a->info.release();
  }
  delete a;
}

extern "C" int kaiju_gpu_merge_text_device(kaiju_gpu_merger *a, const void *d_text1, uint64_t bytes1, const void *d_text2, uint64_t bytes2, int final,
                                           void *d_out, uint64_t out_cap, kaiju_gpu_merge_info *d_info, void *stream) {
  return guarded([&]() -> int {
    if (!a) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(a->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    return launch(a, stream ? static_cast<hipStream_t>(stream) : a->stream, d_text1, bytes1, d_text2, bytes2, final, d_out, out_cap, d_info);
  });
}

extern "C" int kaiju_gpu_merge_text(kaiju_gpu_merger *a, const char *text1, uint64_t bytes1, const char *text2, uint64_t bytes2, int final, char *out,
                                    uint64_t out_cap, kaiju_gpu_merge_info *info) {
  return guarded([&]() -> int {
    if (!a || !info || (!text1 && bytes1) || (!text2 && bytes2) || (!out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (bytes1 > kji::kMaxBytes || bytes2 > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
    if (hipSetDevice(a->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    const char *err = "";
    int rc;
    if ((rc = a->text1.reserve(bytes1 + kChunk, 256, "hipMalloc of the merger's text 1", &err))) return fail(rc, err);
    if ((rc = a->text2.reserve(bytes2 + kChunk, 256, "hipMalloc of the merger's text 2", &err))) return fail(rc, err);
    if ((rc = a->out.reserve(out_cap + kChunk, 256, "hipMalloc of the merger's output", &err))) return fail(rc, err);
    if ((rc = a->info.reserve(sizeof(kaiju_gpu_merge_info) + 8, 256, "hipMalloc of the merger's info", &err))) return fail(rc, err);
    if ((rc = pinned(&a->h_text1, &a->h_text1_cap, bytes1)) || (rc = pinned(&a->h_text2, &a->h_text2_cap, bytes2)) ||
        (rc = pinned(&a->h_out, &a->h_out_cap, out_cap)))
      return rc;
    const hipStream_t s = a->stream;
    if (bytes1) memcpy(a->h_text1, text1, bytes1);
    if (bytes2) memcpy(a->h_text2, text2, bytes2);
    if ((bytes1 && hipMemcpyAsync(a->text1.p, a->h_text1, bytes1, hipMemcpyHostToDevice, s) != hipSuccess) ||
        (bytes2 && hipMemcpyAsync(a->text2.p, a->h_text2, bytes2, hipMemcpyHostToDevice, s) != hipSuccess))
      return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the texts");
    kaiju_gpu_merge_info *d_info = static_cast<kaiju_gpu_merge_info *>(a->info.p);
    if ((rc = launch(a, s, a->text1.p, bytes1, a->text2.p, bytes2, final, a->out.p, out_cap, d_info))) return rc;
    // the info and, behind it, the number of bytes written
    uint8_t *h = static_cast<uint8_t *>(a->h_info);
    if (hipMemcpyAsync(h, d_info, sizeof *info, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(h + sizeof *info, a->st.written, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, std::string("the merge passes: ") + hipGetErrorString(hipGetLastError()));
    memcpy(info, h, sizeof *info);
    uint64_t written;
    memcpy(&written, h + sizeof *info, 8);
    if (written > out_cap) return fail(KAIJU_GPU_ERR_HIP, "the merge passes wrote more than out_cap");
    if (written && (hipMemcpyAsync(a->h_out, a->out.p, written, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess))
      return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the merged text");
    if (written) memcpy(out, a->h_out, written);
    return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_merge_pass_ms(kaiju_gpu_merger *a, float *ms, uint32_t n) {
  return guarded([&]() -> int {
    if (!a || (!ms && n)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (!a->timed) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "the merger was created without KAIJU_GPU_MERGE_TIMES=1");
    if (hipSetDevice(a->device) != hipSuccess || hipEventSynchronize(a->ev[KAIJU_GPU_MERGE_PASSES]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventSynchronize");
    for (uint32_t k = 0; k < n && k < KAIJU_GPU_MERGE_PASSES; k++)
      if (hipEventElapsedTime(&ms[k], a->ev[k], a->ev[k + 1]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventElapsedTime");
    return KAIJU_GPU_OK;
  });
}

extern "C" uint64_t kaiju_gpu_merge_bound(uint64_t bytes1, uint64_t bytes2) { return bound(bytes1, bytes2); }
