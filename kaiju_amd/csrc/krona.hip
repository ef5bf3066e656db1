// krona.hip — kaiju2krona's text from the counts of tallies (gfx950, wave64): the passes of kj_krona.h as kernels, and the
// entry points kaiju_gpu_krona_* of include/kaiju_gpu.h.  The counts live on the device (tally.hip: direct[] per slot of the
// tree), the lineage tables are built there, and the device-pointer form chains behind the tally without a synchronisation:
// the host never learns how many lines there are while the passes are queued.
//
// per (tree, list)  k_kr_keep        keep[] (one lane per slot)
//                   k_kr_tables      anc_len[], own_ok[]; the longest lineage
// per call          k_kr_init        the counters of the call
//                   k_kr_select      one lane per slot: the sum of the tallies' direct[], flag[]; the unnamed taxa
//                   kjl::k_scan_sums / k_scan_top / k_scan_apply <KrSlots>   pos[] = prefix sum of flag[]       (kj_lines.h)
//                   k_kr_compact     sel[], cnt[]: the slots that give a line, dense, in slot order
//                   k_kr_plan        by one lane: the Unclassified line behind them, the number of lines
//                   k_kr_len         one lane per line: its length
//                   kjl::k_scan_* <KrLines>                                  line_off[] = prefix sum of the lengths
//                   k_kr_write       one lane per 16 aligned bytes of the output                  (kj_lines.h: write_blocks)
//                   k_kr_finish      kaiju_gpu_krona_info; by one lane
//
// Every array of a call is sized by the slots of the tree and allocated at create.  Every loop is bounded by the data: the
// walks of kjk::build_anc_len / locate end because the loader refuses cycles, everything else runs over slots, lines or bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "kj_annotate.h"
#include "kj_krona.h"
#include "kj_tally.h"
#include "kj_lines.h"
#include "taxon_names.h"
#include "host/table_rows.h"

using namespace kjk;

typedef unsigned long long kr_u64;     // what atomicAdd takes

namespace {

constexpr int kKrBlock = 256;
static_assert(kKrBlock == (int)kjf::kBlockLanes && kKrBlock == kjs::kScanLanes, "one lane per chunk of a block of output / element of a scan block");
constexpr int kTotalsUnclassified = 2 + kjt::kCntUnclassified;   // in a tally's totals: used, n_lines, the counts

struct KrHdr { uint32_t n_lines, pad; uint64_t unnamed_taxa, unnamed_reads, n_unclassified; };

struct KrJob {
  const uint64_t *direct[kMaxTallies], *totals[kMaxTallies];
  uint32_t n_tallies, cap;
  int count_unclassified;
  uint32_t *flag;                      // cap
  uint64_t *sum;                       // cap
  uint64_t *pos;                       // cap + 1
  uint32_t *sel, *llen;                // cap + 1: a line per slot and the Unclassified line
  uint64_t *cnt;                       // cap + 1
  uint64_t *line_off;                  // cap + 2
  uint64_t *blk, *blk_base;
  KrHdr *hdr;
  uint8_t *out;
  uint64_t out_cap;
  kaiju_gpu_krona_info *info;
};

struct KrSlots { uint64_t cap; __device__ uint64_t operator()() const { return cap; } };                 // elements of the scans
struct KrLines { const KrHdr *hdr; __device__ uint64_t operator()() const { return hdr->n_lines; } };

__global__ __launch_bounds__(kKrBlock) void k_kr_keep(Tab T, const uint16_t *rank_of, const uint8_t *listed, uint8_t *keep) {
  for (uint32_t s = blockIdx.x * kKrBlock + threadIdx.x; s < T.cap; s += gridDim.x * kKrBlock) keep[s] = build_keep(T, rank_of, listed, s);
}

__global__ __launch_bounds__(kKrBlock) void k_kr_tables(Tab T, uint32_t *anc_len, uint8_t *own_ok, kr_u64 *longest) {
  kr_u64 most = 0;
  for (uint32_t s = blockIdx.x * kKrBlock + threadIdx.x; s < T.cap; s += gridDim.x * kKrBlock) {
    const uint64_t len = build_anc_len(T, s);
    anc_len[s] = kjn::clamp32(len);
    own_ok[s] = build_own_ok(T, s);
    most = len > most ? len : most;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const kr_u64 o = __shfl_xor(most, d, 64);
    most = o > most ? o : most;
  }
  if ((threadIdx.x & 63) == 0 && most) atomicMax(longest, most);
}

__global__ void k_kr_init(KrHdr *h) {
  if (blockIdx.x || threadIdx.x) return;
  *h = KrHdr{0, 0, 0, 0, 0};
}

__global__ __launch_bounds__(kKrBlock) void k_kr_select(KrJob J, Tab T) {
  kr_u64 taxa = 0, reads = 0;
  for (uint32_t s = blockIdx.x * kKrBlock + threadIdx.x; s < J.cap; s += gridDim.x * kKrBlock) {
    uint64_t d = 0;
    for (uint32_t t = 0; t < J.n_tallies; t++) d += J.direct[t][s];
    uint32_t unnamed;
    J.flag[s] = selects(T, s, d, &unnamed);
    J.sum[s] = d;
    taxa += unnamed;
    reads += unnamed ? d : 0;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { taxa += __shfl_xor(taxa, d, 64); reads += __shfl_xor(reads, d, 64); }
  if ((threadIdx.x & 63) == 0 && taxa) {
    atomicAdd(reinterpret_cast<kr_u64 *>(&J.hdr->unnamed_taxa), taxa);
    atomicAdd(reinterpret_cast<kr_u64 *>(&J.hdr->unnamed_reads), reads);
  }
}

__global__ __launch_bounds__(kKrBlock) void k_kr_compact(KrJob J) {
  for (uint32_t s = blockIdx.x * kKrBlock + threadIdx.x; s < J.cap; s += gridDim.x * kKrBlock)
    if (J.flag[s]) { const uint64_t i = J.pos[s]; J.sel[i] = s; J.cnt[i] = J.sum[s]; }          // (i < cap: flags of cap slots)
}

__global__ void k_kr_plan(KrJob J) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t n = (uint32_t)J.pos[J.cap];
  uint64_t u = 0;
  if (J.count_unclassified)
    for (uint32_t t = 0; t < J.n_tallies; t++) u += J.totals[t][kTotalsUnclassified];
  if (u) { J.sel[n] = kNone; J.cnt[n] = u; n++; }
  J.hdr->n_lines = n;
  J.hdr->n_unclassified = u;
}

__global__ __launch_bounds__(kKrBlock) void k_kr_len(KrJob J, Tab T) {
  const uint32_t n = J.hdr->n_lines;
  for (uint32_t r = blockIdx.x * kKrBlock + threadIdx.x; r < n; r += gridDim.x * kKrBlock) J.llen[r] = line_len(T, J.sel[r], J.cnt[r]);
}

__global__ __launch_bounds__(kKrBlock) void k_kr_write(KrJob J, Tab T) {
  kjl::write_blocks(J.line_off, J.hdr->n_lines, J.out, J.out_cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) {
    return format_chunk(c, T, J.line_off, J.sel, J.cnt, lo, hi, total, J.out_cap, v);
  });
}

__global__ void k_kr_finish(KrJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const KrHdr &H = *J.hdr;
  *J.info = make_info(J.line_off, H.n_lines, J.out_cap, H.unnamed_taxa, H.unnamed_reads, H.n_unclassified);
}

void carve(kjl::Carver &c, KrJob &J, uint32_t cap) {
  const size_t nblk = ((size_t)cap + 1) / kjs::kScanLanes + 2;
  J.flag = c.take<uint32_t>(cap);
  J.sum = c.take<uint64_t>(cap);
  J.pos = c.take<uint64_t>((size_t)cap + 1);
  J.sel = c.take<uint32_t>((size_t)cap + 1);
  J.llen = c.take<uint32_t>((size_t)cap + 1);
  J.cnt = c.take<uint64_t>((size_t)cap + 1);
  J.line_off = c.take<uint64_t>((size_t)cap + 2);
  J.blk = c.take<uint64_t>(nblk);
  J.blk_base = c.take<uint64_t>(nblk + 1);
  J.hdr = c.take<KrHdr>(1);
}

// p is device memory of a device other than `device` (what the runtime does not know is taken as it is)
bool on_other_device(const void *p, int device) {
  hipPointerAttribute_t at;
  if (!p) return false;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeDevice && at.device != device;
}

dim3 slot_grid(uint32_t cap) { return dim3((unsigned)std::min<uint64_t>(4096, (uint64_t)cap / kKrBlock + 1)); }

}  // namespace

struct kaiju_gpu_krona {
  const kaiju_gpu_taxon_names *names = nullptr;
  int device = -1;
  Tab tab{};
  std::vector<void *> allocs;          // the tables
  KrJob job{};                         // the arrays of a call, carved from `mem`
  void *mem = nullptr;
  kjl::Scratch text, info;             // device staging of the host form
  void *h_info = nullptr;              // pinned
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;           // behind the last call, on whichever stream it ran
  bool timed = false;                  // KAIJU_GPU_KRONA_TIMES=1: events between the passes (kaiju_gpu_krona_pass_ms)
  hipEvent_t ev[KAIJU_GPU_KRONA_PASSES + 1] = {};
};

namespace {

int launch(kaiju_gpu_krona *k, hipStream_t s, kaiju_gpu_tally *const *tallies, uint32_t n_tallies, int count_unclassified, void *d_out, uint64_t out_cap,
           kaiju_gpu_krona_info *d_info) {
  if (!tallies || !d_info || (!d_out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (n_tallies == 0 || n_tallies > kMaxTallies) return fail(KAIJU_GPU_ERR_ARG, "between 1 and " + std::to_string(kMaxTallies) + " tallies");
  if ((uintptr_t)d_out & (kChunk - 1)) return fail(KAIJU_GPU_ERR_ARG, "the output must be 16-byte aligned");
  if (on_other_device(d_out, k->device) || on_other_device(d_info, k->device)) return fail(KAIJU_GPU_ERR_ARG, "the output or the info lives on another device than the taxon names");
  KrJob J = k->job;
  kj_tally_view view[kMaxTallies];
  for (uint32_t t = 0; t < n_tallies; t++) {
    if (!tallies[t]) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    view[t] = kj_tally_view_of(tallies[t]);
    if (view[t].names != k->names || view[t].device != k->device) return fail(KAIJU_GPU_ERR_ARG, "a tally of other taxon names or another device");
    J.direct[t] = view[t].direct;
    J.totals[t] = view[t].totals;
  }
  J.n_tallies = n_tallies;
  J.count_unclassified = count_unclassified ? 1 : 0;
  J.out = static_cast<uint8_t *>(d_out); J.out_cap = out_cap; J.info = d_info;
  const Tab &T = k->tab;

  const dim3 blk(kKrBlock), grid = slot_grid(J.cap);
  const dim3 sgrid((unsigned)std::min<uint64_t>(2048, ((uint64_t)J.cap + 1) / kjs::kScanLanes + 1));
  const dim3 wgrid((unsigned)std::min<uint64_t>(2048, out_cap / kjf::kBlockBytes + 1));
  int mark = 0;
  auto passed = [&]() { if (k->timed) (void)hipEventRecord(k->ev[mark++], s); };
  if (hipStreamWaitEvent(s, k->done, 0) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipStreamWaitEvent of the krona object");
  for (uint32_t t = 0; t < n_tallies; t++)
    if (hipStreamWaitEvent(s, view[t].done, 0) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipStreamWaitEvent of a tally");
  passed();
  hipLaunchKernelGGL(k_kr_init, dim3(1), dim3(64), 0, s, J.hdr);
  hipLaunchKernelGGL(k_kr_select, grid, blk, 0, s, J, T);
  passed();
  kjl::launch_offsets(s, sgrid, KrSlots{J.cap}, J.flag, J.blk, J.blk_base, J.pos);
  hipLaunchKernelGGL(k_kr_compact, grid, blk, 0, s, J);
  hipLaunchKernelGGL(k_kr_plan, dim3(1), dim3(64), 0, s, J);
  passed();
  hipLaunchKernelGGL(k_kr_len, grid, blk, 0, s, J, T);
  kjl::launch_offsets(s, sgrid, KrLines{J.hdr}, J.llen, J.blk, J.blk_base, J.line_off);
  passed();
  hipLaunchKernelGGL(k_kr_write, wgrid, blk, 0, s, J, T);
  passed();
  hipLaunchKernelGGL(k_kr_finish, dim3(1), dim3(64), 0, s, J);
  passed();
  if (hipGetLastError() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "a kernel of the krona passes could not be launched");
  // a later call of a tally (a reset, more text) waits until its counts have been read
  for (uint32_t t = 0; t < n_tallies; t++)
    if (hipEventRecord(view[t].done, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventRecord of a tally");
  if (hipEventRecord(k->done, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventRecord of the krona object");
  return KAIJU_GPU_OK;
}

}  // namespace

extern "C" int kaiju_gpu_krona_create(const kaiju_gpu_taxon_names *names, const char *ranks_csv, kaiju_gpu_krona **out) {
  return guarded([&]() -> int {
    if (!names || !out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    *out = nullptr;
    const kaiju_krona_source &src = *kj_fn_krona_source(names);
    const kjn::Tab &N = *kj_fn_tab(names);
    const uint32_t cap = N.cap_mask + 1;
    const std::vector<std::string> list = kjtr::split_ranks(ranks_csv ? ranks_csv : "");
    if (list.size() > kjn::kMaxList) return fail(KAIJU_GPU_ERR_ARG, "more than " + std::to_string(kjn::kMaxList) + " items in the list of ranks");
    if (src.rank_of.size() != cap || src.dang_len.size() != cap || src.dang_pos.size() != cap) return fail(KAIJU_GPU_ERR_ARG, "the taxon names hold no ranks");
    for (uint32_t l : src.dang_len)
      if (l == kNone) return fail(KAIJU_GPU_ERR_ARG, "a name of 2^24 bytes or more");
    // (the tool keeps a list whenever -l is given, an empty one too: then no name is printed at all)
    const bool has_list = ranks_csv != nullptr;
    std::vector<uint8_t> listed(src.rank_names.size() + 1, 0);
    for (size_t r = 0; r < src.rank_names.size(); r++) listed[r] = std::find(list.begin(), list.end(), src.rank_names[r]) != list.end() ? 1 : 0;

    kaiju_gpu_krona *k = new kaiju_gpu_krona();
    struct Guard { kaiju_gpu_krona *p; ~Guard() { kaiju_gpu_krona_free(p); } } guard{k};
    k->names = names;
    k->device = kj_fn_device(names);
    if (hipSetDevice(k->device) != hipSuccess || hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&k->done, hipEventDisableTiming) != hipSuccess || hipHostMalloc(&k->h_info, sizeof(kaiju_gpu_krona_info), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(KAIJU_GPU_ERR_HIP, "hipStreamCreate / hipHostMalloc of the krona object");
    }
    const char *e = getenv("KAIJU_GPU_KRONA_TIMES");
    if (e && *e == '1') {
      for (hipEvent_t &ev : k->ev)
        if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); return fail(KAIJU_GPU_ERR_HIP, "hipEventCreate of the krona object"); }
      k->timed = true;
    }
    bool ok = true;
    auto alloc = [&](size_t bytes) -> void * {
      void *p = nullptr;
      if (hipMalloc(&p, bytes + 16) != hipSuccess) { (void)hipGetLastError(); ok = false; return nullptr; }
      k->allocs.push_back(p);
      return p;
    };
    auto up = [&](const void *from, size_t bytes) -> const void * {
      void *p = alloc(bytes);
      if (!p || (bytes && hipMemcpy(p, from, bytes, hipMemcpyHostToDevice) != hipSuccess)) { ok = false; return nullptr; }
      return p;
    };
    Tab &T = k->tab;
    T.key = N.key; T.parent = N.parent; T.name_pos = N.name_pos; T.name_len = N.name_len; T.blob = N.blob;
    T.cap = cap; T.has_list = has_list ? 1 : 0;
    T.dang_pos = static_cast<const uint32_t *>(up(src.dang_pos.data(), (size_t)cap * 4));
    T.dang_len = static_cast<const uint32_t *>(up(src.dang_len.data(), (size_t)cap * 4));
    T.dang_blob = static_cast<const uint8_t *>(up(src.dang_blob.data(), src.dang_blob.size()));
    const uint16_t *d_rank_of = static_cast<const uint16_t *>(up(src.rank_of.data(), (size_t)cap * 2));
    const uint8_t *d_listed = static_cast<const uint8_t *>(up(listed.data(), listed.size()));
    uint8_t *keep = static_cast<uint8_t *>(alloc(cap)), *own_ok = static_cast<uint8_t *>(alloc(cap));
    uint32_t *anc_len = static_cast<uint32_t *>(alloc((size_t)cap * 4));
    kr_u64 *d_longest = static_cast<kr_u64 *>(alloc(8));
    kjl::Carver measure{nullptr};
    carve(measure, k->job, cap);
    if (ok && hipMalloc(&k->mem, measure.at + 256) != hipSuccess) { (void)hipGetLastError(); ok = false; }
    if (!ok) return fail(KAIJU_GPU_ERR_NOMEM, "hipMalloc / hipMemcpy of the krona tables");
    kjl::Carver c{static_cast<uint8_t *>(k->mem)};
    carve(c, k->job, cap);
    k->job.cap = cap;
    T.keep = keep; T.own_ok = own_ok; T.anc_len = anc_len;
    if (hipMemset(d_longest, 0, 8) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemset");
    hipLaunchKernelGGL(k_kr_keep, slot_grid(cap), dim3(kKrBlock), 0, 0, T, d_rank_of, d_listed, keep);
    hipLaunchKernelGGL(k_kr_tables, slot_grid(cap), dim3(kKrBlock), 0, 0, T, anc_len, own_ok, d_longest);
    kr_u64 longest = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpy(&longest, d_longest, 8, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, "the kernels that build the krona tables");
    if (longest >= kMaxLineage) return fail(KAIJU_GPU_ERR_ARG, "a lineage of " + std::to_string(longest) + " bytes: 2^24 or more");
    if (hipEventRecord(k->done, k->stream) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventRecord of the krona object");
    guard.p = nullptr;
    *out = k;
    return KAIJU_GPU_OK;
  });
}

extern "C" void kaiju_gpu_krona_free(kaiju_gpu_krona *k) {
  if (!k) return;
  if (k->device >= 0 && hipSetDevice(k->device) == hipSuccess) {
    if (k->done) { (void)hipEventSynchronize(k->done); (void)hipEventDestroy(k->done); }
    if (k->stream) { (void)hipStreamSynchronize(k->stream); (void)hipStreamDestroy(k->stream); }
    for (hipEvent_t ev : k->ev) if (ev) (void)hipEventDestroy(ev);
    if (k->h_info) (void)hipHostFree(k->h_info);
    if (k->mem) (void)hipFree(k->mem);
    for (void *p : k->allocs) (void)hipFree(p);
    k->text.release(); k->info.release();
  }
  delete k;
}

extern "C" int kaiju_gpu_krona_text_device(kaiju_gpu_krona *k, kaiju_gpu_tally *const *tallies, uint32_t n_tallies, int count_unclassified, void *d_out,
                                           uint64_t out_cap, kaiju_gpu_krona_info *d_info, void *stream) {
  return guarded([&]() -> int {
    if (!k) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(k->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    return launch(k, stream ? static_cast<hipStream_t>(stream) : k->stream, tallies, n_tallies, count_unclassified, d_out, out_cap, d_info);
  });
}

extern "C" int kaiju_gpu_krona_text(kaiju_gpu_krona *k, kaiju_gpu_tally *const *tallies, uint32_t n_tallies, int count_unclassified, char *buf, uint64_t cap,
                                    kaiju_gpu_krona_info *info) {
  return guarded([&]() -> int {
    if (!k || !info || (!buf && cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(k->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    const char *err = "";
    int rc;
    if ((rc = k->text.reserve(cap + kChunk, 256, "hipMalloc of the krona text", &err))) return fail(rc, err);
    if ((rc = k->info.reserve(sizeof(kaiju_gpu_krona_info), 256, "hipMalloc of the krona info", &err))) return fail(rc, err);
    const hipStream_t s = k->stream;
    kaiju_gpu_krona_info *d_info = static_cast<kaiju_gpu_krona_info *>(k->info.p);
    if ((rc = launch(k, s, tallies, n_tallies, count_unclassified, cap ? k->text.p : nullptr, cap, d_info))) return rc;
    if (hipMemcpyAsync(k->h_info, d_info, sizeof *info, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, std::string("the krona passes: ") + hipGetErrorString(hipGetLastError()));
    memcpy(info, k->h_info, sizeof *info);
    if (info->written_bytes > cap) return fail(KAIJU_GPU_ERR_HIP, "the krona passes wrote more than the buffer holds");
    if (info->written_bytes && hipMemcpy(buf, k->text.p, info->written_bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the krona text");
    return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_krona_pass_ms(kaiju_gpu_krona *k, float *ms, uint32_t n) {
  return guarded([&]() -> int {
    if (!k || (!ms && n)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (!k->timed) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "the krona object was created without KAIJU_GPU_KRONA_TIMES=1");
    if (hipSetDevice(k->device) != hipSuccess || hipEventSynchronize(k->ev[KAIJU_GPU_KRONA_PASSES]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventSynchronize");
    for (uint32_t p = 0; p < n && p < KAIJU_GPU_KRONA_PASSES; p++)
      if (hipEventElapsedTime(&ms[p], k->ev[p], k->ev[p + 1]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventElapsedTime");
    return KAIJU_GPU_OK;
  });
}
