// gbk.hip — kaiju-gbk2faa on a block of GenBank flat-file text (gfx950, wave64): the passes of kj_gbk.h as kernels, and the
// entry points kaiju_gpu_gbk_* of include/kaiju_gpu.h.  The host never learns a count while the passes are queued: every kernel
// behind the first sizes itself from counts in device memory.
//
// per call    k_gb_init        the counters
//             k_tl_*           the lines                                                              (kj_textlines.h)
//             k_gb_kinds       one lane per line: its kind and capture.  A line without a `"` is nothing: six 16-byte loads
//             k_gb_scan_sums / _top / _apply   the three maximum-scans over the lines on kjs::block_scan_excl, the block on top
//                              seeded with nothing: a result of 0 stands for the carried state        (kj_scan.h)
//             k_gb_len         one lane per line: the bytes it gives to the output, the first line that lacks a taxon
//             kjl::k_scan_* <GbLines>   line_off[]                                                     (kj_lines.h)
//             k_gb_write       per lane 16 aligned bytes of the output: kjl::write_blocks over gbk_chunk
//             k_gb_finish      kaiju_gpu_gbk_info and the scalars of the carried state, by one lane
//             k_gb_carry       the strings of the carried state, if it advanced
// The carried state - kjg::Carry and two strings that may be as long as a line - lives in device memory of the object; the
// strings' buffers grow with the largest block seen.  Every loop runs over bytes or lines.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "kj_gbk.h"
#include "kj_lines.h"
#include "kj_textlines.h"

using namespace kjg;

typedef unsigned long long gb_u64;

namespace {

constexpr int kGbBlock = 256;
static_assert(kGbBlock == (int)kjf::kBlockLanes && kGbBlock == kjs::kScanLanes, "one lane per chunk of a block of output / element of a scan block");

struct OpMax32 { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct OpMax64 { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; } };
template <class T> __device__ __forceinline__ T mx(T a, T b) { return a > b ? a : b; }

struct GbJob {
  TlText t;
  uint8_t *kind;                       // per line
  uint32_t *cap_a, *cap_e;
  uint32_t *tax_src, *pid_src;
  uint8_t *in_t;
  uint64_t *olen;                      // per line
  uint64_t *line_off;                  // lines + 1
  uint64_t *blk, *blk_base;
  uint32_t *sb_tax, *sb_pid, *sbb_tax, *sbb_pid;   // per scan block: its maximum, the maximum in front of it
  uint64_t *sb_ev, *sbb_ev;
  Totals *tot;
  Carry *carry;
  uint8_t *carry_tax, *carry_pid;
  uint8_t *out;
  uint64_t out_cap;
  kaiju_gpu_gbk_info *info;
};

struct GbLines { const uint32_t *n; __device__ uint64_t operator()() const { return *n; } };

void carve(kjl::Carver &c, GbJob &J) {
  tl_carve(c, J.t);
  const size_t lines = J.t.bytes + 1, nblk = lines / kjs::kScanLanes + 2;
  J.kind = c.take<uint8_t>(lines);
  J.cap_a = c.take<uint32_t>(lines);
  J.cap_e = c.take<uint32_t>(lines);
  J.tax_src = c.take<uint32_t>(lines);
  J.pid_src = c.take<uint32_t>(lines);
  J.in_t = c.take<uint8_t>(lines);
  J.olen = c.take<uint64_t>(lines);
  J.line_off = c.take<uint64_t>(lines + 1);
  J.blk = c.take<uint64_t>(nblk);
  J.blk_base = c.take<uint64_t>(nblk + 1);
  J.sb_tax = c.take<uint32_t>(nblk);
  J.sb_pid = c.take<uint32_t>(nblk);
  J.sbb_tax = c.take<uint32_t>(nblk);
  J.sbb_pid = c.take<uint32_t>(nblk);
  J.sb_ev = c.take<uint64_t>(nblk);
  J.sbb_ev = c.take<uint64_t>(nblk);
  J.tot = c.take<Totals>(1);
}

__device__ __forceinline__ View view_of(const GbJob &J) {
  return View{J.t.text, J.t.line_start, J.kind, J.cap_a, J.cap_e, J.tax_src, J.pid_src, J.in_t, J.carry, J.carry_tax, J.carry_pid, *J.t.n_lines};
}

__device__ __forceinline__ gb_u64 wave_sum(gb_u64 v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ void k_gb_init(Totals *t) {
  if (blockIdx.x || threadIdx.x) return;
  *t = Totals{};
  t->no_tax_line = kNone;
}

__global__ __launch_bounds__(kGbBlock) void k_gb_kinds(GbJob J) {
  const uint32_t n = *J.t.n_lines;
  gb_u64 cnt[5] = {0, 0, 0, 0, 0};
  for (uint32_t i = blockIdx.x * kGbBlock + threadIdx.x; i < n; i += gridDim.x * kGbBlock) {
    const LineKind L = classify(J.t.text, J.t.line_start[i], (uint64_t)J.t.line_start[i + 1] - 1);
    J.kind[i] = (uint8_t)L.kind; J.cap_a[i] = L.cap_a; J.cap_e[i] = L.cap_e;
#pragma unroll
    for (uint32_t k = 0; k < 5; k++) cnt[k] += (L.kind & kKindMask) == k + 1 ? 1u : 0u;
  }
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const gb_u64 v = wave_sum(cnt[k]);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(reinterpret_cast<gb_u64 *>(&J.tot->kinds[k]), v);
  }
}

// the maxima of every block of kScanLanes lines
__global__ __launch_bounds__(kGbBlock) void k_gb_scan_sums(GbJob J) {
  const uint64_t n = *J.t.n_lines, nb = (n + kGbBlock - 1) / kGbBlock;
  for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t i = b * kGbBlock + threadIdx.x;
    uint32_t tax = 0, pid = 0, t_tax, t_pid;
    uint64_t ev = 0, t_ev;
    if (i < n) scan_values(J.kind[i], (uint32_t)i, &tax, &pid, &ev);
    kjs::block_scan_excl<uint32_t>(tax, 0u, &t_tax, OpMax32());
    kjs::block_scan_excl<uint32_t>(pid, 0u, &t_pid, OpMax32());
    kjs::block_scan_excl<uint64_t>(ev, 0ull, &t_ev, OpMax64());
    if (threadIdx.x == 0) { J.sb_tax[b] = t_tax; J.sb_pid[b] = t_pid; J.sb_ev[b] = t_ev; }
  }
}

// one block walks those maxima kScanLanes at a time: what lies in front of every block, and the maxima over all lines
__global__ __launch_bounds__(kGbBlock) void k_gb_scan_top(GbJob J) {
  const uint64_t n = *J.t.n_lines, nb = (n + kGbBlock - 1) / kGbBlock;
  uint32_t c_tax = 0, c_pid = 0;
  uint64_t c_ev = 0;
  for (uint64_t i0 = 0; i0 < nb; i0 += kGbBlock) {
    const uint64_t i = i0 + threadIdx.x;
    uint32_t t_tax, t_pid;
    uint64_t t_ev;
    const uint32_t x_tax = kjs::block_scan_excl<uint32_t>(i < nb ? J.sb_tax[i] : 0u, 0u, &t_tax, OpMax32());
    const uint32_t x_pid = kjs::block_scan_excl<uint32_t>(i < nb ? J.sb_pid[i] : 0u, 0u, &t_pid, OpMax32());
    const uint64_t x_ev = kjs::block_scan_excl<uint64_t>(i < nb ? J.sb_ev[i] : 0ull, 0ull, &t_ev, OpMax64());
    if (i < nb) { J.sbb_tax[i] = mx(c_tax, x_tax); J.sbb_pid[i] = mx(c_pid, x_pid); J.sbb_ev[i] = mx(c_ev, x_ev); }
    c_tax = mx(c_tax, t_tax); c_pid = mx(c_pid, t_pid); c_ev = mx(c_ev, t_ev);
  }
  if (threadIdx.x == 0) { J.tot->fin_tax = c_tax; J.tot->fin_pid = c_pid; J.tot->fin_ev = c_ev; }
}

__global__ __launch_bounds__(kGbBlock) void k_gb_scan_apply(GbJob J) {
  const uint64_t n = *J.t.n_lines, nb = (n + kGbBlock - 1) / kGbBlock;
  const Carry C = *J.carry;
  for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t i = b * kGbBlock + threadIdx.x;
    uint32_t tax = 0, pid = 0, t_tax, t_pid;
    uint64_t ev = 0, t_ev;
    if (i < n) scan_values(J.kind[i], (uint32_t)i, &tax, &pid, &ev);
    const uint32_t x_tax = kjs::block_scan_excl<uint32_t>(tax, 0u, &t_tax, OpMax32());
    const uint32_t x_pid = kjs::block_scan_excl<uint32_t>(pid, 0u, &t_pid, OpMax32());
    const uint64_t x_ev = kjs::block_scan_excl<uint64_t>(ev, 0ull, &t_ev, OpMax64());
    if (i < n) {
      J.tax_src[i] = mx(J.sbb_tax[b], x_tax);
      J.pid_src[i] = mx(J.sbb_pid[b], x_pid);
      J.in_t[i] = (uint8_t)inside(mx(J.sbb_ev[b], x_ev), C);
    }
  }
}

__global__ __launch_bounds__(kGbBlock) void k_gb_len(GbJob J) {
  const View V = view_of(J);
  gb_u64 records = 0, kept = 0, dropped = 0;
  uint32_t first_bad = kNone;
  for (uint32_t i = blockIdx.x * kGbBlock + threadIdx.x; i < V.n_lines; i += gridDim.x * kGbBlock) {
    if (lacks_taxon(V, i) && first_bad == kNone) first_bad = i + 1;
    const Out o = line_out(V, i);
    J.olen[i] = o.hdr + o.seq;
    if (o.hdr) records++;
    if (o.seq) { kept += o.seq - 1; dropped += o.span - (o.seq - 1); }
  }
  if (first_bad != kNone) atomicMin(&J.tot->no_tax_line, first_bad);
  records = wave_sum(records); kept = wave_sum(kept); dropped = wave_sum(dropped);
  if ((threadIdx.x & 63) == 0 && (records | kept | dropped)) {
    atomicAdd(reinterpret_cast<gb_u64 *>(&J.tot->records), records);
    atomicAdd(reinterpret_cast<gb_u64 *>(&J.tot->kept), kept);
    atomicAdd(reinterpret_cast<gb_u64 *>(&J.tot->dropped), dropped);
  }
}

__global__ __launch_bounds__(kGbBlock) void k_gb_write(GbJob J) {
  const View V = view_of(J);
  const uint64_t cap = J.tot->no_tax_line != kNone ? 0 : J.out_cap;       // the script's file is empty then
  kjl::write_blocks(J.line_off, V.n_lines, J.out, cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) {
    return gbk_chunk(c, V, J.line_off, lo, hi, total, cap, v);
  });
}

__global__ void k_gb_finish(GbJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const View V = view_of(J);
  *J.info = finish(V, J.line_off, J.out_cap, *J.tot, *J.carry);
}

// the captures of the last kind 1 and kind 2 line into the carried strings (they have room for a whole block)
__global__ __launch_bounds__(kGbBlock) void k_gb_carry(GbJob J) {
  const Totals &T = *J.tot;
  if (!T.advance) return;
  const uint64_t at = (uint64_t)blockIdx.x * kGbBlock + threadIdx.x, step = (uint64_t)gridDim.x * kGbBlock;
  if (T.fin_tax) {
    const uint64_t a = J.cap_a[T.fin_tax - 1], n = J.cap_e[T.fin_tax - 1] - a;
    for (uint64_t p = at; p < n; p += step) J.carry_tax[p] = J.t.text[a + p];
  }
  if (T.fin_pid) {
    const uint64_t a = J.cap_a[T.fin_pid - 1], n = J.cap_e[T.fin_pid - 1] - a;
    for (uint64_t p = at; p < n; p += step) J.carry_pid[p] = J.t.text[a + p];
  }
}

bool on_other_device(const void *p, int device) {
  hipPointerAttribute_t at;
  if (!p) return false;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeDevice && at.device != device;
}

// device memory of `bytes` bytes, asked for only when that much is free
int dev_alloc(void **p, uint64_t bytes, const char *what) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemGetInfo");
  if (bytes > free_b)
    return fail(KAIJU_GPU_ERR_NOMEM, std::string(what) + ": need " + std::to_string(bytes >> 20) + " MiB of device memory, " + std::to_string(free_b >> 20) + " MiB are free");
  if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(KAIJU_GPU_ERR_NOMEM, std::string(what) + ": hipMalloc of " + std::to_string(bytes >> 20) + " MiB"); }
  return KAIJU_GPU_OK;
}

}  // namespace

struct kaiju_gpu_gbk {
  int device = -1;
  Carry *carry = nullptr;
  uint8_t *carry_tax = nullptr, *carry_pid = nullptr;
  uint64_t carry_cap = 0;              // bytes of either string
  kjl::Scratch mem, text, out, info;
  void *h_info = nullptr;              // pinned
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;           // behind the last call, on whichever stream it ran
  bool timed = false;
  hipEvent_t ev[KAIJU_GPU_GBK_PASSES + 1] = {};
};

namespace {

// room for a capture of `bytes` bytes in both carried strings; what they hold is kept
int grow_carry(kaiju_gpu_gbk *k, uint64_t bytes) {
  if (bytes <= k->carry_cap) return KAIJU_GPU_OK;
  const uint64_t want = bytes + bytes / 8 + 256;
  uint8_t *tax = nullptr, *pid = nullptr;
  if (hipDeviceSynchronize() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipDeviceSynchronize in front of growing the carried strings");
  if (int rc = dev_alloc(reinterpret_cast<void **>(&tax), want, "the carried taxon of the GenBank converter")) return rc;
  if (int rc = dev_alloc(reinterpret_cast<void **>(&pid), want, "the carried protein id of the GenBank converter")) { (void)hipFree(tax); return rc; }
  if (k->carry_cap && (hipMemcpy(tax, k->carry_tax, k->carry_cap, hipMemcpyDeviceToDevice) != hipSuccess ||
                       hipMemcpy(pid, k->carry_pid, k->carry_cap, hipMemcpyDeviceToDevice) != hipSuccess)) {
    (void)hipFree(tax); (void)hipFree(pid);
    return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the carried strings");
  }
  if (k->carry_tax) (void)hipFree(k->carry_tax);
  if (k->carry_pid) (void)hipFree(k->carry_pid);
  k->carry_tax = tax; k->carry_pid = pid; k->carry_cap = want;
  return KAIJU_GPU_OK;
}

int launch(kaiju_gpu_gbk *k, hipStream_t s, const void *d_text, uint64_t bytes, void *d_out, uint64_t out_cap, kaiju_gpu_gbk_info *d_info) {
  if (!d_info || (!d_text && bytes) || (!d_out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (bytes > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
  if (((uintptr_t)d_text | (uintptr_t)d_out) & (kChunk - 1)) return fail(KAIJU_GPU_ERR_ARG, "the text and the output pointer must be 16-byte aligned");
  if (on_other_device(d_text, k->device) || on_other_device(d_out, k->device) || on_other_device(d_info, k->device))
    return fail(KAIJU_GPU_ERR_ARG, "the text, the output or the info lives on another device than the converter");
  GbJob J{};
  J.t.text = static_cast<const uint8_t *>(d_text); J.t.bytes = bytes;
  kjl::Carver measure{nullptr};
  carve(measure, J);
  const char *err = "";
  if (int rc = k->mem.reserve(measure.at, 256, "hipMalloc of the GenBank converter's scratch", &err)) return fail(rc, err);
  if (int rc = grow_carry(k, bytes)) return rc;
  kjl::Carver c{static_cast<uint8_t *>(k->mem.p)};
  carve(c, J);
  J.carry = k->carry; J.carry_tax = k->carry_tax; J.carry_pid = k->carry_pid;
  J.out = static_cast<uint8_t *>(d_out); J.out_cap = out_cap; J.info = d_info;

  const dim3 blk(kGbBlock);
  const dim3 lgrid((unsigned)std::min<uint64_t>(4096, bytes / (16 * kGbBlock) + 1));      // passes over lines
  const dim3 sgrid((unsigned)std::min<uint64_t>(2048, (bytes + 1) / kjs::kScanLanes + 1));
  const dim3 wgrid((unsigned)std::min<uint64_t>(8192, out_cap / kjf::kBlockBytes + 1));
  const GbLines count{J.t.n_lines};
  int mark = 0;
  auto passed = [&]() { if (k->timed) (void)hipEventRecord(k->ev[mark++], s); };
  if (hipStreamWaitEvent(s, k->done, 0) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipStreamWaitEvent of the GenBank converter");
  passed();
  hipLaunchKernelGGL(k_gb_init, dim3(1), dim3(64), 0, s, J.tot);
  tl_launch(s, J.t);
  passed();
  hipLaunchKernelGGL(k_gb_kinds, lgrid, blk, 0, s, J);
  passed();
  hipLaunchKernelGGL(k_gb_scan_sums, sgrid, blk, 0, s, J);
  hipLaunchKernelGGL(k_gb_scan_top, dim3(1), blk, 0, s, J);
  hipLaunchKernelGGL(k_gb_scan_apply, sgrid, blk, 0, s, J);
  passed();
  hipLaunchKernelGGL(k_gb_len, lgrid, blk, 0, s, J);
  kjl::launch_offsets(s, sgrid, count, static_cast<const uint64_t *>(J.olen), J.blk, J.blk_base, J.line_off);
  passed();
  hipLaunchKernelGGL(k_gb_write, wgrid, blk, 0, s, J);
  passed();
  hipLaunchKernelGGL(k_gb_finish, dim3(1), dim3(64), 0, s, J);
  hipLaunchKernelGGL(k_gb_carry, dim3(64), blk, 0, s, J);
  passed();
  if (hipGetLastError() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "a kernel of the GenBank passes could not be launched");
  if (hipEventRecord(k->done, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventRecord of the GenBank converter");
  return KAIJU_GPU_OK;
}

}  // namespace

extern "C" int kaiju_gpu_gbk_create(int device_id, kaiju_gpu_gbk **out) {
  return guarded([&]() -> int {
    if (!out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (int rc = no_device()) return rc;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device_id < 0 || device_id >= n_dev) { (void)hipGetLastError(); return fail(KAIJU_GPU_ERR_ARG, "no such device"); }
    kaiju_gpu_gbk *k = new kaiju_gpu_gbk();
    struct Guard { kaiju_gpu_gbk *p; ~Guard() { kaiju_gpu_gbk_free(p); } } guard{k};
    k->device = device_id;
    if (hipSetDevice(k->device) != hipSuccess || hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&k->done, hipEventDisableTiming) != hipSuccess || hipHostMalloc(&k->h_info, sizeof(kaiju_gpu_gbk_info) + 8, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(KAIJU_GPU_ERR_HIP, "hipStreamCreate / hipHostMalloc of the GenBank converter");
    }
    const char *e = getenv("KAIJU_GPU_CONVERT_TIMES");
    if (e && *e == '1') {
      for (hipEvent_t &ev : k->ev)
        if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); return fail(KAIJU_GPU_ERR_HIP, "hipEventCreate of the GenBank converter"); }
      k->timed = true;
    }
    if (int rc = dev_alloc(reinterpret_cast<void **>(&k->carry), 256, "the carried state of the GenBank converter")) return rc;
    if (int rc = grow_carry(k, 4096)) return rc;
    if (hipMemset(k->carry, 0, 256) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemset of the carried state");
    if (hipEventRecord(k->done, k->stream) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventRecord of the GenBank converter");
    guard.p = nullptr;
    *out = k;
    return KAIJU_GPU_OK;
  });
}

extern "C" void kaiju_gpu_gbk_free(kaiju_gpu_gbk *k) {
  if (!k) return;
  if (k->device >= 0 && hipSetDevice(k->device) == hipSuccess) {
    if (k->done) { (void)hipEventSynchronize(k->done); (void)hipEventDestroy(k->done); }
    if (k->stream) { (void)hipStreamSynchronize(k->stream); (void)hipStreamDestroy(k->stream); }
    for (hipEvent_t ev : k->ev) if (ev) (void)hipEventDestroy(ev);
    if (k->h_info) (void)hipHostFree(k->h_info);
    for (void *p : {(void *)k->carry, (void *)k->carry_tax, (void *)k->carry_pid}) if (p) (void)hipFree(p);
    k->mem.release(); k->text.release(); k->out.release(); k->info.release();
  }
  delete k;
}

// behind the last call, on the object's stream: nothing waits for the host
extern "C" int kaiju_gpu_gbk_reset(kaiju_gpu_gbk *k) {
  return guarded([&]() -> int {
    if (!k) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(k->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    if (hipStreamWaitEvent(k->stream, k->done, 0) != hipSuccess || hipMemsetAsync(k->carry, 0, sizeof(Carry), k->stream) != hipSuccess ||
        hipEventRecord(k->done, k->stream) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, "hipMemsetAsync of the carried state");
    return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_gbk_text_device(kaiju_gpu_gbk *k, const void *d_text, uint64_t bytes, void *d_out, uint64_t out_cap, kaiju_gpu_gbk_info *d_info,
                                         void *stream) {
  return guarded([&]() -> int {
    if (!k) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(k->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    return launch(k, stream ? static_cast<hipStream_t>(stream) : k->stream, d_text, bytes, d_out, out_cap, d_info);
  });
}

extern "C" int kaiju_gpu_gbk_text(kaiju_gpu_gbk *k, const char *text, uint64_t bytes, char *out, uint64_t out_cap, kaiju_gpu_gbk_info *info) {
  return guarded([&]() -> int {
    if (!k || !info || (!text && bytes) || (!out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (bytes > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
    if (hipSetDevice(k->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    const char *err = "";
    int rc;
    if ((rc = k->text.reserve(bytes + kChunk, 256, "hipMalloc of the GenBank converter's text", &err))) return fail(rc, err);
    if ((rc = k->out.reserve(out_cap + kChunk, 256, "hipMalloc of the GenBank converter's output", &err))) return fail(rc, err);
    if ((rc = k->info.reserve(sizeof(kaiju_gpu_gbk_info), 256, "hipMalloc of the GenBank converter's info", &err))) return fail(rc, err);
    const hipStream_t s = k->stream;
    if (bytes && hipMemcpyAsync(k->text.p, text, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the text");
    kaiju_gpu_gbk_info *d_info = static_cast<kaiju_gpu_gbk_info *>(k->info.p);
    if ((rc = launch(k, s, k->text.p, bytes, out_cap ? k->out.p : nullptr, out_cap, d_info))) return rc;
    if (hipMemcpyAsync(k->h_info, d_info, sizeof *info, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, std::string("the GenBank passes: ") + hipGetErrorString(hipGetLastError()));
    memcpy(info, k->h_info, sizeof *info);
    if (info->written_bytes > out_cap) return fail(KAIJU_GPU_ERR_HIP, "the GenBank passes wrote more than out_cap");
    if (info->written_bytes && hipMemcpy(out, k->out.p, info->written_bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the converted text");
    return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_gbk_pass_ms(kaiju_gpu_gbk *k, float *ms, uint32_t n) {
  return guarded([&]() -> int {
    if (!k || (!ms && n)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (!k->timed) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "the GenBank converter was created without KAIJU_GPU_CONVERT_TIMES=1");
    if (hipSetDevice(k->device) != hipSuccess || hipEventSynchronize(k->ev[KAIJU_GPU_GBK_PASSES]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventSynchronize");
    for (uint32_t p = 0; p < n && p < KAIJU_GPU_GBK_PASSES; p++)
      if (hipEventElapsedTime(&ms[p], k->ev[p], k->ev[p + 1]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventElapsedTime");
    return KAIJU_GPU_OK;
  });
}
