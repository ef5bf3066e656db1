// annotate.hip — kaiju-addTaxonNames on a text of output lines (gfx950, wave64): the passes of kj_annotate.h as kernels, and
// the entry points kaiju_gpu_annotator_* / kaiju_gpu_annotate_* of include/kaiju_gpu.h.  As in ingest.hip and format_names.hip
// the host never learns a count while the passes are queued: every kernel behind the first sizes itself from counts in device
// memory, and the scratch is sized for the worst case (a text of nothing but '\n': one line per byte).
//
//   k_an_init           counters
//   k_an_lines_count    '\n' per tile                          k_an_top   prefix sum over the tiles, one block
//   k_an_lines_fill     line_start[], the number of lines                                          (kj_ingest.h: lines)
//   k_an_len            per line: olen[], aslot[], the counts of the info
//   kjl::k_scan_sums / k_scan_top / k_scan_apply <AnCount>   out_off[] = prefix sum of olen[] (64 bit; kj_lines.h)
//   k_an_write          per lane 16 aligned bytes of the output: kjl::write_blocks over annotate_chunk
//   k_an_finish         kaiju_gpu_annotate_info, by one lane with ordinary stores
//
// Every loop is bounded by the data: the hash probe of kjn::find_slot ends at an empty slot (the table is at least half
// empty), the walks of kjn::locate end because the loader refuses cycles, everything else runs over bytes or lines of the text.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>

#include "../../include/kaiju_gpu.h"
#include "kj_annotate.h"
#include "kj_lines.h"

using namespace kja;
using kjs::OpAdd32;
using kjs::block_scan_excl;

extern "C" __attribute__((weak)) void kj_set_last_error(const char *msg);

struct kaiju_gpu_annotator {
  const kaiju_gpu_taxon_names *names = nullptr;
  int device = -1;
  kjl::Lines st;
  kjl::Scratch text, out, info;        // device staging of the host form
  void *h_info = nullptr;              // pinned
  void *h_text = nullptr, *h_out = nullptr;   // pinned staging of the host form, grown on demand
  size_t h_text_cap = 0, h_out_cap = 0;
  hipStream_t stream = nullptr;
};

namespace {

constexpr int kAnBlock = 256;
static_assert(kAnBlock == (int)kji::kTileLanes && kAnBlock == (int)kjf::kBlockLanes && kAnBlock == kjs::kScanLanes,
              "one lane per chunk of a tile / of a block of output / element of a scan block");

int fail(int code, const std::string &msg) {
  if (kj_set_last_error) kj_set_last_error(msg.c_str());
  return code;
}

struct AnHdr { uint64_t written; uint32_t n_lines; uint32_t count[kWhyCount]; };

struct AnJob {
  const uint8_t *text;
  uint64_t bytes;
  uint32_t n_tiles;
  uint8_t *out;
  uint64_t out_cap;
  kaiju_gpu_annotate_info *info;
  uint32_t *tile_cnt, *tile_base;      // n_tiles + 1
  uint32_t *line_start;                // bytes + 2
  uint32_t *aslot;                     // bytes + 1
  uint64_t *olen, *out_off;            // bytes + 1, bytes + 2
  uint64_t *oblk, *oblk_base;          // per block of kScanLanes lines (+ 1)
  AnHdr *hdr;
  int drop;
};

struct AnCount { const AnHdr *hdr; __device__ uint64_t operator()() const { return hdr->n_lines; } };   // elements of the scan

__global__ void k_an_init(AnHdr *h) {
  if (blockIdx.x || threadIdx.x) return;
  AnHdr z{};
  *h = z;
}

__global__ __launch_bounds__(kAnBlock) void k_an_lines_count(AnJob J) {
  const uint64_t c = (uint64_t)blockIdx.x * kji::kTileLanes + threadIdx.x;
  uint32_t tot;
  block_scan_excl<uint32_t>(kji::popc16(kji::nl_mask(J.text, J.bytes, c)), 0u, &tot, OpAdd32());
  if (threadIdx.x == 0) J.tile_cnt[blockIdx.x] = tot;
}

// out[i] = in[0] + .. + in[i - 1] for i <= n, by one block
__global__ __launch_bounds__(kAnBlock) void k_an_top(const uint32_t *in, uint32_t *out, uint32_t n) {
  uint32_t carry = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kAnBlock) {
    const uint32_t i = i0 + threadIdx.x;
    uint32_t tot;
    const uint32_t ex = block_scan_excl<uint32_t>(i < n ? in[i] : 0u, 0u, &tot, OpAdd32());
    if (i < n) out[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) out[n] = carry;
}

__global__ __launch_bounds__(kAnBlock) void k_an_lines_fill(AnJob J) {
  const uint64_t c = (uint64_t)blockIdx.x * kji::kTileLanes + threadIdx.x;
  const uint32_t m = kji::nl_mask(J.text, J.bytes, c);
  uint32_t tot;
  const uint32_t ex = block_scan_excl<uint32_t>(kji::popc16(m), 0u, &tot, OpAdd32());
  uint32_t j = J.tile_base[blockIdx.x] + ex;                       // the line that ends at the next '\n'
  for (uint32_t mm = m; mm; mm &= mm - 1, j++) J.line_start[j + 1] = (uint32_t)(c * kChunk + kji::ctz16(mm) + 1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    uint32_t sentinel;
    const uint32_t n_lines = kji::line_count(J.text, J.bytes, J.tile_base[J.n_tiles], &sentinel);
    J.line_start[0] = 0;
    J.line_start[n_lines] = sentinel;                              // (a text that ends in '\n': the value the last '\n' gives too)
    J.hdr->n_lines = n_lines;
  }
}

__global__ __launch_bounds__(kAnBlock) void k_an_len(AnJob J, Tab T) {
  const uint32_t n = J.hdr->n_lines;
  uint32_t cnt[kWhyCount];
#pragma unroll
  for (int w = 0; w < kWhyCount; w++) cnt[w] = 0;
  for (uint32_t r = blockIdx.x * kAnBlock + threadIdx.x; r < n; r += gridDim.x * kAnBlock) {
    uint32_t slot, why;
    J.olen[r] = line_out(J.text, J.line_start[r], kji::line_len(J.line_start, r), T, J.drop, &slot, &why);
    J.aslot[r] = slot;
#pragma unroll
    for (int w = 0; w < kWhyCount; w++) cnt[w] += why == (uint32_t)w ? 1u : 0u;
  }
#pragma unroll
  for (int w = 0; w < kWhyCount; w++) {
    uint32_t v = cnt[w];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&J.hdr->count[w], v);
  }
}

__global__ __launch_bounds__(kAnBlock) void k_an_write(AnJob J, Tab T) {
  kjl::write_blocks(J.out_off, J.hdr->n_lines, J.out, J.out_cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) {
    return annotate_chunk(c, J.text, J.line_start, J.out_off, J.aslot, T, lo, hi, total, J.out_cap, v);
  });
}

__global__ void k_an_finish(AnJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t n = J.hdr->n_lines;
  const uint64_t total = J.out_off[n];
  // the lines that fit: out_off[0 .. k] with out_off[k] <= out_cap
  J.hdr->written = total <= J.out_cap ? total : J.out_off[kjn::find_last_start(J.out_off, 0, n + 1, J.out_cap)];
  *J.info = make_info(total, n, J.hdr->count, J.out_cap);
}

// ---- host side: scratch and the queue of passes ----------------------------------------------------------------------
void carve(kjl::Carver &c, AnJob &J, uint64_t bytes) {
  J.n_tiles = (uint32_t)((bytes + kji::kTileBytes - 1) / kji::kTileBytes);
  const size_t nblk = (size_t)((bytes + 1) / kjs::kScanLanes + 2);
  J.tile_cnt = c.take<uint32_t>((size_t)J.n_tiles + 1);
  J.tile_base = c.take<uint32_t>((size_t)J.n_tiles + 1);
  J.line_start = c.take<uint32_t>(bytes + 2);
  J.aslot = c.take<uint32_t>(bytes + 1);
  J.olen = c.take<uint64_t>(bytes + 1);
  J.out_off = c.take<uint64_t>(bytes + 2);
  J.oblk = c.take<uint64_t>(nblk);
  J.oblk_base = c.take<uint64_t>(nblk + 1);
  J.hdr = c.take<AnHdr>(1);
}

// p is device memory of a device other than `device` (what the runtime does not know is taken as it is)
bool on_other_device(const void *p, int device) {
  hipPointerAttribute_t at;
  if (!p) return false;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeDevice && at.device != device;
}

int launch(kaiju_gpu_annotator *a, hipStream_t s, const void *d_text, uint64_t bytes, int drop, void *d_out, uint64_t out_cap,
           kaiju_gpu_annotate_info *d_info) {
  if (!d_info || (!d_text && bytes) || (!d_out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (bytes > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
  if (((uintptr_t)d_text | (uintptr_t)d_out) & (kChunk - 1)) return fail(KAIJU_GPU_ERR_ARG, "the text and the output pointer must be 16-byte aligned");
  if (on_other_device(d_text, a->device) || on_other_device(d_out, a->device)) return fail(KAIJU_GPU_ERR_ARG, "the text or the output lives on another device than the taxon names");
  AnJob J{};
  kjl::Carver measure{nullptr};
  carve(measure, J, bytes);
  const char *err = "";
  if (int rc = a->st.mem.reserve(measure.at, 256, "hipMalloc of the annotate scratch", &err)) return fail(rc, err);
  kjl::Carver c{static_cast<uint8_t *>(a->st.mem.p)};
  carve(c, J, bytes);
  a->st.total = nullptr;                                   // (out_off[n_lines]: n_lines is known on the device only)
  a->st.written = &J.hdr->written;
  J.text = static_cast<const uint8_t *>(d_text); J.bytes = bytes; J.out = static_cast<uint8_t *>(d_out); J.out_cap = out_cap;
  J.info = d_info; J.drop = drop ? 1 : 0;
  const Tab T = *kj_fn_tab(a->names);

  const dim3 blk(kAnBlock);
  // blocks for the passes over lines: how many there are is known on the device only
  const dim3 lgrid((unsigned)std::min<uint64_t>(4096, (bytes + 1) / kAnBlock + 1));
  const dim3 ogrid((unsigned)std::min<uint64_t>(2048, (bytes + 1) / kjs::kScanLanes + 1));
  const dim3 wgrid((unsigned)std::min<uint64_t>(8192, out_cap / kjf::kBlockBytes + 1));
  hipLaunchKernelGGL(k_an_init, dim3(1), dim3(64), 0, s, J.hdr);
  if (J.n_tiles) hipLaunchKernelGGL(k_an_lines_count, dim3(J.n_tiles), blk, 0, s, J);
  hipLaunchKernelGGL(k_an_top, dim3(1), blk, 0, s, J.tile_cnt, J.tile_base, J.n_tiles);
  hipLaunchKernelGGL(k_an_lines_fill, dim3(std::max(1u, J.n_tiles)), blk, 0, s, J);
  hipLaunchKernelGGL(k_an_len, lgrid, blk, 0, s, J, T);
  kjl::launch_offsets(s, ogrid, AnCount{J.hdr}, J.olen, J.oblk, J.oblk_base, J.out_off);
  hipLaunchKernelGGL(k_an_write, wgrid, blk, 0, s, J, T);
  hipLaunchKernelGGL(k_an_finish, dim3(1), dim3(64), 0, s, J);
  if (hipGetLastError() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "a kernel of the annotate passes could not be launched");
  return KAIJU_GPU_OK;
}

// pinned host memory of at least `bytes` bytes
int pinned(void **p, size_t *cap, size_t bytes) {
  if (bytes <= *cap) return KAIJU_GPU_OK;
  if (*p) { (void)hipHostFree(*p); *p = nullptr; *cap = 0; }
  const size_t want = bytes + bytes / 8 + 256;
  if (hipHostMalloc(p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return fail(KAIJU_GPU_ERR_NOMEM, "hipHostMalloc of the annotator's staging"); }
  *cap = want;
  return KAIJU_GPU_OK;
}

template <class F>
int guarded(F f) {
  try { return f(); }
  catch (const std::bad_alloc &) { return fail(KAIJU_GPU_ERR_NOMEM, "out of host memory"); }
}

}  // namespace

extern "C" int kaiju_gpu_annotator_create(const kaiju_gpu_taxon_names *names, kaiju_gpu_annotator **out) {
  return guarded([&]() -> int {
    if (!names || !out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    *out = nullptr;
    kaiju_gpu_annotator *a = new kaiju_gpu_annotator();
    a->names = names;
    a->device = kj_fn_device(names);
    if (hipSetDevice(a->device) != hipSuccess || hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc(&a->h_info, sizeof(kaiju_gpu_annotate_info) + 8, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      kaiju_gpu_annotator_free(a);
      return fail(KAIJU_GPU_ERR_HIP, "hipStreamCreate / hipHostMalloc of the annotator");
    }
    *out = a;
    return KAIJU_GPU_OK;
  });
}

extern "C" void kaiju_gpu_annotator_free(kaiju_gpu_annotator *a) {
  if (!a) return;
  if (a->device >= 0 && hipSetDevice(a->device) == hipSuccess) {
    if (a->stream) { (void)hipStreamSynchronize(a->stream); (void)hipStreamDestroy(a->stream); }
    if (a->h_info) (void)hipHostFree(a->h_info);
    if (a->h_text) (void)hipHostFree(a->h_text);
    if (a->h_out) (void)hipHostFree(a->h_out);
    a->st.release(); a->text.release(); a->out.release(); a->info.release();
  }
  delete a;
}

extern "C" int kaiju_gpu_annotate_text_device(kaiju_gpu_annotator *a, const void *d_text, uint64_t bytes, int drop_unclassified, void *d_out,
                                              uint64_t out_cap, kaiju_gpu_annotate_info *d_info, void *stream) {
  return guarded([&]() -> int {
    if (!a) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(a->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    return launch(a, stream ? static_cast<hipStream_t>(stream) : a->stream, d_text, bytes, drop_unclassified, d_out, out_cap, d_info);
  });
}

extern "C" int kaiju_gpu_annotate_text(kaiju_gpu_annotator *a, const char *text, uint64_t bytes, int drop_unclassified, char *out, uint64_t out_cap,
                                       kaiju_gpu_annotate_info *info) {
  return guarded([&]() -> int {
    if (!a || !info || (!text && bytes) || (!out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (bytes > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
    if (hipSetDevice(a->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    const char *err = "";
    int rc;
    if ((rc = a->text.reserve(bytes + kChunk, 256, "hipMalloc of the annotator's text", &err))) return fail(rc, err);
    if ((rc = a->out.reserve(out_cap + kChunk, 256, "hipMalloc of the annotator's output", &err))) return fail(rc, err);
    if ((rc = a->info.reserve(sizeof(kaiju_gpu_annotate_info) + 8, 256, "hipMalloc of the annotator's info", &err))) return fail(rc, err);
    if ((rc = pinned(&a->h_text, &a->h_text_cap, bytes)) || (rc = pinned(&a->h_out, &a->h_out_cap, out_cap))) return rc;
    const hipStream_t s = a->stream;
    if (bytes) memcpy(a->h_text, text, bytes);
    if (bytes && hipMemcpyAsync(a->text.p, a->h_text, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the text");
    kaiju_gpu_annotate_info *d_info = static_cast<kaiju_gpu_annotate_info *>(a->info.p);
    if ((rc = launch(a, s, a->text.p, bytes, drop_unclassified, a->out.p, out_cap, d_info))) return rc;
    // the info and, behind it, the number of bytes written
    uint8_t *h = static_cast<uint8_t *>(a->h_info);
    if (hipMemcpyAsync(h, d_info, sizeof *info, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(h + sizeof *info, a->st.written, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, std::string("the annotate passes: ") + hipGetErrorString(hipGetLastError()));
    memcpy(info, h, sizeof *info);
    uint64_t written;
    memcpy(&written, h + sizeof *info, 8);
    if (written > out_cap) return fail(KAIJU_GPU_ERR_HIP, "the annotate passes wrote more than out_cap");
    if (written && (hipMemcpyAsync(a->h_out, a->out.p, written, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess))
      return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the annotated text");
    if (written) memcpy(out, a->h_out, written);
    return KAIJU_GPU_OK;
  });
}

extern "C" uint64_t kaiju_gpu_annotate_bound(uint64_t bytes, uint64_t n_lines, const kaiju_gpu_taxon_names *names) {
  return bound(bytes, n_lines, names ? kaiju_gpu_taxon_names_max_annotation(names) : 0);
}
