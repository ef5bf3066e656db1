// format_names.hip — the lines of format.hip with the column of kaiju-addTaxonNames (gfx950, wave64): the tables of
// kj_format_names.h on the device, and its passes as kernels.  As in format.hip every kernel behind the first sizes itself
// from counts in device memory and nothing waits for the host.
//
//   k_fn_tables         at upload, one lane per slot: path_len[] (path mode) or rank_src[] / rank_len[] (ranks mode), and the
//                       largest annotation of any slot
//   k_fn_len            per record: the decision, the slot whose annotation the line carries, the length of the line (0: no
//                       line); the counts of the info
//   kjl::k_scan_sums / k_scan_top / k_scan_apply <FnCount>   line_off[] = prefix sum of the lengths (64 bit; kj_lines.h)
//   k_fn_write          per lane 16 aligned bytes of the output: kjl::write_blocks over format_chunk
//   k_fn_finish         kaiju_gpu_format_names_info, by one lane with ordinary stores
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/kaiju_gpu.h"
#include "kj_format_names.h"
#include "kj_lines.h"
#include "taxon_names.h"

using namespace kjn;

extern "C" __attribute__((weak)) void kj_set_last_error(const char *msg);

struct kaiju_gpu_taxon_names {
  int device = -1;
  Tab tab{};
  uint32_t cap = 0;
  uint64_t max_annotation = 0;
  kaiju_krona_source krona;            // host side, for krona.hip
  std::vector<void *> allocs;
  ~kaiju_gpu_taxon_names() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    for (void *p : allocs) (void)hipFree(p);
  }
};

namespace {

constexpr int kFnBlock = 256;
static_assert(kFnBlock == (int)kBlockLanes && kFnBlock == (int)kScanBlock && kFnBlock == kjs::kScanLanes,
              "one lane per chunk of a block of output / element of a scan block");

int fail(int code, const std::string &msg) {
  if (kj_set_last_error) kj_set_last_error(msg.c_str());
  return code;
}

// ---- the tables ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFnBlock) void k_fn_tables(Tab T, uint32_t cap, uint32_t *path_len, uint32_t *rank_src, uint32_t *rank_len,
                                                        unsigned long long *max_annotation) {
  unsigned long long most = 0;
  for (uint32_t s = blockIdx.x * kFnBlock + threadIdx.x; s < cap; s += gridDim.x * kFnBlock) {
    uint64_t len = 0;
    if (T.mode == KAIJU_NAMES_PATH) {
      len = build_path_len(T, s);
      path_len[s] = clamp32(len);
    } else if (T.mode == KAIJU_NAMES_RANKS) {
      len = build_ranks(T, s, rank_src + (uint64_t)s * T.n_ranks);
      rank_len[s] = clamp32(len);
    } else if (T.key[s] != ~0ull && !(T.name_len[s] & kGenerated)) {
      len = T.name_len[s];
    }
    most = len > most ? len : most;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_xor(most, d, 64);
    most = o > most ? o : most;
  }
  if ((threadIdx.x & 63) == 0 && most) atomicMax(max_annotation, most);
}

// ---- the passes ---------------------------------------------------------------------------------------------------
struct FnHdr { uint64_t written; uint32_t n, n_classified, n_inexact, n_unknown, n_unnamed, n_dropped; };

struct FnJob {
  Params P;
  const double *pw;
  const kaiju_gpu_compact *recs;
  const uint64_t *off;
  const uint8_t *text;
  uint64_t bytes1;
  const kaiju_gpu_name_span *names;
  uint8_t *out;
  uint64_t out_cap;
  kaiju_gpu_format_names_info *info;
  uint32_t *llen, *aslot;              // n
  uint64_t *line_off, *tax;            // n + 1, n
  uint64_t *oblk, *oblk_base;          // per block of kScanBlock records (+ 1)
  FnHdr *hdr;
  int drop;
};

struct FnCount { const FnHdr *hdr; __device__ uint64_t operator()() const { return hdr->n; } };   // elements of the scan

__global__ void k_fn_init(FnHdr *h, uint32_t n) {
  if (blockIdx.x || threadIdx.x) return;
  *h = FnHdr{0, n, 0, 0, 0, 0, 0};
}

__global__ __launch_bounds__(kFnBlock) void k_fn_len(FnJob J, Tab T, uint32_t n) {
  uint32_t nc = 0, ni = 0, nk = 0, nu = 0, nd = 0;
  for (uint32_t r = blockIdx.x * kFnBlock + threadIdx.x; r < n; r += gridDim.x * kFnBlock) {
    uint64_t t;
    uint32_t slot, why;
    J.llen[r] = record_line(J.recs, J.off, J.names, r, J.bytes1, J.P, J.pw, T, J.drop, &t, &slot, &why);
    J.tax[r] = t;
    J.aslot[r] = slot;
    nc += t ? 1u : 0u;
    ni += (J.recs[r].info & KAIJU_HIT_INEXACT) ? 1u : 0u;
    nk += why == kWhyUnknown ? 1u : 0u;
    nu += why == kWhyUnnamed ? 1u : 0u;
    nd += why == kWhyDropped ? 1u : 0u;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    nc += __shfl_xor(nc, d, 64); ni += __shfl_xor(ni, d, 64); nk += __shfl_xor(nk, d, 64); nu += __shfl_xor(nu, d, 64); nd += __shfl_xor(nd, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (nc) atomicAdd(&J.hdr->n_classified, nc);
    if (ni) atomicAdd(&J.hdr->n_inexact, ni);
    if (nk) atomicAdd(&J.hdr->n_unknown, nk);
    if (nu) atomicAdd(&J.hdr->n_unnamed, nu);
    if (nd) atomicAdd(&J.hdr->n_dropped, nd);
  }
}

__global__ __launch_bounds__(kFnBlock) void k_fn_write(FnJob J, Tab T) {
  kjl::write_blocks(J.line_off, J.hdr->n, J.out, J.out_cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) {
    return format_chunk(c, J.text, J.bytes1, J.names, J.line_off, J.tax, J.aslot, T, lo, hi, total, J.out_cap, v);
  });
}

__global__ void k_fn_finish(FnJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t n = J.hdr->n;
  const uint64_t total = J.line_off[n];
  // the lines that fit: line_off[0 .. k] with line_off[k] <= out_cap
  J.hdr->written = total <= J.out_cap ? total : J.line_off[find_last_start(J.line_off, 0, n + 1, J.out_cap)];
  *J.info = make_info(total, n, J.hdr->n_classified, J.hdr->n_inexact, J.out_cap, J.hdr->n_unknown, J.hdr->n_unnamed, J.hdr->n_dropped);
}

}  // namespace

// ---- the tables on a device -----------------------------------------------------------------------------------------
extern "C" int kaiju_gpu_taxon_names_upload(const kaiju_taxon_names *names, int device_id, kaiju_gpu_taxon_names **out) {
  try {
    if (!names || !out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(KAIJU_GPU_ERR_NO_DEVICE, "hipGetDeviceCount found no device"); }
    if (device_id < 0 || device_id >= ndev) return fail(KAIJU_GPU_ERR_ARG, "device_id out of range");
    const uint32_t cap = (uint32_t)names->key.size();
    if (cap == 0 || (cap & (cap - 1))) return fail(KAIJU_GPU_ERR_ARG, "the table's size is no power of two");
    std::unique_ptr<kaiju_gpu_taxon_names> g(new kaiju_gpu_taxon_names());
    if (hipSetDevice(device_id) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    g->device = device_id;
    g->cap = cap;
    auto alloc = [&](size_t bytes) -> void * {
      void *p = nullptr;
      if (hipMalloc(&p, bytes + 16) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
      g->allocs.push_back(p);
      return p;
    };
    bool ok = true;
    auto up = [&](const void *src, size_t bytes) -> const void * {
      void *p = alloc(bytes);
      if (!p || (bytes && hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess)) { ok = false; return nullptr; }
      return p;
    };
    Tab &T = g->tab;
    T.key = static_cast<const uint64_t *>(up(names->key.data(), (size_t)cap * 8));
    T.parent = static_cast<const uint32_t *>(up(names->parent.data(), (size_t)cap * 4));
    T.name_pos = static_cast<const uint32_t *>(up(names->name_pos.data(), (size_t)cap * 4));
    T.name_len = static_cast<const uint32_t *>(up(names->name_len.data(), (size_t)cap * 4));
    T.rank = static_cast<const uint8_t *>(up(names->rank.data(), (size_t)cap));
    T.blob = static_cast<const uint8_t *>(up(names->blob.data(), names->blob.size()));
    T.cap_mask = cap - 1;
    T.mode = (uint32_t)names->mode;
    T.n_ranks = (uint32_t)names->ranks.size();
    T.n_list = (uint32_t)names->list.size();
    if (T.n_ranks > kMaxRanks || T.n_list > kMaxList) return fail(KAIJU_GPU_ERR_ARG, "too many ranks");
    for (uint32_t j = 0; j < T.n_list; j++) T.list[j] = names->list[j];
    uint32_t *path_len = nullptr, *rank_src = nullptr, *rank_len = nullptr;
    if (T.mode == KAIJU_NAMES_PATH) path_len = static_cast<uint32_t *>(alloc((size_t)cap * 4));
    if (T.mode == KAIJU_NAMES_RANKS) {
      rank_src = static_cast<uint32_t *>(alloc((size_t)cap * 4 * std::max(1u, T.n_ranks)));
      rank_len = static_cast<uint32_t *>(alloc((size_t)cap * 4));
    }
    unsigned long long *d_max = static_cast<unsigned long long *>(alloc(8));
    if (!ok || !d_max || (T.mode == KAIJU_NAMES_PATH && !path_len) || (T.mode == KAIJU_NAMES_RANKS && (!rank_src || !rank_len)))
      return fail(KAIJU_GPU_ERR_NOMEM, "hipMalloc / hipMemcpy of the name tables");
    if (hipMemset(d_max, 0, 8) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemset");
    hipLaunchKernelGGL(k_fn_tables, dim3(std::min<uint32_t>(4096, cap / kFnBlock + 1)), dim3(kFnBlock), 0, 0, T, cap, path_len, rank_src, rank_len, d_max);
    unsigned long long most = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpy(&most, d_max, 8, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, "the kernel that builds the name tables");
    T.path_len = path_len; T.rank_src = rank_src; T.rank_len = rank_len;
    g->max_annotation = most;
    g->krona = kaiju_krona_source{names->rank_names, names->rank_of, names->dang_pos, names->dang_len, names->dang_blob};
    if (most >= kMaxAnnotation) return fail(KAIJU_GPU_ERR_ARG, "an annotation of " + std::to_string(most) + " bytes: 2^24 or more");
    *out = g.release();
    return KAIJU_GPU_OK;
  } catch (const std::bad_alloc &) { return fail(KAIJU_GPU_ERR_NOMEM, "out of host memory"); }
}

extern "C" void kaiju_gpu_taxon_names_free(kaiju_gpu_taxon_names *names) { delete names; }
extern "C" uint64_t kaiju_gpu_taxon_names_max_annotation(const kaiju_gpu_taxon_names *names) { return names ? names->max_annotation : 0; }
int kj_fn_device(const kaiju_gpu_taxon_names *names) { return names ? names->device : -1; }
const kjn::Tab *kj_fn_tab(const kaiju_gpu_taxon_names *names) { return names ? &names->tab : nullptr; }   // (for annotate.hip)
const kaiju_krona_source *kj_fn_krona_source(const kaiju_gpu_taxon_names *names) { return names ? &names->krona : nullptr; }   // (for krona.hip)

extern "C" int kaiju_gpu_taxon_names_read(const kaiju_gpu_taxon_names *names, int which, void *host_out, uint64_t out_bytes, uint64_t *n_slots) {
  if (!names || (!host_out && out_bytes)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  const Tab &T = names->tab;
  const void *src[8] = {T.key, T.parent, T.name_pos, T.name_len, T.path_len, T.rank_len, T.rank_src, T.rank};
  const uint64_t width[8] = {8, 4, 4, 4, 4, 4, 4ull * T.n_ranks, 1};
  if (which < 0 || which > 7 || !src[which]) return fail(KAIJU_GPU_ERR_ARG, "no such table in this mode");
  if (n_slots) *n_slots = names->cap;
  const uint64_t bytes = std::min<uint64_t>(out_bytes, width[which] * names->cap);
  if (hipSetDevice(names->device) != hipSuccess || (bytes && hipMemcpy(host_out, src[which], bytes, hipMemcpyDeviceToHost) != hipSuccess))
    return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of a name table");
  return KAIJU_GPU_OK;
}

// ---- host side: scratch and the queue of passes ----------------------------------------------------------------------
namespace {
void carve(kjl::Carver &c, FnJob &J, uint32_t n) {
  const size_t nblk = (size_t)n / kScanBlock + 2;
  J.llen = c.take<uint32_t>((size_t)n + 1);
  J.aslot = c.take<uint32_t>((size_t)n + 1);
  J.line_off = c.take<uint64_t>((size_t)n + 1);
  J.tax = c.take<uint64_t>((size_t)n + 1);
  J.oblk = c.take<uint64_t>(nblk);
  J.oblk_base = c.take<uint64_t>(nblk + 1);
  J.hdr = c.take<FnHdr>(1);
}
}  // namespace

int kj_fn_launch(kjl::Lines &st, hipStream_t s, const Params &P, const double *d_pw, const kaiju_gpu_compact *d_recs, const uint64_t *d_off,
                 uint32_t n, const void *d_text1, uint64_t bytes1, const kaiju_gpu_name_span *d_names, const kaiju_gpu_taxon_names *names,
                 int drop_unclassified, void *d_out, uint64_t out_cap, kaiju_gpu_format_names_info *d_info, const char **err) {
  *err = "";
  if (!d_info || !d_pw || !names || (n && (!d_recs || !d_off || !d_names)) || (!d_text1 && bytes1) || (!d_out && out_cap)) {
    *err = "NULL argument";
    return KAIJU_GPU_ERR_ARG;
  }
  // (a line is at most its name, 25 bytes and an annotation below 2^24: its length fits 32 bits)
  if (bytes1 > kjf::kMaxBytes - kMaxAnnotation || n > kjf::kMaxRecords) { *err = "a block of text must be below 2^32 - 2^24 - 32 bytes, a batch below 2^31 records"; return KAIJU_GPU_ERR_ARG; }
  if ((uintptr_t)d_out & (kChunk - 1)) { *err = "the output pointer must be 16-byte aligned"; return KAIJU_GPU_ERR_ARG; }
  FnJob J{};
  kjl::Carver measure{nullptr};
  carve(measure, J, n);
  if (int rc = st.mem.reserve(measure.at, 256, "hipMalloc of the format scratch", err)) return rc;
  kjl::Carver c{static_cast<uint8_t *>(st.mem.p)};
  carve(c, J, n);
  st.total = J.line_off + n;
  st.written = &J.hdr->written;
  J.P = P; J.pw = d_pw; J.recs = d_recs; J.off = d_off; J.text = static_cast<const uint8_t *>(d_text1); J.bytes1 = bytes1;
  J.names = d_names; J.out = static_cast<uint8_t *>(d_out); J.out_cap = out_cap; J.info = d_info; J.drop = drop_unclassified ? 1 : 0;
  const Tab &T = names->tab;

  const dim3 blk(kFnBlock);
  const dim3 rgrid((unsigned)std::min<uint64_t>(4096, (uint64_t)n / kFnBlock + 1));
  const dim3 ogrid((unsigned)std::min<uint64_t>(2048, (uint64_t)n / kScanBlock + 1));
  // blocks of the write pass: how many bytes there are is known on the device only
  const uint64_t most = std::min<uint64_t>(out_cap, bytes1 + ((uint64_t)kNamesExtra + names->max_annotation) * n);
  const dim3 wgrid((unsigned)std::min<uint64_t>(8192, most / kBlockBytes + 1));
  hipLaunchKernelGGL(k_fn_init, dim3(1), dim3(64), 0, s, J.hdr, n);
  hipLaunchKernelGGL(k_fn_len, rgrid, blk, 0, s, J, T, n);
  kjl::launch_offsets(s, ogrid, FnCount{J.hdr}, J.llen, J.oblk, J.oblk_base, J.line_off);
  hipLaunchKernelGGL(k_fn_write, wgrid, blk, 0, s, J, T);
  hipLaunchKernelGGL(k_fn_finish, dim3(1), dim3(64), 0, s, J);
  if (hipGetLastError() != hipSuccess) { *err = "a kernel of the format passes could not be launched"; return KAIJU_GPU_ERR_HIP; }
  return KAIJU_GPU_OK;
}
