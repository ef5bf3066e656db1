// convert.hip — kaiju-convertNR and kaiju-convertRefSeq on a block of FASTA text (gfx950, wave64): the passes of kj_convert.h as
// kernels, and the entry points kaiju_gpu_converter_* / kaiju_gpu_convert_* of include/kaiju_gpu.h.  The host never learns a count while the
// passes are queued: every kernel behind the first sizes itself from counts in device memory.
//
// at create   k_cv_listed / k_cv_keep   per slot of the tree: is it on the include list; does the include walk from it keep
// per call    k_cv_init        the counters
//             k_tl_*           the lines                                                              (kj_textlines.h)
//             k_cv_kinds       one lane per line: header or not
//             kjl::k_scan_* <CvLines>   hdr_pos[] = headers in front of a line: the record numbers     (kj_lines.h)
//             k_cv_records     one lane per line: rec_line[] and the start values of a record's reduction
//             k_cv_entries     one lane per 16 bytes of text: the entries that start in them, the lookups in both maps, the
//                              record's reduction with atomics (LCA by compare-and-swap, excluded, first accession)
//             k_cv_first       in its place under the RefSeq rules: one lane per record, the header read in 16-byte chunks up
//                              to its first space, one lookup, plain stores
//             k_cv_decide      one lane per record: the taxon or the reason it is dropped
//             k_cv_len         one lane per line: the bytes it gives to the output
//             kjl::k_scan_* <CvLines>   line_off[]
//             k_cv_write       per lane 16 aligned bytes of the output: kjl::write_blocks over convert_chunk
//             k_cv_finish      kaiju_gpu_convert_info, by one lane
//
// Every loop is bounded by the data: the probes of kjc::map_find by the slots of the map, the walks of lca_pair and
// include_walk by the depth stored with a slot, the compare-and-swap of a record's LCA ends because one lane of those that
// compete always succeeds, everything else runs over bytes, lines or records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "kj_convert.h"
#include "kj_lines.h"
#include "kj_textlines.h"

using namespace kjc;

typedef unsigned long long cv_u64;

namespace {

constexpr int kCvBlock = 256;
static_assert(kCvBlock == (int)kjf::kBlockLanes && kCvBlock == kjs::kScanLanes, "one lane per chunk of a block of output / element of a scan block");

struct CvHdr {
  uint64_t n_entries, n_hits, written;
  uint64_t kept, excluded, no_taxon, not_included, no_lca;
};

struct CvJob {
  TlText t;
  uint8_t *is_header;                  // per line
  uint64_t *hdr_pos;                   // lines + 1
  uint32_t *olen;                      // per line
  uint64_t *line_off;                  // lines + 1
  uint64_t *blk, *blk_base;
  uint32_t *rec_line, *rec_lca, *rec_flags, *rec_first;   // per record (+ 1)
  uint64_t *rec_taxon;
  CvHdr *hdr;
  uint8_t *out;
  uint64_t out_cap;
  kaiju_gpu_convert_info *info;
  int add_acc;
};

struct CvLines { const uint32_t *n; __device__ uint64_t operator()() const { return *n; } };

void carve(kjl::Carver &c, CvJob &J) {
  tl_carve(c, J.t);
  const size_t lines = J.t.bytes + 1, recs = J.t.bytes / 2 + 2, nblk = lines / kjs::kScanLanes + 2;   // (a header line has two bytes at least, or is the last)
  J.is_header = c.take<uint8_t>(lines);
  J.hdr_pos = c.take<uint64_t>(lines + 1);
  J.olen = c.take<uint32_t>(lines);
  J.line_off = c.take<uint64_t>(lines + 1);
  J.blk = c.take<uint64_t>(nblk);
  J.blk_base = c.take<uint64_t>(nblk + 1);
  J.rec_line = c.take<uint32_t>(recs + 1);
  J.rec_lca = c.take<uint32_t>(recs);
  J.rec_flags = c.take<uint32_t>(recs);
  J.rec_first = c.take<uint32_t>(recs);
  J.rec_taxon = c.take<uint64_t>(recs);
  J.hdr = c.take<CvHdr>(1);
}

__device__ __forceinline__ View view_of(const CvJob &J) {
  const uint32_t n = *J.t.n_lines;
  return View{J.t.text, J.t.line_start, J.is_header, J.hdr_pos, J.rec_line, J.rec_taxon, J.rec_first, n, (uint32_t)J.hdr_pos[n], J.add_acc};
}

__global__ __launch_bounds__(kCvBlock) void k_cv_listed(Tree T, const uint64_t *ids, uint32_t n, uint8_t *listed) {
  for (uint32_t i = blockIdx.x * kCvBlock + threadIdx.x; i < n; i += gridDim.x * kCvBlock) {
    const uint32_t s = kjm::find_slot(T, ids[i]);
    if (s != kNoSlot) listed[s] = 1;
  }
}
__global__ __launch_bounds__(kCvBlock) void k_cv_keep(Tree T, const uint8_t *listed, uint8_t *keep) {
  for (uint32_t s = blockIdx.x * kCvBlock + threadIdx.x; s <= T.cap_mask; s += gridDim.x * kCvBlock) keep[s] = T.key[s] == ~0ull ? 0 : include_walk(T, listed, s);
}

__global__ void k_cv_init(CvHdr *h) {
  if (blockIdx.x || threadIdx.x) return;
  *h = CvHdr{};
}

__global__ __launch_bounds__(kCvBlock) void k_cv_kinds(CvJob J) {
  const uint32_t n = *J.t.n_lines;
  for (uint32_t i = blockIdx.x * kCvBlock + threadIdx.x; i < n; i += gridDim.x * kCvBlock)
    J.is_header[i] = kji::line_len(J.t.line_start, i) > 0 && J.t.text[J.t.line_start[i]] == '>';
}

__global__ __launch_bounds__(kCvBlock) void k_cv_records(CvJob J) {
  const uint32_t n = *J.t.n_lines;
  for (uint32_t i = blockIdx.x * kCvBlock + threadIdx.x; i < n; i += gridDim.x * kCvBlock) {
    if (!J.is_header[i]) continue;
    const uint64_t r = J.hdr_pos[i];
    J.rec_line[r] = i; J.rec_lca[r] = kNone; J.rec_flags[r] = 0; J.rec_first[r] = kNone;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) J.rec_line[J.hdr_pos[n]] = n;
}

// the taxon's slot joins the LCA of record r
__device__ void join_lca(const CvJob &J, const Tree &T, uint32_t r, uint32_t slot) {
  uint32_t cur = __hip_atomic_load(&J.rec_lca[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {                                                   // (a failed compare-and-swap means another lane's succeeded)
    const uint32_t next = cur == kNone ? slot : lca_pair(T, cur, slot);
    if (next == kNoSlot) { atomicOr(&J.rec_flags[r], kFlagNoLca); return; }
    if (next == cur) return;
    const uint32_t seen = atomicCAS(&J.rec_lca[r], cur, next);
    if (seen == cur) return;
    cur = seen;
  }
}

__global__ __launch_bounds__(kCvBlock) void k_cv_entries(CvJob J, Tree T, Map M, Map X) {
  const uint32_t n = *J.t.n_lines;
  const uint64_t bytes = J.t.bytes, n_chunks = (bytes + kChunk - 1) / kChunk;
  cv_u64 entries = 0, hits = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * kCvBlock + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * kCvBlock) {
    const kji::Chunk v = kji::load_chunk(J.t.text, c);
    uint32_t m = (kji::eq_mask(v, 1) | kji::eq_mask(v, '>')) & kji::range_mask(c * kChunk, 0, bytes);
    if (!m) continue;
    // the line of the chunk's first mark: the largest i with line_start[i] <= p
    uint32_t lo = 0, hi = n;
    const uint64_t p0 = c * kChunk + kji::ctz16(m);
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (J.t.line_start[mid] <= p0) lo = mid; else hi = mid; }
    uint32_t i = lo;
    for (; m; m &= m - 1) {
      const uint64_t p = c * kChunk + kji::ctz16(m);
      while (i + 1 < n && J.t.line_start[i + 1] <= p) i++;
      const uint64_t a = J.t.line_start[i], e = (uint64_t)J.t.line_start[i + 1] - 1;
      if (!J.is_header[i] || p >= e) continue;
      if (J.t.text[p] == '>' && p != a) continue;             // ('>' is a mark as byte 0 only)
      uint64_t acc_end;
      if (!entry_at(J.t.text, a, e, p, &acc_end)) continue;
      entries++;
      const uint32_t r = (uint32_t)J.hdr_pos[i];
      const uint8_t *key = J.t.text + p + 1;
      const uint32_t len = (uint32_t)(acc_end - p - 1);
      uint32_t probes;
      if (map_find(X, key, len, &probes)) atomicOr(&J.rec_flags[r], kFlagExcluded);
      const uint8_t *ent = map_find(M, key, len, &probes);
      if (!ent || entry_taxon(ent) == 0) continue;
      const uint32_t slot = kjm::find_slot(T, entry_taxon(ent));
      if (slot == kNoSlot) continue;                           // (the map holds nodes only)
      hits++;
      atomicMin(&J.rec_first[r], (uint32_t)(p + 1));
      join_lca(J, T, r, slot);
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { entries += __shfl_xor(entries, d, 64); hits += __shfl_xor(hits, d, 64); }
  if ((threadIdx.x & 63) == 0 && entries) {
    atomicAdd(reinterpret_cast<cv_u64 *>(&J.hdr->n_entries), entries);
    atomicAdd(reinterpret_cast<cv_u64 *>(&J.hdr->n_hits), hits);
  }
}

// The RefSeq rules: one accession at the front of each header.  One lane per record and no atomics on the records: the lane
// owns rec_lca, rec_flags and rec_first of its record.  What a lane waits for is a chain of dependent loads (rec_line,
// line_start, the header's chunks, the slot of the map, the entry, the slot of the tree) and nothing else: no LDS, few
// registers, so blocks of 256 lanes fill a CU with its 32 wavefronts and the chains of that many records overlap.
__global__ __launch_bounds__(kCvBlock) void k_cv_first(CvJob J, Tree T, Map M) {
  const uint32_t n = *J.t.n_lines, n_rec = (uint32_t)J.hdr_pos[n];
  cv_u64 entries = 0, hits = 0;
  for (uint32_t r = blockIdx.x * kCvBlock + threadIdx.x; r < n_rec; r += gridDim.x * kCvBlock) {
    const uint32_t i = J.rec_line[r];
    const First F = first_entry(J.t.text, J.t.line_start[i], (uint64_t)J.t.line_start[i + 1] - 1, M, T);
    J.rec_lca[r] = F.slot; J.rec_first[r] = F.first; J.rec_flags[r] = 0;
    entries += F.entry; hits += F.hit;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { entries += __shfl_xor(entries, d, 64); hits += __shfl_xor(hits, d, 64); }
  if ((threadIdx.x & 63) == 0 && entries) {
    atomicAdd(reinterpret_cast<cv_u64 *>(&J.hdr->n_entries), entries);
    atomicAdd(reinterpret_cast<cv_u64 *>(&J.hdr->n_hits), hits);
  }
}

__global__ __launch_bounds__(kCvBlock) void k_cv_decide(CvJob J, Tree T, const uint8_t *keep) {
  const uint32_t n = *J.t.n_lines, n_rec = (uint32_t)J.hdr_pos[n];
  cv_u64 cnt[5] = {0, 0, 0, 0, 0};                            // kept, excluded, no taxon, not included, no lca
  for (uint32_t r = blockIdx.x * kCvBlock + threadIdx.x; r < n_rec; r += gridDim.x * kCvBlock) {
    const uint32_t flags = J.rec_flags[r], s = J.rec_lca[r];
    uint64_t taxon = 0;
    if (flags & kFlagExcluded) cnt[1]++;
    else if (s == kNone) cnt[2]++;
    else if (flags & kFlagNoLca) cnt[4]++;
    else if (!keep[s]) cnt[3]++;
    else { taxon = T.key[s]; cnt[0]++; }
    J.rec_taxon[r] = taxon;
  }
#pragma unroll
  for (int w = 0; w < 5; w++) {
    cv_u64 v = cnt[w];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(reinterpret_cast<cv_u64 *>(&J.hdr->kept) + w, v);
  }
}

__global__ __launch_bounds__(kCvBlock) void k_cv_len(CvJob J) {
  const View V = view_of(J);
  for (uint32_t i = blockIdx.x * kCvBlock + threadIdx.x; i < V.n_lines; i += gridDim.x * kCvBlock) J.olen[i] = line_out_len(V, i);
}

__global__ __launch_bounds__(kCvBlock) void k_cv_write(CvJob J) {
  const View V = view_of(J);
  kjl::write_blocks(J.line_off, V.n_lines, J.out, J.out_cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) {
    return convert_chunk(c, V, J.line_off, lo, hi, total, J.out_cap, v);
  });
}

__global__ void k_cv_finish(CvJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const View V = view_of(J);
  const CvHdr &H = *J.hdr;
  kaiju_gpu_convert_info o{};
  o.text_bytes = J.line_off[V.n_lines];
  o.written_bytes = written_bytes(V, J.line_off, J.out_cap);
  o.n_records = V.n_records; o.n_kept = H.kept;
  o.dropped_excluded = H.excluded; o.dropped_no_taxon = H.no_taxon; o.dropped_not_included = H.not_included; o.dropped_no_lca = H.no_lca;
  o.n_entries = H.n_entries; o.n_hits = H.n_hits;
  o.n_lines = V.n_lines;
  o.overflow = o.text_bytes > J.out_cap ? 1u : 0u;
  J.hdr->written = o.written_bytes;
  *J.info = o;
}

bool on_other_device(const void *p, int device) {
  hipPointerAttribute_t at;
  if (!p) return false;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeDevice && at.device != device;
}

}  // namespace

struct kaiju_gpu_converter {
  int device = -1;
  const kaiju_gpu_taxonomy *tax = nullptr;
  const kaiju_gpu_accmap *map = nullptr, *excluded = nullptr;
  int add_acc = 0, rules = kRulesNr;
  Tree tree{};
  uint8_t *listed = nullptr, *keep = nullptr;
  uint64_t *d_ids = nullptr;
  kjl::Scratch mem, text, out, info;
  void *h_info = nullptr;              // pinned
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;           // behind the last call, on whichever stream it ran
  bool timed = false;
  hipEvent_t ev[KAIJU_GPU_CONVERT_PASSES + 1] = {};
};

namespace {

int launch(kaiju_gpu_converter *k, hipStream_t s, const void *d_text, uint64_t bytes, void *d_out, uint64_t out_cap, kaiju_gpu_convert_info *d_info) {
  if (!d_info || (!d_text && bytes) || (!d_out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (bytes > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
  if (((uintptr_t)d_text | (uintptr_t)d_out) & (kChunk - 1)) return fail(KAIJU_GPU_ERR_ARG, "the text and the output pointer must be 16-byte aligned");
  if (on_other_device(d_text, k->device) || on_other_device(d_out, k->device) || on_other_device(d_info, k->device))
    return fail(KAIJU_GPU_ERR_ARG, "the text, the output or the info lives on another device than the converter");
  CvJob J{};
  J.t.text = static_cast<const uint8_t *>(d_text); J.t.bytes = bytes;
  kjl::Carver measure{nullptr};
  carve(measure, J);
  const char *err = "";
  if (int rc = k->mem.reserve(measure.at, 256, "hipMalloc of the converter's scratch", &err)) return fail(rc, err);
  kjl::Carver c{static_cast<uint8_t *>(k->mem.p)};
  carve(c, J);
  J.out = static_cast<uint8_t *>(d_out); J.out_cap = out_cap; J.info = d_info; J.add_acc = k->add_acc;
  const Map M = kj_accmap_view(k->map, nullptr, nullptr);
  const Map X = k->excluded ? kj_accmap_view(k->excluded, nullptr, nullptr) : Map{nullptr, 0, nullptr};

  const dim3 blk(kCvBlock);
  const dim3 lgrid((unsigned)std::min<uint64_t>(4096, bytes / (4 * kCvBlock) + 1));       // passes over lines or records
  const dim3 cgrid((unsigned)std::min<uint64_t>(8192, bytes / kji::kTileBytes + 1));      // ... over the chunks of the text
  const dim3 sgrid((unsigned)std::min<uint64_t>(2048, (bytes + 1) / kjs::kScanLanes + 1));
  const dim3 wgrid((unsigned)std::min<uint64_t>(8192, out_cap / kjf::kBlockBytes + 1));
  const CvLines count{J.t.n_lines};
  int mark = 0;
  auto passed = [&]() { if (k->timed) (void)hipEventRecord(k->ev[mark++], s); };
  if (hipStreamWaitEvent(s, k->done, 0) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipStreamWaitEvent of the converter");
  passed();
  hipLaunchKernelGGL(k_cv_init, dim3(1), dim3(64), 0, s, J.hdr);
  tl_launch(s, J.t);
  passed();
  hipLaunchKernelGGL(k_cv_kinds, lgrid, blk, 0, s, J);
  kjl::launch_offsets(s, sgrid, count, static_cast<const uint8_t *>(J.is_header), J.blk, J.blk_base, J.hdr_pos);
  hipLaunchKernelGGL(k_cv_records, lgrid, blk, 0, s, J);
  passed();
  if (k->rules == kRulesRefSeq) hipLaunchKernelGGL(k_cv_first, lgrid, blk, 0, s, J, k->tree, M);
  else hipLaunchKernelGGL(k_cv_entries, cgrid, blk, 0, s, J, k->tree, M, X);
  passed();
  hipLaunchKernelGGL(k_cv_decide, lgrid, blk, 0, s, J, k->tree, static_cast<const uint8_t *>(k->keep));
  passed();
  hipLaunchKernelGGL(k_cv_len, lgrid, blk, 0, s, J);
  kjl::launch_offsets(s, sgrid, count, static_cast<const uint32_t *>(J.olen), J.blk, J.blk_base, J.line_off);
  passed();
  hipLaunchKernelGGL(k_cv_write, wgrid, blk, 0, s, J);
  passed();
  hipLaunchKernelGGL(k_cv_finish, dim3(1), dim3(64), 0, s, J);
  passed();
  if (hipGetLastError() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "a kernel of the convert passes could not be launched");
  if (hipEventRecord(k->done, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventRecord of the converter");
  return KAIJU_GPU_OK;
}

int create(const kaiju_gpu_taxonomy *tax, const uint64_t *include_ids, uint32_t n_include, const kaiju_gpu_accmap *map, const kaiju_gpu_accmap *excluded, int rules,
           int add_acc, kaiju_gpu_converter **out) {
  return guarded([&]() -> int {
    if (!tax || !map || !out || (!include_ids && n_include)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (rules != kRulesNr && rules != kRulesRefSeq) return fail(KAIJU_GPU_ERR_ARG, "the rule set is KAIJU_GPU_CONVERT_RULES_NR or KAIJU_GPU_CONVERT_RULES_REFSEQ");
    if (kj_accmap_rules(map) != rules) return fail(KAIJU_GPU_ERR_ARG, "the accession map was made for the other rule set");
    const kaiju_gpu_taxonomy *map_tax = nullptr;
    int map_dev = -1, ex_dev = -1;
    (void)kj_accmap_view(map, &map_tax, &map_dev);
    if (map_tax != tax) return fail(KAIJU_GPU_ERR_ARG, "the accession map was built on another taxonomy");
    if (excluded) (void)kj_accmap_view(excluded, nullptr, &ex_dev);
    if (map_dev != tax->device || (excluded && ex_dev != tax->device)) return fail(KAIJU_GPU_ERR_ARG, "a map lives on another device than the tree");
    static const uint64_t kDefault[3] = {2, 2157, 10239};
    if (!include_ids) { include_ids = kDefault; n_include = 3; }

    kaiju_gpu_converter *k = new kaiju_gpu_converter();
    struct Guard { kaiju_gpu_converter *p; ~Guard() { kaiju_gpu_converter_free(p); } } guard{k};
    k->device = tax->device; k->tax = tax; k->map = map; k->excluded = excluded; k->add_acc = add_acc ? 1 : 0; k->rules = rules;
    k->tree = Tree{tax->dev.key, tax->dev.parent_slot, tax->dev.depth, tax->dev.cap_mask};
    if (hipSetDevice(k->device) != hipSuccess || hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&k->done, hipEventDisableTiming) != hipSuccess || hipHostMalloc(&k->h_info, sizeof(kaiju_gpu_convert_info) + 8, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(KAIJU_GPU_ERR_HIP, "hipStreamCreate / hipHostMalloc of the converter");
    }
    const char *e = getenv("KAIJU_GPU_CONVERT_TIMES");
    if (e && *e == '1') {
      for (hipEvent_t &ev : k->ev)
        if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); return fail(KAIJU_GPU_ERR_HIP, "hipEventCreate of the converter"); }
      k->timed = true;
    }
    const size_t cap = (size_t)tax->dev.cap_mask + 1;
    if (hipMalloc(&k->listed, cap) != hipSuccess || hipMalloc(&k->keep, cap) != hipSuccess || hipMalloc(&k->d_ids, ((size_t)n_include + 1) * 8) != hipSuccess) {
      (void)hipGetLastError();
      return fail(KAIJU_GPU_ERR_NOMEM, "hipMalloc of the converter's tables");
    }
    if (hipMemset(k->listed, 0, cap) != hipSuccess || (n_include && hipMemcpy(k->d_ids, include_ids, (size_t)n_include * 8, hipMemcpyHostToDevice) != hipSuccess))
      return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the include list");
    const dim3 grid((unsigned)std::min<uint64_t>(4096, cap / kCvBlock + 1));
    hipLaunchKernelGGL(k_cv_listed, grid, dim3(kCvBlock), 0, 0, k->tree, static_cast<const uint64_t *>(k->d_ids), n_include, k->listed);
    hipLaunchKernelGGL(k_cv_keep, grid, dim3(kCvBlock), 0, 0, k->tree, static_cast<const uint8_t *>(k->listed), k->keep);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "the kernels that build the converter's tables");
    if (hipEventRecord(k->done, k->stream) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventRecord of the converter");
    guard.p = nullptr;
    *out = k;
    return KAIJU_GPU_OK;
  });
}

}  // namespace

extern "C" int kaiju_gpu_converter_create(const kaiju_gpu_taxonomy *tax, const uint64_t *include_ids, uint32_t n_include, const kaiju_gpu_accmap *map,
                                          const kaiju_gpu_accmap *excluded, int add_acc, kaiju_gpu_converter **out) {
  return create(tax, include_ids, n_include, map, excluded, kRulesNr, add_acc, out);
}

extern "C" int kaiju_gpu_converter_create_rules(const kaiju_gpu_taxonomy *tax, const uint64_t *include_ids, uint32_t n_include, const kaiju_gpu_accmap *map,
                                                int rules, int add_acc, kaiju_gpu_converter **out) {
  return create(tax, include_ids, n_include, map, nullptr, rules, add_acc, out);
}

extern "C" void kaiju_gpu_converter_free(kaiju_gpu_converter *k) {
  if (!k) return;
  if (k->device >= 0 && hipSetDevice(k->device) == hipSuccess) {
    if (k->done) { (void)hipEventSynchronize(k->done); (void)hipEventDestroy(k->done); }
    if (k->stream) { (void)hipStreamSynchronize(k->stream); (void)hipStreamDestroy(k->stream); }
    for (hipEvent_t ev : k->ev) if (ev) (void)hipEventDestroy(ev);
    if (k->h_info) (void)hipHostFree(k->h_info);
    for (void *p : {(void *)k->listed, (void *)k->keep, (void *)k->d_ids}) if (p) (void)hipFree(p);
    k->mem.release(); k->text.release(); k->out.release(); k->info.release();
  }
  delete k;
}

extern "C" int kaiju_gpu_convert_text_device(kaiju_gpu_converter *k, const void *d_text, uint64_t bytes, void *d_out, uint64_t out_cap,
                                             kaiju_gpu_convert_info *d_info, void *stream) {
  return guarded([&]() -> int {
    if (!k) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(k->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    return launch(k, stream ? static_cast<hipStream_t>(stream) : k->stream, d_text, bytes, d_out, out_cap, d_info);
  });
}

extern "C" int kaiju_gpu_convert_text(kaiju_gpu_converter *k, const char *text, uint64_t bytes, char *out, uint64_t out_cap, kaiju_gpu_convert_info *info) {
  return guarded([&]() -> int {
    if (!k || !info || (!text && bytes) || (!out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (bytes > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
    if (hipSetDevice(k->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    const char *err = "";
    int rc;
    if ((rc = k->text.reserve(bytes + kChunk, 256, "hipMalloc of the converter's text", &err))) return fail(rc, err);
    if ((rc = k->out.reserve(out_cap + kChunk, 256, "hipMalloc of the converter's output", &err))) return fail(rc, err);
    if ((rc = k->info.reserve(sizeof(kaiju_gpu_convert_info), 256, "hipMalloc of the converter's info", &err))) return fail(rc, err);
    const hipStream_t s = k->stream;
    if (bytes && hipMemcpyAsync(k->text.p, text, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the text");
    kaiju_gpu_convert_info *d_info = static_cast<kaiju_gpu_convert_info *>(k->info.p);
    if ((rc = launch(k, s, k->text.p, bytes, out_cap ? k->out.p : nullptr, out_cap, d_info))) return rc;
    if (hipMemcpyAsync(k->h_info, d_info, sizeof *info, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, std::string("the convert passes: ") + hipGetErrorString(hipGetLastError()));
    memcpy(info, k->h_info, sizeof *info);
    if (info->written_bytes > out_cap) return fail(KAIJU_GPU_ERR_HIP, "the convert passes wrote more than out_cap");
    if (info->written_bytes && hipMemcpy(out, k->out.p, info->written_bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the converted text");
    return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_convert_pass_ms(kaiju_gpu_converter *k, float *ms, uint32_t n) {
  return guarded([&]() -> int {
    if (!k || (!ms && n)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (!k->timed) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "the converter was created without KAIJU_GPU_CONVERT_TIMES=1");
    if (hipSetDevice(k->device) != hipSuccess || hipEventSynchronize(k->ev[KAIJU_GPU_CONVERT_PASSES]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventSynchronize");
    for (uint32_t p = 0; p < n && p < KAIJU_GPU_CONVERT_PASSES; p++)
      if (hipEventElapsedTime(&ms[p], k->ev[p], k->ev[p + 1]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventElapsedTime");
    return KAIJU_GPU_OK;
  });
}
