// accmap.hip — the accession -> taxon map of kaiju-convertNR and kaiju-convertRefSeq on the device (gfx950, wave64): the entry
// points kaiju_gpu_accmap_* of include/kaiju_gpu.h.  The rules of either tool and the layout: kj_convert.h.
//
// per block   k_tl_*         the lines of the block                                                    (kj_textlines.h)
//             k_am_parse     one lane per line: key span, taxon, node / merged decision by the map's rule set (parse_map_line or
//                            refseq_map_line); what the block needs of the arena
//             (the host reads the two counts, grows the arena by reallocation and the slots by k_am_rehash)
//             k_am_insert    one lane per line that inserts: probe; an empty slot takes a new entry by compare-and-swap, an
//                            equal key takes the minimum of the line numbers
//             k_am_resolve   the line whose number an entry carries writes the entry's taxon
// lookups     k_am_lookup    one lane per line of keys          k_am_hist   the probe lengths, one lane per slot
//
// Every probe loop runs over at most `slots` slots and reports a full table in the header instead of spinning.  Entries that
// other lanes of k_am_insert have just published are read with agent-scope atomic loads: a plain load may hit a line of the
// arena that the lane's cache holds from in front of the write.
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

typedef unsigned long long am_u64;     // what the atomics take

namespace {

constexpr int kAmBlock = 256;

struct AmHdr {
  uint64_t arena_used, entries, lines, no_insert, duplicates;
  uint64_t need_bytes, n_valid;        // of the block
  uint32_t full, pad;
};

struct AmJob {
  TlText t;
  uint32_t *key_pos, *key_len;         // per line; key_len kNone: the line inserts nothing
  uint64_t *taxon, *ent;               // per line: its taxon, the entry of its key (offset / 8)
  AmHdr *hdr;
  uint64_t *slots, mask;
  uint8_t *arena;
  uint64_t ord_base, value;
  int first_block, keys_only, rules;
};

void carve(kjl::Carver &c, AmJob &J) {
  tl_carve(c, J.t);
  const size_t lines = J.t.bytes + 1;
  J.key_pos = c.take<uint32_t>(lines);
  J.key_len = c.take<uint32_t>(lines);
  J.taxon = c.take<uint64_t>(lines);
  J.ent = c.take<uint64_t>(lines);
}

__device__ __forceinline__ am_u64 wave_sum(am_u64 v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(kAmBlock) void k_am_parse(AmJob J, Tree T, Merged G) {
  const uint32_t n = *J.t.n_lines;
  am_u64 lines = 0, none = 0, need = 0, valid = 0;
  for (uint32_t i = blockIdx.x * kAmBlock + threadIdx.x; i < n; i += gridDim.x * kAmBlock) {
    J.key_len[i] = kNone;
    const uint64_t a = J.t.line_start[i], e = (uint64_t)J.t.line_start[i + 1] - 1;
    if (a >= e || (J.first_block && i == 0)) continue;
    lines++;
    MapLine L;
    uint32_t slot;
    if (J.rules == kRulesRefSeq && !J.keys_only) L = refseq_map_line(J.t.text, a, e, T, G);
    else {
      L = parse_map_line(J.t.text, a, e, J.keys_only != 0, J.value);
      if (L.valid && !J.keys_only) L.valid = resolve_taxon(T, G, &L.taxon, &slot);
    }
    if (!L.valid) { none++; continue; }
    J.key_pos[i] = (uint32_t)L.key;
    J.key_len[i] = (uint32_t)(L.key_end - L.key);
    J.taxon[i] = L.taxon;
    need += entry_bytes((uint32_t)(L.key_end - L.key));
    valid++;
  }
  lines = wave_sum(lines); none = wave_sum(none); need = wave_sum(need); valid = wave_sum(valid);
  if ((threadIdx.x & 63) == 0 && lines) {
    atomicAdd(reinterpret_cast<am_u64 *>(&J.hdr->lines), lines);
    atomicAdd(reinterpret_cast<am_u64 *>(&J.hdr->no_insert), none);
    atomicAdd(reinterpret_cast<am_u64 *>(&J.hdr->need_bytes), need);
    atomicAdd(reinterpret_cast<am_u64 *>(&J.hdr->n_valid), valid);
  }
}

__device__ __forceinline__ uint64_t fresh(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the entry at e (eight-byte words, the key zero-padded) holds key[0, n)
__device__ bool entry_is(const uint8_t *e, const uint8_t *key, uint32_t n) {
  const uint64_t *w = reinterpret_cast<const uint64_t *>(e);
  if ((uint32_t)fresh(w + 2) != n) return false;
  for (uint32_t k = 0; k < n; k += 8)
    if (fresh(w + 3 + k / 8) != load_word(key + k, n - k < 8 ? n - k : 8)) return false;
  return true;
}

__global__ __launch_bounds__(kAmBlock) void k_am_insert(AmJob J) {
  const uint32_t n = *J.t.n_lines;
  for (uint32_t i = blockIdx.x * kAmBlock + threadIdx.x; i < n; i += gridDim.x * kAmBlock) {
    const uint32_t len = J.key_len[i];
    if (len == kNone) continue;
    const uint8_t *key = J.t.text + J.key_pos[i];
    const uint64_t ord = J.ord_base + i;
    const uint64_t h = key_hash(key, len), tag = slot_tag(h);
    uint64_t s = slot_home(h, J.mask), mine = 0;
    bool done = false;
    for (uint64_t k = 0; k <= J.mask && !done; k++, s = (s + 1) & J.mask) {
      uint64_t v = fresh(J.slots + s);
      if (v == 0) {
        if (!mine) {                                           // the entry, complete in memory before a slot names it
          const uint64_t off = atomicAdd(reinterpret_cast<am_u64 *>(&J.hdr->arena_used), (am_u64)entry_bytes(len));
          uint64_t *w = reinterpret_cast<uint64_t *>(J.arena + off);
          w[0] = ord; w[1] = J.taxon[i]; w[2] = len;
          for (uint32_t q = 0; q < len; q += 8) w[3 + q / 8] = load_word(key + q, len - q < 8 ? len - q : 8);
          __threadfence();
          mine = tag << 40 | (off / 8 + 1);
        }
        v = atomicCAS(reinterpret_cast<am_u64 *>(J.slots + s), 0ull, (am_u64)mine);
        if (v == 0) {
          J.ent[i] = (mine & kEntryMask) - 1;
          atomicAdd(reinterpret_cast<am_u64 *>(&J.hdr->entries), 1ull);
          done = true;
          continue;
        }
      }
      if ((v >> 40) != tag) continue;
      uint8_t *e = J.arena + ((v & kEntryMask) - 1) * 8;
      if (!entry_is(e, key, len)) continue;
      atomicMin(reinterpret_cast<am_u64 *>(e), (am_u64)ord);
      J.ent[i] = (v & kEntryMask) - 1;
      atomicAdd(reinterpret_cast<am_u64 *>(&J.hdr->duplicates), 1ull);
      done = true;
    }
    if (!done) { J.key_len[i] = kNone; J.hdr->full = 1; }
  }
}

__global__ __launch_bounds__(kAmBlock) void k_am_resolve(AmJob J) {
  const uint32_t n = *J.t.n_lines;
  for (uint32_t i = blockIdx.x * kAmBlock + threadIdx.x; i < n; i += gridDim.x * kAmBlock) {
    if (J.key_len[i] == kNone) continue;
    uint64_t *w = reinterpret_cast<uint64_t *>(J.arena + J.ent[i] * 8);
    if (w[0] == J.ord_base + i) w[1] = J.taxon[i];
  }
}

__global__ __launch_bounds__(kAmBlock) void k_am_rehash(const uint64_t *old, uint64_t n_old, uint64_t *slots, uint64_t mask, const uint8_t *arena, AmHdr *hdr) {
  for (uint64_t i = (uint64_t)blockIdx.x * kAmBlock + threadIdx.x; i < n_old; i += (uint64_t)gridDim.x * kAmBlock) {
    const uint64_t v = old[i];
    if (!v) continue;
    const uint8_t *e = arena + ((v & kEntryMask) - 1) * 8;
    uint64_t s = slot_home(key_hash(e + kEntryHead, entry_len(e)), mask);
    bool done = false;
    for (uint64_t k = 0; k <= mask && !done; k++, s = (s + 1) & mask)
      done = atomicCAS(reinterpret_cast<am_u64 *>(slots + s), 0ull, (am_u64)v) == 0;
    if (!done) hdr->full = 1;
  }
}

__global__ __launch_bounds__(kAmBlock) void k_am_lookup(TlText X, Map M, uint64_t *out, uint64_t cap) {
  const uint32_t n = *X.n_lines;
  for (uint32_t i = blockIdx.x * kAmBlock + threadIdx.x; i < n && i < cap; i += gridDim.x * kAmBlock) {
    const uint64_t a = X.line_start[i], e = (uint64_t)X.line_start[i + 1] - 1;
    uint32_t probes;
    const uint8_t *ent = map_find(M, X.text + a, (uint32_t)(e - a), &probes);
    out[i] = ent ? entry_taxon(ent) : ~0ull;
  }
}

__global__ __launch_bounds__(kAmBlock) void k_am_hist(Map M, am_u64 *hist) {
  for (uint64_t s = (uint64_t)blockIdx.x * kAmBlock + threadIdx.x; s <= M.mask; s += (uint64_t)gridDim.x * kAmBlock) {
    const uint64_t v = M.slots[s];
    if (!v) continue;
    const uint8_t *e = M.arena + ((v & kEntryMask) - 1) * 8;
    const uint64_t d = ((s - slot_home(key_hash(e + kEntryHead, entry_len(e)), M.mask)) & M.mask) + 1;
    atomicAdd(&hist[d < 16 ? d - 1 : 15], 1ull);
  }
}

}  // namespace

struct kaiju_gpu_accmap {
  int device = -1;
  const kaiju_gpu_taxonomy *tax = nullptr;
  Tree tree{};
  Merged merged{};
  void *d_merged = nullptr;
  uint64_t *slots = nullptr, n_slots = 0;
  uint8_t *arena = nullptr;
  uint64_t arena_cap = 0;
  AmHdr *hdr = nullptr;                // device
  AmHdr host{};                        // what the last call left
  uint64_t ord_base = 0, rehashes = 0;
  int rules = kRulesNr;
  kjl::Scratch scratch, text, out;
  hipStream_t stream = nullptr;
  bool timed = false;
  hipEvent_t ev[KAIJU_GPU_ACCMAP_PASSES + 1] = {};
};

namespace {

// device memory of `bytes` bytes, asked for only when that much is free
int dev_alloc(void **p, uint64_t bytes, const char *what) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemGetInfo");
  if (bytes > free_b)
    return fail(KAIJU_GPU_ERR_NOMEM, std::string(what) + ": need " + std::to_string(bytes >> 20) + " MiB of device memory, " + std::to_string(free_b >> 20) + " MiB are free");
  if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(KAIJU_GPU_ERR_NOMEM, std::string(what) + ": hipMalloc of " + std::to_string(bytes >> 20) + " MiB"); }
  return KAIJU_GPU_OK;
}

dim3 grid_for(uint64_t n) { return dim3((unsigned)std::min<uint64_t>(8192, n / kAmBlock + 1)); }

// room for `need` more bytes of entries and `more` more keys
int grow(kaiju_gpu_accmap *m, uint64_t need, uint64_t more) {
  const hipStream_t s = m->stream;
  if (m->host.arena_used + need > m->arena_cap) {
    const uint64_t want = std::max<uint64_t>(m->arena_cap * 2, m->host.arena_used + need + (1u << 16));
    void *p = nullptr;
    if (int rc = dev_alloc(&p, want, "the arena of the accession map")) return rc;
    if (m->host.arena_used && hipMemcpyAsync(p, m->arena, m->host.arena_used, hipMemcpyDeviceToDevice, s) != hipSuccess) { (void)hipFree(p); return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the arena"); }
    if (hipStreamSynchronize(s) != hipSuccess) { (void)hipFree(p); return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the arena"); }
    if (m->arena) (void)hipFree(m->arena);
    m->arena = static_cast<uint8_t *>(p);
    m->arena_cap = want;
  }
  const uint64_t keys = m->host.entries + more;
  if (keys > m->n_slots / 4 * 3) {                              // at most 3/4 full; a new table is at most 1/2 full
    uint64_t want = m->n_slots;
    while (keys > want / 2) want *= 2;
    void *p = nullptr;
    if (int rc = dev_alloc(&p, want * 8, "the slots of the accession map")) return rc;
    if (hipMemsetAsync(p, 0, want * 8, s) != hipSuccess) { (void)hipFree(p); return fail(KAIJU_GPU_ERR_HIP, "hipMemset of the slots"); }
    hipLaunchKernelGGL(k_am_rehash, grid_for(m->n_slots), dim3(kAmBlock), 0, s, static_cast<const uint64_t *>(m->slots), m->n_slots, static_cast<uint64_t *>(p), want - 1,
                       static_cast<const uint8_t *>(m->arena), m->hdr);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { (void)hipFree(p); return fail(KAIJU_GPU_ERR_HIP, "the rehash of the accession map"); }
    (void)hipFree(m->slots);
    m->slots = static_cast<uint64_t *>(p);
    m->n_slots = want;
    m->rehashes++;
  }
  return KAIJU_GPU_OK;
}

int read_hdr(kaiju_gpu_accmap *m) {
  if (hipMemcpyAsync(&m->host, m->hdr, sizeof(AmHdr), hipMemcpyDeviceToHost, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess)
    return fail(KAIJU_GPU_ERR_HIP, std::string("the passes of the accession map: ") + hipGetErrorString(hipGetLastError()));
  return KAIJU_GPU_OK;
}

int add(kaiju_gpu_accmap *m, const void *d_text, uint64_t bytes, int first_block, int keys_only, uint64_t value) {
  if (!d_text && bytes) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (bytes > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
  if ((uintptr_t)d_text & (kChunk - 1)) return fail(KAIJU_GPU_ERR_ARG, "the text must be 16-byte aligned");
  if (!keys_only && !m->tax) return fail(KAIJU_GPU_ERR_ARG, "a map without a taxonomy takes keys only");
  AmJob J{};
  J.t.text = static_cast<const uint8_t *>(d_text); J.t.bytes = bytes;
  kjl::Carver measure{nullptr};
  carve(measure, J);
  const char *err = "";
  if (int rc = m->scratch.reserve(measure.at, 256, "hipMalloc of the accession map's scratch", &err)) return fail(rc, err);
  kjl::Carver c{static_cast<uint8_t *>(m->scratch.p)};
  carve(c, J);
  J.hdr = m->hdr; J.ord_base = m->ord_base; J.value = value; J.first_block = first_block ? 1 : 0; J.keys_only = keys_only; J.rules = m->rules;
  const hipStream_t s = m->stream;
  const dim3 blk(kAmBlock), grid = grid_for(bytes / 4);
  int mark = 0;
  auto passed = [&]() { if (m->timed) (void)hipEventRecord(m->ev[mark++], s); };
  // the counts of the block
  if (hipMemsetAsync(&m->hdr->need_bytes, 0, 16, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemset");
  passed();
  tl_launch(s, J.t);
  passed();
  hipLaunchKernelGGL(k_am_parse, grid, blk, 0, s, J, m->tree, m->merged);
  if (hipGetLastError() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "a kernel of the accession map could not be launched");
  if (int rc = read_hdr(m)) return rc;
  passed();
  if (int rc = grow(m, m->host.need_bytes, m->host.n_valid)) return rc;
  passed();
  J.slots = m->slots; J.mask = m->n_slots - 1; J.arena = m->arena;
  hipLaunchKernelGGL(k_am_insert, grid, blk, 0, s, J);
  passed();
  hipLaunchKernelGGL(k_am_resolve, grid, blk, 0, s, J);
  passed();
  if (hipGetLastError() != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "a kernel of the accession map could not be launched");
  if (int rc = read_hdr(m)) return rc;
  m->ord_base += bytes + 1;                                     // (more than the block has lines)
  if (m->host.full) return fail(KAIJU_GPU_ERR_FORMAT, "the accession map is full: " + std::to_string(m->host.entries) + " keys in " + std::to_string(m->n_slots) + " slots");
  return KAIJU_GPU_OK;
}

int add_host(kaiju_gpu_accmap *m, const char *text, uint64_t n, int first_block, int keys_only, uint64_t value) {
  if (!m || (!text && n)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (n > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
  if (hipSetDevice(m->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
  const char *err = "";
  if (int rc = m->text.reserve(n + kChunk, 256, "hipMalloc of the accession map's text", &err)) return fail(rc, err);
  if (n && hipMemcpyAsync(m->text.p, text, n, hipMemcpyHostToDevice, m->stream) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the text");
  return add(m, m->text.p, n, first_block, keys_only, value);
}

}  // namespace

// what convert.hip reads of a map, at every call: the map may have grown
kjc::Map kj_accmap_view(const kaiju_gpu_accmap *m, const kaiju_gpu_taxonomy **tax, int *device) {
  if (tax) *tax = m->tax;
  if (device) *device = m->device;
  return Map{m->slots, m->n_slots - 1, m->arena};
}
int kj_accmap_rules(const kaiju_gpu_accmap *m) { return m->rules; }

static_assert(kRulesNr == KAIJU_GPU_CONVERT_RULES_NR && kRulesRefSeq == KAIJU_GPU_CONVERT_RULES_REFSEQ, "the rule sets of kj_convert.h are those of kaiju_gpu.h");

extern "C" int kaiju_gpu_accmap_create_rules(const kaiju_gpu_taxonomy *tax, int device_id, const uint64_t *merged_pairs, uint64_t n_merged, int rules,
                                             uint64_t initial_slots, kaiju_gpu_accmap **out) {
  return guarded([&]() -> int {
    if (!out || (!merged_pairs && n_merged)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (rules != kRulesNr && rules != kRulesRefSeq) return fail(KAIJU_GPU_ERR_ARG, "the rule set is KAIJU_GPU_CONVERT_RULES_NR or KAIJU_GPU_CONVERT_RULES_REFSEQ");
    if (tax && tax->device != device_id) return fail(KAIJU_GPU_ERR_ARG, "the tree lives on another device");
    if (n_merged > 0xfffffff0ull) return fail(KAIJU_GPU_ERR_ARG, "too many merged pairs");
    if (initial_slots > (1ull << 40)) return fail(KAIJU_GPU_ERR_ARG, "initial_slots above 2^40");
    if (int rc = no_device()) return rc;
    // the first pair of an old id wins (emplace), then sorted by the old id
    std::vector<std::pair<uint64_t, uint64_t>> pairs;
    pairs.reserve(n_merged);
    for (uint64_t i = 0; i < n_merged; i++) pairs.emplace_back(merged_pairs[2 * i], merged_pairs[2 * i + 1]);
    std::stable_sort(pairs.begin(), pairs.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    pairs.erase(std::unique(pairs.begin(), pairs.end(), [](const auto &x, const auto &y) { return x.first == y.first; }), pairs.end());
    std::vector<uint64_t> flat(2 * pairs.size() + 2);
    for (size_t i = 0; i < pairs.size(); i++) { flat[i] = pairs[i].first; flat[pairs.size() + i] = pairs[i].second; }

    kaiju_gpu_accmap *m = new kaiju_gpu_accmap();
    struct Guard { kaiju_gpu_accmap *p; ~Guard() { kaiju_gpu_accmap_free(p); } } guard{m};
    m->device = device_id;
    m->tax = tax;
    m->rules = rules;
    if (tax) m->tree = Tree{tax->dev.key, tax->dev.parent_slot, tax->dev.depth, tax->dev.cap_mask};
    if (hipSetDevice(m->device) != hipSuccess || hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return fail(KAIJU_GPU_ERR_HIP, "hipStreamCreate of the accession map"); }
    const char *e = getenv("KAIJU_GPU_CONVERT_TIMES");
    if (e && *e == '1') {
      for (hipEvent_t &ev : m->ev)
        if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); return fail(KAIJU_GPU_ERR_HIP, "hipEventCreate of the accession map"); }
      m->timed = true;
    }
    uint64_t n_slots = 8;
    const uint64_t want = initial_slots ? initial_slots : (1ull << 16);
    while (n_slots < want) n_slots *= 2;
    void *p = nullptr;
    int rc;
    if ((rc = dev_alloc(&p, flat.size() * 8, "the merged ids"))) return rc;
    m->d_merged = p;
    if ((rc = dev_alloc(&p, n_slots * 8, "the slots of the accession map"))) return rc;
    m->slots = static_cast<uint64_t *>(p); m->n_slots = n_slots;
    m->arena_cap = 1u << 16;
    if ((rc = dev_alloc(&p, m->arena_cap, "the arena of the accession map"))) return rc;
    m->arena = static_cast<uint8_t *>(p);
    if ((rc = dev_alloc(&p, sizeof(AmHdr), "the header of the accession map"))) return rc;
    m->hdr = static_cast<AmHdr *>(p);
    if (hipMemcpy(m->d_merged, flat.data(), flat.size() * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemset(m->slots, 0, n_slots * 8) != hipSuccess ||
        hipMemset(m->hdr, 0, sizeof(AmHdr)) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy / hipMemset of the accession map");
    const uint64_t *d = static_cast<const uint64_t *>(m->d_merged);
    m->merged = Merged{d, d + pairs.size(), (uint32_t)pairs.size()};
    guard.p = nullptr;
    *out = m;
    return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_accmap_create(const kaiju_gpu_taxonomy *tax, int device_id, const uint64_t *merged_pairs, uint64_t n_merged, uint32_t key_col,
                                       uint32_t taxon_col, uint64_t initial_slots, kaiju_gpu_accmap **out) {
  const int rc = guarded([&]() -> int {
    if (!out || (!merged_pairs && n_merged)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (key_col != 1 || taxon_col != 2) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "the key is column 1 and the taxon column 2 (prot.accession2taxid); other columns are not built yet");
    return KAIJU_GPU_OK;
  });
  if (rc != KAIJU_GPU_OK) return rc;
  return kaiju_gpu_accmap_create_rules(tax, device_id, merged_pairs, n_merged, KAIJU_GPU_CONVERT_RULES_NR, initial_slots, out);
}

extern "C" void kaiju_gpu_accmap_free(kaiju_gpu_accmap *m) {
  if (!m) return;
  if (m->device >= 0 && hipSetDevice(m->device) == hipSuccess) {
    if (m->stream) { (void)hipStreamSynchronize(m->stream); (void)hipStreamDestroy(m->stream); }
    for (hipEvent_t ev : m->ev) if (ev) (void)hipEventDestroy(ev);
    for (void *p : {(void *)m->d_merged, (void *)m->slots, (void *)m->arena, (void *)m->hdr}) if (p) (void)hipFree(p);
    m->scratch.release(); m->text.release(); m->out.release();
  }
  delete m;
}

extern "C" int kaiju_gpu_accmap_add_text(kaiju_gpu_accmap *m, const char *text, uint64_t n, int is_first_block) {
  return guarded([&]() -> int { return add_host(m, text, n, is_first_block, 0, 0); });
}

extern "C" int kaiju_gpu_accmap_add_keys(kaiju_gpu_accmap *m, const char *text, uint64_t n, uint64_t value) {
  return guarded([&]() -> int { return add_host(m, text, n, 0, 1, value); });
}

extern "C" int kaiju_gpu_accmap_add_text_device(kaiju_gpu_accmap *m, const void *d_text, uint64_t n, int is_first_block) {
  return guarded([&]() -> int {
    if (!m) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(m->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    return add(m, d_text, n, is_first_block, 0, 0);
  });
}

extern "C" int kaiju_gpu_accmap_lookup(kaiju_gpu_accmap *m, const char *keys, uint64_t n, uint64_t *taxa, uint64_t cap, uint64_t *n_keys) {
  return guarded([&]() -> int {
    if (!m || !n_keys || (!keys && n) || (!taxa && cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (n > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 16 bytes");
    if (hipSetDevice(m->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    TlText X{};
    X.bytes = n;
    kjl::Carver measure{nullptr};
    tl_carve(measure, X);
    const char *err = "";
    int rc;
    if ((rc = m->scratch.reserve(measure.at, 256, "hipMalloc of the accession map's scratch", &err))) return fail(rc, err);
    if ((rc = m->text.reserve(n + kChunk, 256, "hipMalloc of the accession map's text", &err))) return fail(rc, err);
    if ((rc = m->out.reserve((n + 1) * 8, 256, "hipMalloc of the looked-up taxa", &err))) return fail(rc, err);
    X.text = static_cast<const uint8_t *>(m->text.p);
    kjl::Carver c{static_cast<uint8_t *>(m->scratch.p)};
    tl_carve(c, X);
    const hipStream_t s = m->stream;
    if (n && hipMemcpyAsync(m->text.p, keys, n, hipMemcpyHostToDevice, s) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the keys");
    tl_launch(s, X);
    hipLaunchKernelGGL(k_am_lookup, grid_for(n / 4), dim3(kAmBlock), 0, s, X, Map{m->slots, m->n_slots - 1, m->arena}, static_cast<uint64_t *>(m->out.p), (uint64_t)n + 1);
    uint32_t lines = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&lines, X.n_lines, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, std::string("the lookup in the accession map: ") + hipGetErrorString(hipGetLastError()));
    *n_keys = lines;
    const uint64_t take = std::min<uint64_t>(lines, cap);
    if (take && hipMemcpy(taxa, m->out.p, take * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemcpy of the looked-up taxa");
    return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_accmap_info(kaiju_gpu_accmap *m, kaiju_gpu_accmap_stats *out) {
  return guarded([&]() -> int {
    if (!m || !out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (hipSetDevice(m->device) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipSetDevice");
    memset(out, 0, sizeof *out);
    out->entries = m->host.entries; out->slots = m->n_slots;
    out->arena_bytes = m->host.arena_used; out->arena_cap = m->arena_cap;
    out->lines = m->host.lines; out->lines_no_insert = m->host.no_insert; out->duplicates = m->host.duplicates;
    out->rehashes = m->rehashes;
    const char *err = "";
    if (int rc = m->out.reserve(16 * 8, 256, "hipMalloc of the probe lengths", &err)) return fail(rc, err);
    if (hipMemsetAsync(m->out.p, 0, 16 * 8, m->stream) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipMemset");
    hipLaunchKernelGGL(k_am_hist, grid_for(m->n_slots), dim3(kAmBlock), 0, m->stream, Map{m->slots, m->n_slots - 1, m->arena}, static_cast<am_u64 *>(m->out.p));
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(out->probe_hist, m->out.p, 16 * 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
      return fail(KAIJU_GPU_ERR_HIP, "the probe lengths of the accession map");
    return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_accmap_pass_ms(kaiju_gpu_accmap *m, float *ms, uint32_t n) {
  return guarded([&]() -> int {
    if (!m || (!ms && n)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (!m->timed) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "the accession map was created without KAIJU_GPU_CONVERT_TIMES=1");
    if (hipSetDevice(m->device) != hipSuccess || hipEventSynchronize(m->ev[KAIJU_GPU_ACCMAP_PASSES]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventSynchronize");
    for (uint32_t p = 0; p < n && p < KAIJU_GPU_ACCMAP_PASSES; p++)
      if (hipEventElapsedTime(&ms[p], m->ev[p], m->ev[p + 1]) != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, "hipEventElapsedTime");
    return KAIJU_GPU_OK;
  });
}
