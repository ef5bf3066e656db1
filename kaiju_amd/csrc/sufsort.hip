// sufsort.hip - the suffix sort of the index builder on the device (gfx950): prefix doubling over ranks, kj_sufsort.h has the
// definition, the rank invariant and the per-lane logic.  Here: the kernels and the driver loop.  The stable radix sort of
// (64-bit key, position) and the prefix scans are rocPRIM's; everything else is below.
//
// Passes.  Round 1: k_ss_count (letters per tile of 4096 text bytes) -> exclusive scan of the tile counts -> k_ss_keys (keys
// of 12 symbols and positions in position order, sequence numbers as ranks of the terminators) -> radix sort, 60 bits.
// Round h: k_ss_round_keys (rank[p] << 32 | rank[p + h] of the active list) -> radix sort.  Every round then: k_ss_heads ->
// inclusive max-scan of (last old head, last new head) -> k_ss_ranks (new ranks, flags of what stays active) -> inclusive scan
// of the flags -> k_ss_compact (the next active list) -> ONE read-back: the active count.  At the end k_ss_scatter writes
// SA[rank[p] - nseq] = p.  All memory is allocated in front of round 1 (ss_scratch_bytes + rocPRIM's temporary storage,
// compared with the free HBM first).
//
// Two instantiations of all of it on the position type P (kj_sufsort.h): uint32_t, the narrow one, and uint64_t, the wide one,
// in which positions, ranks, list indexes, tile bases, flags and the active count have 64 bits.  The wide round key
// (rank[p], rank[p + h]) does not fit a 64-bit radix key, so a wide round sorts twice, both times stable and over
// bits(rank_bias + tlen) bits: k_ss_round_keys writes rank[p + h], sort, k_ss_round_keys_hi writes rank[p] of the sorted
// positions, sort.  Behind that the key buffer holds rank[p]; k_ss_heads loads rank[p + h] again for an entry and its
// predecessor.  The wide scan item has 16 bytes and lies over the free key buffer and the active list, which is dead between
// k_ss_round_keys and k_ss_compact (the slab below keeps the two side by side).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <string>
#include <type_traits>

#include "kj_sufsort.h"
#include "mkfmi.h"

static_assert((int)KJ_SS_STATS_ROUNDS == (int)KAIJU_SUFSORT_STATS_ROUNDS, "kaiju_sufsort_stats");

namespace {

template <class P> struct SsTypes;
template <> struct SsTypes<uint32_t> { typedef uint64_t Item; typedef SsScanMax Scan; static constexpr bool wide = false; };
template <> struct SsTypes<uint64_t> { typedef SsScanItemW Item; typedef SsScanMaxW Scan; static constexpr bool wide = true; };

// ---- kernels -------------------------------------------------------------------------------------------------------------
// text is allocated to ss_text_alloc(tlen) bytes, zero behind tlen: lane g reads bytes [16 g, 16 g + 32)
template <class P>
__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_count(const uint4 *__restrict__ text, uint64_t nlanes, P *__restrict__ tile_count) {
  const uint64_t g = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x;
  uint32_t c = 0;
  if (g < nlanes) {
    const uint4 v = text[g];
    c = ss_lane_letters((uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32));
  }
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  __shared__ uint32_t part[KJ_SS_BLOCK / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < KJ_SS_BLOCK / 64; w++) s += part[w];
    tile_count[blockIdx.x] = s;
  }
}

// rank_bias: 0 in the narrow instantiation
template <class P>
__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_keys(const uint4 *__restrict__ text, uint64_t nlanes, uint64_t tlen, uint64_t nsuf,
                                                        const P *__restrict__ tile_base, uint64_t rank_bias, uint64_t *__restrict__ keys,
                                                        P *__restrict__ vals, P *__restrict__ rank) {
  const uint64_t g = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x;
  uint64_t k[KJ_SS_LANE_BYTES];
  uint32_t letters = 0;
  if (g < nlanes) {
    const uint4 a = text[g], b = text[g + 1];
    const uint64_t w[4] = {(uint64_t)a.x | ((uint64_t)a.y << 32), (uint64_t)a.z | ((uint64_t)a.w << 32),
                           (uint64_t)b.x | ((uint64_t)b.y << 32), (uint64_t)b.z | ((uint64_t)b.w << 32)};
    letters = ss_lane_keys(w, k);
  }
  // exclusive prefix of the letter counts inside the block
  const uint32_t cnt = __popc(letters);
  uint32_t inc = cnt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
  __shared__ uint32_t part[KJ_SS_BLOCK / 64];
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; w++) before += part[w];
  if (g >= nlanes) return;
  uint64_t o = ss_lane_base(tile_base[blockIdx.x], before, inc, cnt);      // letters in front of the lane's first byte
  const uint64_t p0 = g * KJ_SS_LANE_BYTES;
#pragma unroll
  for (int j = 0; j < KJ_SS_LANE_BYTES; j++) {
    const uint64_t p = p0 + j;
    if ((letters >> j) & 1u) {
      if (o < nsuf) { keys[o] = k[j]; vals[o] = (P)p; }
      o++;
    } else if (p < tlen) {
      rank[p] = (P)(rank_bias + (p - o));    // a terminator: its sequence number = the terminators in front of it
    }
  }
}

// narrow: the whole key; wide: its low part rank[p + h], the key of the first of the two sorts
template <class P>
__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_round_keys(const P *__restrict__ act, uint64_t m, const P *__restrict__ rank, uint64_t h,
                                                              uint64_t tlen, uint64_t *__restrict__ keys, P *__restrict__ vals) {
  for (uint64_t i = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const P p = act[i];
    if constexpr (SsTypes<P>::wide) keys[i] = p < tlen ? ss_rank_ahead(rank, p, h, tlen) : 0ull;
    else keys[i] = p < tlen ? ss_round_key(rank, p, h, tlen) : 0ull;
    vals[i] = p;
  }
}

// wide: the high part rank[p] of the positions as the first sort left them, the key of the second sort
__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_round_keys_hi(const uint64_t *__restrict__ vals, uint64_t m, const uint64_t *__restrict__ rank,
                                                                 uint64_t tlen, uint64_t *__restrict__ keys) {
  for (uint64_t i = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const uint64_t p = vals[i];
    keys[i] = p < tlen ? rank[p] : 0ull;
  }
}

// keys: round 1 the keys of 12 symbols; round h narrow the whole key, wide rank[p] (rank[p + h] is loaded again through vals)
template <class P>
__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_heads(const uint64_t *__restrict__ keys, const P *__restrict__ vals, const P *__restrict__ rank,
                                                         uint64_t m, int first, uint64_t h, uint64_t tlen,
                                                         typename SsTypes<P>::Item *__restrict__ items) {
  for (uint64_t i = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const uint64_t k = keys[i], kp = i ? keys[i - 1] : 0ull;
    if constexpr (SsTypes<P>::wide) {
      if (first) {
        items[i] = ss_scan_item_wide(i, false, ss_head_first(i, kp, k));
      } else {
        const SsKeyW key = {k, ss_rank_ahead(rank, vals[i], h, tlen)}, prev = {kp, i ? ss_rank_ahead(rank, vals[i - 1], h, tlen) : 0ull};
        items[i] = ss_scan_item_wide(i, ss_head_old(i, prev, key), ss_head_new(i, prev, key));
      }
    } else {
      items[i] = first ? ss_scan_item((uint32_t)i, false, ss_head_first(i, kp, k))
                       : ss_scan_item((uint32_t)i, ss_head_old(i, kp, k), ss_head_new(i, kp, k));
    }
  }
}

// first_rank: the rank of the first letter suffix, rank_bias + nseq
template <class P>
__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_ranks(const uint64_t *__restrict__ keys, const P *__restrict__ vals,
                                                         const typename SsTypes<P>::Item *__restrict__ scanned, uint64_t m, int first,
                                                         uint64_t first_rank, uint64_t tlen, P *__restrict__ rank, P *__restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const typename SsTypes<P>::Item s = scanned[i], sn = i + 1 < m ? scanned[i + 1] : typename SsTypes<P>::Item();
    const P p = vals[i];
    if (p < tlen) {
      if constexpr (SsTypes<P>::wide) {
        const SsKeyW key = {keys[i], 0ull};
        rank[p] = first ? ss_rank_first(first_rank, s) : ss_rank_round(key, s);
      } else {
        rank[p] = first ? ss_rank_first((uint32_t)first_rank, s) : ss_rank_round(keys[i], s);
      }
    }
    flags[i] = ss_is_final(i, m, s, sn) ? 0u : 1u;
  }
}

template <class P>
__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_compact(const P *__restrict__ vals, const P *__restrict__ incl, uint64_t m, P *__restrict__ act) {
  for (uint64_t i = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const P c = incl[i], b = i ? incl[i - 1] : 0u;
    if (c != b && c <= m) act[c - 1] = vals[i];        // (c <= i + 1 by construction)
  }
}

// rank is allocated to 16 nlanes entries: lane g reads its 16
template <class P>
__global__ __launch_bounds__(KJ_SS_BLOCK) void k_ss_scatter(const uint4 *__restrict__ text, const P *__restrict__ rank, uint64_t nlanes,
                                                           uint64_t first_rank, uint64_t nsuf, P *__restrict__ sa) {
  for (uint64_t g = (uint64_t)blockIdx.x * KJ_SS_BLOCK + threadIdx.x; g < nlanes; g += (uint64_t)gridDim.x * KJ_SS_BLOCK) {
    const uint4 t = text[g];
    const uint32_t tw[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (!tw[q]) continue;
      P rw[4];
      if constexpr (SsTypes<P>::wide) {
        const ulonglong2 a = reinterpret_cast<const ulonglong2 *>(rank)[g * 8 + q * 2], b = reinterpret_cast<const ulonglong2 *>(rank)[g * 8 + q * 2 + 1];
        rw[0] = a.x; rw[1] = a.y; rw[2] = b.x; rw[3] = b.y;
      } else {
        const uint4 r = reinterpret_cast<const uint4 *>(rank)[g * 4 + q];
        rw[0] = r.x; rw[1] = r.y; rw[2] = r.z; rw[3] = r.w;
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (!((tw[q] >> (8 * j)) & 0xffu)) continue;
        const uint64_t row = (uint64_t)rw[j] - first_rank;       // (wraps to a huge value if the rank were below the first letter's)
        if (row < nsuf) sa[row] = (P)(g * KJ_SS_LANE_BYTES + q * 4 + j);
      }
    }
  }
}

// ---- driver ---------------------------------------------------------------------------------------------------------------
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
  template <class T> T *as() { return static_cast<T *>(p); }
};
struct Events {
  hipEvent_t a = nullptr, b = nullptr;
  ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};
struct DeviceGuard {
  int prev = -1;
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

unsigned grid_for(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + KJ_SS_BLOCK - 1) / KJ_SS_BLOCK, 2048)); }
int bits_of(uint64_t v) { int b = 0; while (v >> b) ++b; return b; }

#define SS_HIP(call)                                                                                          \
  do {                                                                                                        \
    const hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) { err = std::string("suffix sort on the device: ") + #call + ": " + hipGetErrorString(e_); return KAIJU_GPU_ERR_HIP; } \
  } while (0)

// rocPRIM's temporary storage: asked with the element counts as size_t, which pass 2^32 in the wide instantiation
template <class P> size_t sort_temp(uint64_t n, unsigned end_bit) {
  rocprim::double_buffer<uint64_t> k(nullptr, nullptr);
  rocprim::double_buffer<P> v(nullptr, nullptr);
  size_t s = 0;
  (void)rocprim::radix_sort_pairs(nullptr, s, k, v, (size_t)n, 0u, end_bit);
  return s;
}
template <class P> size_t scan_items_temp(uint64_t n) {
  typedef typename SsTypes<P>::Item Item;
  size_t s = 0;
  (void)rocprim::inclusive_scan(nullptr, s, (Item *)nullptr, (Item *)nullptr, (size_t)n, typename SsTypes<P>::Scan());
  return s;
}
template <class P> size_t scan_flags_temp(uint64_t n) { size_t s = 0; (void)rocprim::inclusive_scan(nullptr, s, (P *)nullptr, (P *)nullptr, (size_t)n, rocprim::plus<P>()); return s; }
template <class P> size_t tile_temp(uint64_t n) { size_t s = 0; (void)rocprim::exclusive_scan(nullptr, s, (P *)nullptr, (P *)nullptr, (P)0, (size_t)n, rocprim::plus<P>()); return s; }

// the bits a round's radix sort runs over.  Narrow: rank[p] above bit 32.  Wide: each of the two sorts over one rank, and every
// rank, the bias included, is below rank_bias + tlen
template <class P> unsigned round_bits_of(uint64_t tlen, uint64_t rank_bias) {
  return SsTypes<P>::wide ? (unsigned)bits_of(rank_bias + tlen) : 32u + (unsigned)bits_of(tlen);
}

// what one sort allocates (the caller has selected the device: rocPRIM sizes its temporary storage for it)
template <class P> uint64_t need_bytes(uint64_t tlen, uint64_t nsuf, uint64_t rank_bias, uint64_t *temp_bytes_out) {
  const uint64_t n = std::max<uint64_t>(nsuf, 1);
  const uint64_t nlanes = (tlen + KJ_SS_LANE_BYTES - 1) / KJ_SS_LANE_BYTES, ntiles = (nlanes + KJ_SS_BLOCK - 1) / KJ_SS_BLOCK;
  const uint64_t rank_entries = nlanes * KJ_SS_LANE_BYTES;
  const unsigned round_bits = round_bits_of<P>(tlen, rank_bias);
  const size_t temp_bytes = std::max({sort_temp<P>(n, KJ_SS_KEY_BITS), sort_temp<P>(n, round_bits), scan_items_temp<P>(n), scan_flags_temp<P>(n), tile_temp<P>(ntiles)});
  if (temp_bytes_out) *temp_bytes_out = temp_bytes;
  if (SsTypes<P>::wide) return ss_scratch_bytes_wide(tlen, nsuf) + 8 * (rank_entries - tlen) + temp_bytes;      // (both tile arrays are in the formula)
  return ss_scratch_bytes(tlen, nsuf) + 4 * (rank_entries - tlen) + temp_bytes + 4 * ntiles;
}

// keep != nullptr (narrow only): SA is not downloaded (sa_out may be nullptr); text, rank[], SA, the first key buffer and the
// temporary storage stay allocated and are handed to the caller, who frees them (hipFree) - also for a text without a suffix,
// whose terminators still get their ranks
template <class P>
int sufsort_run(const uint8_t *text, uint64_t tlen, int device_id, P *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats, SsKeep *keep,
                uint64_t rank_bias, std::string &err) {
  constexpr bool wide = SsTypes<P>::wide;
  typedef typename SsTypes<P>::Item Item;
  if (stats) memset(stats, 0, sizeof *stats);
  if (n_out) *n_out = 0;
  if (wide) {
    if (keep) { err = "internal: suffix sort on the device: the wide sort keeps nothing"; return KAIJU_GPU_ERR_ARG; }
    if (tlen >= (1ull << 40) || rank_bias >= (1ull << 40) || !ss_tlen_ok_wide(tlen + rank_bias)) {
      err = "suffix sort on the device: 40-bit ranks only (text of " + std::to_string(tlen) + " symbols, rank bias " + std::to_string(rank_bias) +
            "); kaiju_build_fmi, the host builder, sorts texts of any length";
      return KAIJU_GPU_ERR_ARG;
    }
  } else if (!ss_tlen_ok(tlen)) {
    err = "suffix sort on the device: 32-bit positions only (text of " + std::to_string(tlen) + " symbols); kaiju_suffix_sort_device_wide sorts with 64-bit positions on the device, kaiju_build_fmi, the host builder, on the host";
    return KAIJU_GPU_ERR_ARG;
  }
  if (!text || tlen == 0 || (!sa_out && !keep)) { err = "suffix sort on the device: no text"; return KAIJU_GPU_ERR_ARG; }
  if (text[tlen - 1] != 0) { err = "suffix sort on the device: the text does not end with a terminator"; return KAIJU_GPU_ERR_ARG; }
  int rc = kj_sufsort_check_device(device_id, err);
  if (rc != KAIJU_GPU_OK) return rc;
  // sequences and the longest of them: the bound of the round loop
  uint64_t nseq = 0, maxlen = 0;
  for (uint64_t p = 0; p < tlen;) {
    const uint8_t *z = static_cast<const uint8_t *>(memchr(text + p, 0, (size_t)(tlen - p)));
    const uint64_t e = (uint64_t)(z - text);                 // (found: the last byte is a terminator)
    maxlen = std::max(maxlen, e - p);
    nseq++;
    p = e + 1;
  }
  const uint64_t nsuf = tlen - nseq;
  if (n_out) *n_out = nsuf;
  if (nsuf == 0 && !keep) return KAIJU_GPU_OK;

  DeviceGuard dg;
  SS_HIP(hipGetDevice(&dg.prev));
  SS_HIP(hipSetDevice(device_id));

  const uint64_t nlanes = (tlen + KJ_SS_LANE_BYTES - 1) / KJ_SS_LANE_BYTES, ntiles = (nlanes + KJ_SS_BLOCK - 1) / KJ_SS_BLOCK;
  const uint64_t text_bytes = ss_text_alloc(tlen), rank_entries = nlanes * KJ_SS_LANE_BYTES;
  const unsigned round_bits = round_bits_of<P>(tlen, rank_bias);
  const uint64_t first_rank = rank_bias + nseq;
  uint64_t temp_bytes64 = 0;
  const uint64_t need = need_bytes<P>(tlen, nsuf, rank_bias, &temp_bytes64);
  const size_t temp_bytes = (size_t)temp_bytes64;
  size_t free_b = 0, total_b = 0;
  SS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (getenv("KAIJU_GPU_LOAD_TIMES") && wide)
    fprintf(stderr, "[kaiju mkfmi]   wide suffix sort: needs %llu bytes of device memory (%.2f per symbol, %llu of them temporary storage), %llu are free\n",
            (unsigned long long)need, (double)need / (double)tlen, (unsigned long long)temp_bytes64, (unsigned long long)free_b);
  if (need > free_b) {
    err = "suffix sort on the device: needs " + std::to_string(need >> 20) + " MiB of device memory, " + std::to_string(free_b >> 20) +
          " MiB are free; kaiju_build_fmi sorts on the host";
    return KAIJU_GPU_ERR_NOMEM;
  }
  // narrow: an allocation each (some are handed on to the stages behind the sort).  Wide: the five arrays of 8 bytes per suffix
  // in one slab, key buffer / active list / key buffer / positions / positions, so that whichever key buffer is free lies next
  // to the active list and the two hold the scan items of 16 bytes
  DevBuf d_text, d_rank, d_k0, d_k1, d_v0, d_v1, d_act, d_tcnt, d_tbase, d_temp;
  SS_HIP(d_text.alloc(text_bytes));
  SS_HIP(d_rank.alloc(sizeof(P) * rank_entries));
  uint64_t *k0, *k1;
  P *v0, *v1, *act;
  if (wide) {
    const uint64_t stride = ss_wide_stride(nsuf);
    SS_HIP(d_k0.alloc(5 * stride));
    uint8_t *slab = d_k0.as<uint8_t>();
    k0 = reinterpret_cast<uint64_t *>(slab); act = reinterpret_cast<P *>(slab + stride); k1 = reinterpret_cast<uint64_t *>(slab + 2 * stride);
    v0 = reinterpret_cast<P *>(slab + 3 * stride); v1 = reinterpret_cast<P *>(slab + 4 * stride);
  } else {
    SS_HIP(d_k0.alloc(8 * nsuf));
    SS_HIP(d_k1.alloc(8 * nsuf));
    SS_HIP(d_v0.alloc(4 * nsuf));
    SS_HIP(d_v1.alloc(4 * nsuf));
    SS_HIP(d_act.alloc(4 * nsuf));
    k0 = d_k0.as<uint64_t>(); k1 = d_k1.as<uint64_t>(); v0 = d_v0.as<P>(); v1 = d_v1.as<P>(); act = d_act.as<P>();
  }
  SS_HIP(d_tcnt.alloc(sizeof(P) * ntiles));
  SS_HIP(d_tbase.alloc(sizeof(P) * ntiles));
  SS_HIP(d_temp.alloc(temp_bytes));
  Events ev;
  SS_HIP(hipEventCreate(&ev.a));
  SS_HIP(hipEventCreate(&ev.b));
  const hipStream_t st = nullptr;
  SS_HIP(hipEventRecord(ev.a, st));
  SS_HIP(hipMemsetAsync(d_text.as<uint8_t>() + (text_bytes - KJ_SS_TEXT_PAD - KJ_SS_LANE_BYTES), 0, KJ_SS_TEXT_PAD + KJ_SS_LANE_BYTES, st));
  SS_HIP(hipMemcpyAsync(d_text.p, text, tlen, hipMemcpyHostToDevice, st));
  SS_HIP(hipMemsetAsync(d_rank.p, 0, sizeof(P) * rank_entries, st));

  // ---- round 1 ----
  size_t tb = temp_bytes;
  k_ss_count<P><<<(unsigned)ntiles, KJ_SS_BLOCK, 0, st>>>(d_text.as<uint4>(), nlanes, d_tcnt.as<P>());
  SS_HIP(hipGetLastError());
  SS_HIP(rocprim::exclusive_scan(d_temp.p, tb, d_tcnt.as<P>(), d_tbase.as<P>(), (P)0, (size_t)ntiles, rocprim::plus<P>(), st));
  k_ss_keys<P><<<(unsigned)ntiles, KJ_SS_BLOCK, 0, st>>>(d_text.as<uint4>(), nlanes, tlen, nsuf, d_tbase.as<P>(), rank_bias, k0, v0, d_rank.as<P>());
  SS_HIP(hipGetLastError());

  rocprim::double_buffer<uint64_t> kb(k0, k1);
  rocprim::double_buffer<P> vb(v0, v1);
  uint64_t m = nsuf, h = 0;
  uint32_t rounds = 0;
  while (m != 0) {                                          // (a text without a suffix, kept: no round)
    const int first = rounds == 0;
    if (stats && rounds < KJ_SS_STATS_ROUNDS) stats->active[rounds] = m;
    if (!first) {
      if (!ss_round_allowed(h, maxlen)) {
        err = "internal: suffix sort on the device: " + std::to_string(m) + " suffixes still active at h = " + std::to_string(h) + " beyond the longest sequence (" +
              std::to_string(maxlen) + ")";
        return KAIJU_GPU_ERR_ARG;
      }
      k_ss_round_keys<P><<<grid_for(m), KJ_SS_BLOCK, 0, st>>>(act, m, d_rank.as<P>(), h, tlen, kb.current(), vb.current());
      SS_HIP(hipGetLastError());
    }
    const unsigned end_bit = first ? (unsigned)KJ_SS_KEY_BITS : round_bits;
    if (sort_temp<P>(m, end_bit) > temp_bytes || scan_items_temp<P>(m) > temp_bytes || scan_flags_temp<P>(m) > temp_bytes) { err = "internal: suffix sort on the device: temporary storage"; return KAIJU_GPU_ERR_ARG; }
    tb = temp_bytes;
    SS_HIP(rocprim::radix_sort_pairs(d_temp.p, tb, kb, vb, (size_t)m, 0u, end_bit, st));
    if constexpr (wide) {
      if (!first) {                                         // sorted by rank[p + h]; now, stable, by rank[p]
        k_ss_round_keys_hi<<<grid_for(m), KJ_SS_BLOCK, 0, st>>>(vb.current(), m, d_rank.as<uint64_t>(), tlen, kb.current());
        SS_HIP(hipGetLastError());
        tb = temp_bytes;
        SS_HIP(rocprim::radix_sort_pairs(d_temp.p, tb, kb, vb, (size_t)m, 0u, end_bit, st));
      }
    }
    // wide: 16-byte items from the lower of (free key buffer, active list) over both of them
    Item *items = wide ? reinterpret_cast<Item *>(std::min(reinterpret_cast<uint8_t *>(kb.alternate()), reinterpret_cast<uint8_t *>(act)))
                       : reinterpret_cast<Item *>(kb.alternate());
    P *flags = vb.alternate();
    k_ss_heads<P><<<grid_for(m), KJ_SS_BLOCK, 0, st>>>(kb.current(), vb.current(), d_rank.as<P>(), m, first, h, tlen, items);
    SS_HIP(hipGetLastError());
    tb = temp_bytes;
    SS_HIP(rocprim::inclusive_scan(d_temp.p, tb, items, items, (size_t)m, typename SsTypes<P>::Scan(), st));
    k_ss_ranks<P><<<grid_for(m), KJ_SS_BLOCK, 0, st>>>(kb.current(), vb.current(), items, m, first, first_rank, tlen, d_rank.as<P>(), flags);
    SS_HIP(hipGetLastError());
    tb = temp_bytes;
    SS_HIP(rocprim::inclusive_scan(d_temp.p, tb, flags, flags, (size_t)m, rocprim::plus<P>(), st));
    k_ss_compact<P><<<grid_for(m), KJ_SS_BLOCK, 0, st>>>(vb.current(), flags, m, act);
    SS_HIP(hipGetLastError());
    P left = 0;
    SS_HIP(hipMemcpyAsync(&left, flags + (m - 1), sizeof(P), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));                       // the one synchronisation of a round: is there another one?
    rounds++;
    h = first ? (uint64_t)KJ_SS_K : 2 * h;
    if (left > m) { err = "internal: suffix sort on the device: active count"; return KAIJU_GPU_ERR_ARG; }
    m = left;
    if (m == 0) break;
  }
  k_ss_scatter<P><<<grid_for(nlanes), KJ_SS_BLOCK, 0, st>>>(d_text.as<uint4>(), d_rank.as<P>(), nlanes, first_rank, nsuf, v0);
  SS_HIP(hipGetLastError());
  if (!keep) SS_HIP(hipMemcpyAsync(sa_out, v0, sizeof(P) * nsuf, hipMemcpyDeviceToHost, st));
  SS_HIP(hipEventRecord(ev.b, st));
  SS_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  SS_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
  if (stats) { stats->rounds = rounds; stats->ms_sort = ms; }
  if (keep) {
    keep->text = d_text.p; keep->rank = d_rank.p; keep->sa = d_v0.p; keep->k0 = d_k0.p; keep->temp = d_temp.p;
    d_text.p = d_rank.p = d_v0.p = d_k0.p = d_temp.p = nullptr;
    keep->temp_bytes = temp_bytes; keep->nseq = nseq; keep->nsuf = nsuf; keep->maxlen = maxlen; keep->bytes = need;
  }
  return KAIJU_GPU_OK;
}

}  // namespace

int kj_sufsort_check_device(int device_id, std::string &err) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { err = "suffix sort on the device: no HIP device (kaiju_build_fmi is the host builder)"; return KAIJU_GPU_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= n) { err = "suffix sort on the device: device_id " + std::to_string(device_id) + " of " + std::to_string(n) + " devices"; return KAIJU_GPU_ERR_ARG; }
  return KAIJU_GPU_OK;
}

int kj_sufsort_device(const uint8_t *text, uint64_t tlen, int device_id, uint32_t *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats,
                      std::string &err) {
  return sufsort_run<uint32_t>(text, tlen, device_id, sa_out, n_out, stats, nullptr, 0, err);
}

int kj_sufsort_device_keep(const uint8_t *text, uint64_t tlen, int device_id, uint32_t *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats,
                           SsKeep *keep, std::string &err) {
  return sufsort_run<uint32_t>(text, tlen, device_id, sa_out, n_out, stats, keep, 0, err);
}

int kj_sufsort_device_wide(const uint8_t *text, uint64_t tlen, int device_id, uint64_t *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats,
                           uint64_t rank_bias, std::string &err) {
  return sufsort_run<uint64_t>(text, tlen, device_id, sa_out, n_out, stats, nullptr, rank_bias, err);
}

uint64_t kj_sufsort_need_bytes(uint64_t tlen, uint64_t nsuf, uint64_t *temp_bytes_out) { return need_bytes<uint32_t>(tlen, nsuf, 0, temp_bytes_out); }
uint64_t kj_sufsort_need_bytes_wide(uint64_t tlen, uint64_t nsuf, uint64_t rank_bias, uint64_t *temp_bytes_out) {
  return need_bytes<uint64_t>(tlen, nsuf, rank_bias, temp_bytes_out);
}
