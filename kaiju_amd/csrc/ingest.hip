// ingest.hip — FASTQ / FASTA text to the buffers of kaiju_gpu_classify_batch_device (gfx950, wave64): the passes of
// kj_ingest.h as kernels.  Nothing here walks the text serially; the host never learns a count while the passes are queued,
// so every kernel behind the first sizes itself from counts in device memory (grid-stride over lines / records) and the
// scratch is sized for the worst case (a text of nothing but '\n': one line per byte).
//
//   k_ing_init          counters of both texts
//   k_ing_lines_count   '\n' per tile                          k_ing_top_u32   prefix sum over block sums, one block
//   k_ing_lines_fill    line_start[], lines of length 0, first non-empty line, number of lines
//   k_ing_rec_fast      FASTQ without a line of length 0: rec_line[r] = 4r
//   k_ing_fq_func / k_ing_fq_top / k_ing_fq_flag   FASTQ otherwise: scan of the transition functions, header flags
//   k_ing_fa_flag       FASTA: header flags
//   k_ing_rec_scatter   rec_line[] from the prefix sum over the header flags
//   k_ing_span_len      per record: letters of the span(s), the name, the name comparison of pairs, longest mate
//   kjl::k_scan_sums / k_scan_top / k_scan_apply <IngMates>   off[] = prefix sum of the mate lengths (64 bit; kj_lines.h)
//   k_ing_span_copy     the letters to seqs + off[..]
//   k_ing_finish        kaiju_gpu_parse_info, by one lane with ordinary stores
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/kaiju_gpu.h"
#include "kj_ingest.h"
#include "kj_lines.h"

using namespace kji;
using kjs::OpAdd32;
using kjs::block_scan_excl;

namespace {

constexpr int kIngBlock = 256;
static_assert(kIngBlock == (int)kTileLanes && kIngBlock == (int)kScanBlock && kIngBlock == kjs::kScanLanes,
              "one lane per chunk of a tile / element of a scan block");

struct IngHdr { uint32_t n_lines, any_empty, first_nonempty, n_records; };
struct IngShared { uint32_t max_mate_len, name_mismatch; };

struct IngFile {
  const uint8_t *text;
  uint64_t bytes;
  uint32_t n_tiles;
  uint32_t *tile_cnt, *tile_base;      // n_tiles, n_tiles + 1
  uint32_t *line_start;                // bytes + 2
  uint8_t *lflag;                      // bytes + 1: 1 = the line is a header
  uint32_t *blk, *blk_base;            // per block of kScanBlock lines (+ 1)
  uint32_t *rec_line;                  // rec_cap + 1
  IngHdr *hdr;
};

struct IngRec {
  IngFile f1, f2;
  int paired, fastq, keep_names;
  uint32_t rec_cap;
  uint32_t *mlen;                      // 2 * rec_cap
  uint64_t *oblk, *oblk_base;          // per block of kScanBlock mates (+ 1)
  IngShared *sh;
  uint8_t *seqs;
  uint64_t *off;
  kaiju_gpu_name_span *names;
  kaiju_gpu_parse_info *info;
};

struct OpFq { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return fq_compose(a, b); } };

__global__ void k_ing_init(IngHdr *h1, IngHdr *h2, IngShared *sh) {
  if (blockIdx.x || threadIdx.x) return;
  *h1 = IngHdr{0, 0, kNone, 0};
  *h2 = IngHdr{0, 0, kNone, 0};
  *sh = IngShared{0, kNone};
}

__global__ __launch_bounds__(kIngBlock) void k_ing_lines_count(IngFile f) {
  const uint64_t c = (uint64_t)blockIdx.x * kTileLanes + threadIdx.x;
  uint32_t tot;
  block_scan_excl<uint32_t>(popc16(nl_mask(f.text, f.bytes, c)), 0u, &tot, OpAdd32());
  if (threadIdx.x == 0) f.tile_cnt[blockIdx.x] = tot;
}

// out[i] = in[0] + .. + in[i - 1] for i <= n, by one block.  n = n_host, or the blocks of kScanBlock that *n_elems elements
// make.  need_flag: nothing happens unless *need_flag is set (passes of the FASTQ state machine).
__global__ __launch_bounds__(kIngBlock) void k_ing_top_u32(const uint32_t *in, uint32_t *out, uint32_t n_host, const uint32_t *n_elems,
                                                           uint32_t *total_out, const uint32_t *need_flag) {
  if (need_flag && !*need_flag) return;
  const uint32_t n = n_elems ? (*n_elems + kScanBlock - 1) / kScanBlock : n_host;
  uint32_t carry = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kIngBlock) {
    const uint32_t i = i0 + threadIdx.x;
    uint32_t tot;
    const uint32_t ex = block_scan_excl<uint32_t>(i < n ? in[i] : 0u, 0u, &tot, OpAdd32());
    if (i < n) out[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) { out[n] = carry; if (total_out) *total_out = carry; }
}

__global__ __launch_bounds__(kIngBlock) void k_ing_lines_fill(IngFile f) {
  __shared__ uint32_t s_min, s_any;
  if (threadIdx.x == 0) { s_min = kNone; s_any = 0; }
  const uint64_t c = (uint64_t)blockIdx.x * kTileLanes + threadIdx.x;
  uint32_t m = nl_mask(f.text, f.bytes, c);
  uint32_t tot;
  const uint32_t ex = block_scan_excl<uint32_t>(popc16(m), 0u, &tot, OpAdd32());   // (its barriers order the init above)
  if (m) {
    const uint32_t empty = empty_line_mask(f.text, c, m);
    uint32_t j = f.tile_base[blockIdx.x] + ex, first = kNone;      // the line that ends at the next '\n'
    for (uint32_t mm = m; mm; mm &= mm - 1, j++) {
      const uint32_t k = ctz16(mm);
      f.line_start[j + 1] = (uint32_t)(c * kChunk + k + 1);
      if (!((empty >> k) & 1u) && first == kNone) first = j;
    }
    if (empty) atomicOr(&s_any, 1u);
    if (first != kNone) atomicMin(&s_min, first);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_any) atomicOr(&f.hdr->any_empty, 1u);
    if (s_min != kNone) atomicMin(&f.hdr->first_nonempty, s_min);
    if (blockIdx.x == 0) {
      uint32_t sentinel;
      const uint32_t n_lines = line_count(f.text, f.bytes, f.tile_base[f.n_tiles], &sentinel);
      f.line_start[0] = 0;
      f.line_start[n_lines] = sentinel;                            // (a text that ends in '\n': the value the last '\n' gives too)
      f.hdr->n_lines = n_lines;
      if (f.bytes && f.text[f.bytes - 1] != '\n') atomicMin(&f.hdr->first_nonempty, n_lines - 1);   // the open last line has bytes
    }
  }
}

__global__ __launch_bounds__(kIngBlock) void k_ing_rec_fast(IngFile f, uint32_t rec_cap) {
  if (f.hdr->any_empty) return;
  const uint32_t n = (f.hdr->n_lines + 3) / 4;
  const uint32_t lim = n < rec_cap ? n : rec_cap;
  for (uint32_t r = blockIdx.x * kIngBlock + threadIdx.x; r < lim; r += gridDim.x * kIngBlock) f.rec_line[r] = 4 * r;
  if (blockIdx.x == 0 && threadIdx.x == 0) f.hdr->n_records = n;
}

__global__ __launch_bounds__(kIngBlock) void k_ing_fq_func(IngFile f) {
  if (!f.hdr->any_empty) return;
  const uint32_t L = f.hdr->n_lines, nb = (L + kScanBlock - 1) / kScanBlock;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint32_t i = b * kScanBlock + threadIdx.x;
    uint32_t tot;
    block_scan_excl<uint32_t>(i < L ? fq_func(line_len(f.line_start, i) == 0) : kFqIdent, kFqIdent, &tot, OpFq());
    if (threadIdx.x == 0) f.blk[b] = tot;
  }
}

// state of the machine at the first line of every block
__global__ __launch_bounds__(kIngBlock) void k_ing_fq_top(IngFile f) {
  if (!f.hdr->any_empty) return;
  const uint32_t nb = (f.hdr->n_lines + kScanBlock - 1) / kScanBlock;
  uint32_t carry = kFqIdent;
  for (uint32_t i0 = 0; i0 < nb; i0 += kIngBlock) {
    const uint32_t i = i0 + threadIdx.x;
    uint32_t tot;
    const uint32_t ex = block_scan_excl<uint32_t>(i < nb ? f.blk[i] : kFqIdent, kFqIdent, &tot, OpFq());
    if (i < nb) f.blk_base[i] = fq_apply(fq_compose(carry, ex), 0);
    carry = fq_compose(carry, tot);
  }
}

__global__ __launch_bounds__(kIngBlock) void k_ing_fq_flag(IngFile f) {
  if (!f.hdr->any_empty) return;
  const uint32_t L = f.hdr->n_lines, nb = (L + kScanBlock - 1) / kScanBlock;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint32_t i = b * kScanBlock + threadIdx.x;
    const bool empty = i < L && line_len(f.line_start, i) == 0;
    uint32_t tot;
    const uint32_t ex = block_scan_excl<uint32_t>(i < L ? fq_func(empty) : kFqIdent, kFqIdent, &tot, OpFq());
    const bool h = i < L && fq_is_header(fq_apply(ex, f.blk_base[b]), empty);
    if (i < L) f.lflag[i] = h ? 1 : 0;
    const int cnt = __syncthreads_count(h);
    if (threadIdx.x == 0) f.blk[b] = (uint32_t)cnt;       // (k_ing_fq_top has read the functions that stood here)
    __syncthreads();
  }
}

__global__ __launch_bounds__(kIngBlock) void k_ing_fa_flag(IngFile f) {
  const uint32_t L = f.hdr->n_lines, nb = (L + kScanBlock - 1) / kScanBlock, first = f.hdr->first_nonempty;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint32_t i = b * kScanBlock + threadIdx.x;
    const bool h = i < L && fa_is_header(f.text, f.line_start, i, first);
    if (i < L) f.lflag[i] = h ? 1 : 0;
    const int cnt = __syncthreads_count(h);
    if (threadIdx.x == 0) f.blk[b] = (uint32_t)cnt;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kIngBlock) void k_ing_rec_scatter(IngFile f, uint32_t rec_cap, int fastq) {
  if (fastq && !f.hdr->any_empty) return;
  const uint32_t L = f.hdr->n_lines, nb = (L + kScanBlock - 1) / kScanBlock;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint32_t i = b * kScanBlock + threadIdx.x;
    const uint32_t h = i < L ? f.lflag[i] : 0u;
    uint32_t tot;
    const uint32_t r = f.blk_base[b] + block_scan_excl<uint32_t>(h, 0u, &tot, OpAdd32());
    if (h && r <= rec_cap) f.rec_line[r] = i;             // (rec_line[rec_cap]: where the span of the last record held ends)
  }
}

// ---- records: teams of kTeam lanes ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t team_lane() { return threadIdx.x & (kTeam - 1); }
__device__ __forceinline__ uint32_t team_ballot(bool p) {
  return (uint32_t)(__ballot(p) >> (threadIdx.x & 63u & ~(kTeam - 1))) & 0xffffu;
}
__device__ __forceinline__ uint32_t team_sum(uint32_t v) {
#pragma unroll
  for (int d = 1; d < (int)kTeam; d <<= 1) v += __shfl_xor(v, d, kTeam);
  return v;
}
__device__ __forceinline__ uint32_t emitted(const IngRec &R, uint32_t *n1, uint32_t *n2) {
  *n1 = R.f1.hdr->n_records;
  *n2 = R.paired ? R.f2.hdr->n_records : *n1;
  const uint32_t n = *n1 < *n2 ? *n1 : *n2;
  return n < R.rec_cap ? n : R.rec_cap;
}

__device__ uint32_t team_count_letters(const uint8_t *text, const Span &s) {
  const uint64_t nc = span_chunks(s);
  uint32_t cnt = 0;
  for (uint64_t k = team_lane(); k < nc; k += kTeam) { Chunk v; cnt += popc16(span_letters(text, s, k, &v)); }
  return team_sum(cnt);
}

// name of the record whose header line is h: the line without its first byte, cut at the first of " /\t\r"
__device__ kaiju_gpu_name_span team_name(const uint8_t *text, const Span &h, int keep_names) {
  const uint64_t pos = h.a + 1;
  const uint32_t maxlen = (uint32_t)(h.e - pos);
  uint32_t len = maxlen;
  if (!keep_names)
    for (uint32_t base = 0; base < maxlen; base += kTeam) {
      const uint32_t i = base + team_lane();
      const uint32_t hit = team_ballot(i < maxlen && name_stop(text[pos + i]));
      if (hit) { len = base + ctz16(hit); break; }
    }
  return kaiju_gpu_name_span{(uint32_t)pos, len};
}

__global__ __launch_bounds__(kIngBlock) void k_ing_span_len(IngRec R) {
  uint32_t n1, n2;
  const uint32_t n = emitted(R, &n1, &n2);
  const uint32_t teams = gridDim.x * (kIngBlock / kTeam);
  uint32_t lmax = 0;
  for (uint32_t r = (blockIdx.x * kIngBlock + threadIdx.x) / kTeam; r < n; r += teams) {
    const IngFile &a = R.f1;
    const uint32_t c1 = team_count_letters(a.text, seq_span(a.line_start, a.rec_line, r, n1, a.hdr->n_lines, a.bytes, R.fastq != 0));
    const kaiju_gpu_name_span nm1 = team_name(a.text, header_span(a.line_start, a.rec_line, r), R.keep_names);
    uint32_t c2 = 0;
    if (R.paired) {
      const IngFile &b = R.f2;
      c2 = team_count_letters(b.text, seq_span(b.line_start, b.rec_line, r, n2, b.hdr->n_lines, b.bytes, R.fastq != 0));
      const kaiju_gpu_name_span nm2 = team_name(b.text, header_span(b.line_start, b.rec_line, r), R.keep_names);
      bool diff = nm1.len != nm2.len;
      if (!diff)
        for (uint32_t i = team_lane(); i < nm1.len; i += kTeam) diff |= a.text[nm1.pos + i] != b.text[nm2.pos + i];
      if (team_ballot(diff) && team_lane() == 0) atomicMin(&R.sh->name_mismatch, r);
    }
    if (team_lane() == 0) { R.mlen[2 * (size_t)r] = c1; R.mlen[2 * (size_t)r + 1] = c2; R.names[r] = nm1; }
    lmax = max(lmax, max(c1, c2));
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) lmax = max(lmax, (uint32_t)__shfl_xor(lmax, d, 64));
  if ((threadIdx.x & 63) == 0 && lmax) atomicMax(&R.sh->max_mate_len, lmax);
}

// elements of the scan that makes off[]: the mates of the records emitted
struct IngMates {
  IngRec R;
  __device__ uint64_t operator()() const { uint32_t n1, n2; return 2 * (uint64_t)emitted(R, &n1, &n2); }
};

__device__ void team_copy_letters(const uint8_t *text, const Span &s, uint8_t *dst) {
  const uint64_t nc = span_chunks(s);
  const uint32_t tl = team_lane();
  uint64_t run = 0;
  for (uint64_t k0 = 0; k0 < nc; k0 += kTeam) {
    const uint64_t k = k0 + tl;
    Chunk v{};
    const uint32_t m = k < nc ? span_letters(text, s, k, &v) : 0u;
    uint32_t x = popc16(m);
#pragma unroll
    for (int d = 1; d < (int)kTeam; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, kTeam);
      if ((int)tl >= d) x += y;
    }
    const uint32_t tot = __shfl(x, kTeam - 1, kTeam);
    if (m) put_letters(dst + run + (x - popc16(m)), v, m);
    run += tot;
  }
}

__global__ __launch_bounds__(kIngBlock) void k_ing_span_copy(IngRec R) {
  uint32_t n1, n2;
  const uint32_t n = emitted(R, &n1, &n2);
  const uint32_t teams = gridDim.x * (kIngBlock / kTeam);
  for (uint32_t r = (blockIdx.x * kIngBlock + threadIdx.x) / kTeam; r < n; r += teams) {
    const IngFile &a = R.f1;
    team_copy_letters(a.text, seq_span(a.line_start, a.rec_line, r, n1, a.hdr->n_lines, a.bytes, R.fastq != 0), R.seqs + R.off[2 * (size_t)r]);
    if (R.paired) {
      const IngFile &b = R.f2;
      team_copy_letters(b.text, seq_span(b.line_start, b.rec_line, r, n2, b.hdr->n_lines, b.bytes, R.fastq != 0), R.seqs + R.off[2 * (size_t)r + 1]);
    }
  }
}

__global__ void k_ing_finish(IngRec R) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t n1, n2;
  const uint32_t n = emitted(R, &n1, &n2);
  kaiju_gpu_parse_info o;
  o.n_records = n1;
  o.n_records2 = R.paired ? n2 : 0;
  o.max_mate_len = R.sh->max_mate_len;
  o.name_mismatch = R.sh->name_mismatch;
  o.seq_bytes = R.off[2 * (size_t)n];
  o.overflow = (n1 < n2 ? n1 : n2) > R.rec_cap ? 1u : 0u;
  o.reserved = 0;
  *R.info = o;
}

// ---- host side: scratch and the queue of passes ----------------------------------------------------------------------
void carve_file(kjl::Carver &c, IngFile &f, const void *text, uint64_t bytes, uint32_t rec_cap) {
  f.text = static_cast<const uint8_t *>(text);
  f.bytes = bytes;
  f.n_tiles = (uint32_t)((bytes + kTileBytes - 1) / kTileBytes);
  const size_t nblk = (size_t)((bytes + 1) / kScanBlock + 2);
  f.tile_cnt = c.take<uint32_t>(f.n_tiles + 1);
  f.tile_base = c.take<uint32_t>(f.n_tiles + 1);
  f.line_start = c.take<uint32_t>(bytes + 2);
  f.lflag = c.take<uint8_t>(bytes + 1);
  f.blk = c.take<uint32_t>(nblk);
  f.blk_base = c.take<uint32_t>(nblk + 1);
  f.rec_line = c.take<uint32_t>((size_t)rec_cap + 1);
  f.hdr = c.take<IngHdr>(1);
}
void carve(kjl::Carver &c, IngRec &R, const void *t1, uint64_t b1, const void *t2, uint64_t b2, uint32_t rec_cap) {
  carve_file(c, R.f1, t1, b1, rec_cap);
  carve_file(c, R.f2, t2, b2, rec_cap);
  const size_t nblk = (2 * (size_t)rec_cap) / kScanBlock + 2;
  R.mlen = c.take<uint32_t>(2 * (size_t)rec_cap + 1);
  R.oblk = c.take<uint64_t>(nblk);
  R.oblk_base = c.take<uint64_t>(nblk + 1);
  R.sh = c.take<IngShared>(1);
}
}  // namespace

int kj_ingest_launch(kjl::Scratch &scratch, hipStream_t s, const void *d_text1, uint64_t bytes1, const void *d_text2,
                     uint64_t bytes2, int fastq, int keep_names, uint32_t rec_cap, void *d_seqs, uint64_t *d_off,
                     kaiju_gpu_name_span *d_names, kaiju_gpu_parse_info *d_info, const char **err) {
  *err = "";
  const bool paired = d_text2 != nullptr;
  if (!d_off || !d_info || (!d_text1 && bytes1) || (!paired && bytes2) || (rec_cap && !d_names) || (bytes1 + bytes2 && !d_seqs)) {
    *err = "NULL argument";
    return KAIJU_GPU_ERR_ARG;
  }
  if (bytes1 > kMaxBytes || bytes2 > kMaxBytes || rec_cap > 0x7ffffff0u) { *err = "a block of text must be below 2^32 bytes"; return KAIJU_GPU_ERR_ARG; }
  if (((uintptr_t)d_text1 | (uintptr_t)d_text2) & (kChunk - 1)) { *err = "text pointers must be 16-byte aligned"; return KAIJU_GPU_ERR_ARG; }
  IngRec R{};
  kjl::Carver measure{nullptr};
  carve(measure, R, d_text1, bytes1, d_text2, bytes2, rec_cap);
  if (int rc = scratch.reserve(measure.at, 256, "hipMalloc of the ingest scratch", err)) return rc;
  kjl::Carver c{static_cast<uint8_t *>(scratch.p)};
  carve(c, R, d_text1, bytes1, d_text2, bytes2, rec_cap);
  R.paired = paired ? 1 : 0; R.fastq = fastq ? 1 : 0; R.keep_names = keep_names ? 1 : 0; R.rec_cap = rec_cap;
  R.seqs = static_cast<uint8_t *>(d_seqs); R.off = d_off; R.names = d_names; R.info = d_info;

  const dim3 blk(kIngBlock);
  hipLaunchKernelGGL(k_ing_init, dim3(1), dim3(64), 0, s, R.f1.hdr, R.f2.hdr, R.sh);
  for (int which = 0; which < (paired ? 2 : 1); which++) {
    const IngFile &f = which ? R.f2 : R.f1;
    // blocks for the passes over lines: how many there are is known on the device only
    const dim3 lgrid((unsigned)std::min<uint64_t>(4096, (f.bytes + 1 + kScanBlock - 1) / kScanBlock));
    if (f.n_tiles) hipLaunchKernelGGL(k_ing_lines_count, dim3(f.n_tiles), blk, 0, s, f);
    hipLaunchKernelGGL(k_ing_top_u32, dim3(1), blk, 0, s, f.tile_cnt, f.tile_base, f.n_tiles, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(k_ing_lines_fill, dim3(std::max(1u, f.n_tiles)), blk, 0, s, f);
    if (fastq) {
      hipLaunchKernelGGL(k_ing_rec_fast, dim3((unsigned)std::min<uint64_t>(1024, (uint64_t)rec_cap / kIngBlock + 1)), blk, 0, s, f, rec_cap);
      hipLaunchKernelGGL(k_ing_fq_func, lgrid, blk, 0, s, f);
      hipLaunchKernelGGL(k_ing_fq_top, dim3(1), blk, 0, s, f);
      hipLaunchKernelGGL(k_ing_fq_flag, lgrid, blk, 0, s, f);
      hipLaunchKernelGGL(k_ing_top_u32, dim3(1), blk, 0, s, f.blk, f.blk_base, 0u, &f.hdr->n_lines, &f.hdr->n_records, &f.hdr->any_empty);
    } else {
      hipLaunchKernelGGL(k_ing_fa_flag, lgrid, blk, 0, s, f);
      hipLaunchKernelGGL(k_ing_top_u32, dim3(1), blk, 0, s, f.blk, f.blk_base, 0u, &f.hdr->n_lines, &f.hdr->n_records, nullptr);
    }
    hipLaunchKernelGGL(k_ing_rec_scatter, lgrid, blk, 0, s, f, rec_cap, fastq ? 1 : 0);
  }
  const dim3 tgrid((unsigned)std::min<uint64_t>(8192, (uint64_t)rec_cap / (kIngBlock / kTeam) + 1));
  const dim3 ogrid((unsigned)std::min<uint64_t>(2048, (2 * (uint64_t)rec_cap) / kScanBlock + 1));
  hipLaunchKernelGGL(k_ing_span_len, tgrid, blk, 0, s, R);
  kjl::launch_offsets(s, ogrid, IngMates{R}, R.mlen, R.oblk, R.oblk_base, R.off);
  hipLaunchKernelGGL(k_ing_span_copy, tgrid, blk, 0, s, R);
  hipLaunchKernelGGL(k_ing_finish, dim3(1), dim3(64), 0, s, R);
  if (hipGetLastError() != hipSuccess) { *err = "a kernel of the ingest passes could not be launched"; return KAIJU_GPU_ERR_HIP; }
  return KAIJU_GPU_OK;
}
