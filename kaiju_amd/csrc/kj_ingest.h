// kj_ingest.h — record extraction from FASTQ / FASTA text: the per-lane logic, for the device (ingest.hip) and for the
// host (tests/emu/ingest_emu.cpp drives the same functions tile by tile).
//
// The rules are those of BlockCursor::next in csrc/host/kaiju_main.cpp (the reference's reading loop, kaiju.cpp:288-386):
//   lines     a line ends at '\n'; the last one may lack it; a trailing '\n' opens no line
//   header    lines of length 0 in front of a header are skipped; the first non-empty line is a header whatever it starts with
//   name      the header without its first byte, cut at the first of " /\t\r" (not cut with keep_names)
//   FASTQ     the line behind the header is the sequence span (none: empty sequence); two more lines are skipped unseen
//   FASTA     the span runs from the end of the header line to the next line that starts with '>' (or the end of the text)
//   sequence  the bytes of the span in [A-Za-z], in order (strip(), util.cpp:25-32)
//
// Passes (every one works on independent tiles; the tiles of a pass may run in any order):
//   lines   tiles of kTileBytes bytes, 16 per lane: count the '\n' of a tile; prefix sum over the tiles; write line_start[]
//           (line i is text[line_start[i], line_start[i + 1] - 1)), note lines of length 0 and the first non-empty line
//   records FASTQ without a line of length 0: record r is lines 4r .. 4r + 3.  FASTQ otherwise: the four-state machine
//           (expect header / sequence / separator / quality) as a prefix scan over per-line transition functions.  FASTA: a
//           line is a header iff it starts with '>' or is the first non-empty line.  A prefix sum over the header flags
//           numbers the records: rec_line[r] = line of record r's header
//   spans   teams of kTeam lanes per record: letters of the span (-> off[] by a prefix sum), the name, then the copy
#ifndef KJ_INGEST_H
#define KJ_INGEST_H

#include <stdint.h>

#if defined(__HIPCC__)
#define KJI_HD __host__ __device__ __forceinline__
#else
#define KJI_HD inline
#endif

namespace kji {

constexpr uint32_t kChunk = 16;                       // bytes per lane and step: one aligned 16-byte load
constexpr uint32_t kTileLanes = 256;
constexpr uint32_t kTileBytes = kTileLanes * kChunk;  // 4096
constexpr uint32_t kScanBlock = 256;                  // elements (tiles, lines, mates) per block of a prefix scan; the one block
                                                      // on top of them walks the block sums kScanBlock at a time
constexpr uint32_t kTeam = 16;                        // lanes per record
constexpr uint64_t kMaxBytes = 0xfffffff0ull;         // positions and the sentinel bytes + 1 fit 32 bits
constexpr uint32_t kNone = 0xffffffffu;

struct alignas(16) Chunk { uint32_t w[4]; };

// 16 bytes at text + 16 * c.  The chunk holds at least one byte of the text; what lies behind the text's end inside the
// chunk is read (an aligned 16-byte granule never leaves the page of its first byte) and masked out by the caller.
KJI_HD Chunk load_chunk(const uint8_t *text, uint64_t c) { return *reinterpret_cast<const Chunk *>(text + c * kChunk); }
KJI_HD uint32_t chunk_byte(const Chunk &v, uint32_t k) { return (v.w[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// bit k set: base + k lies in [lo, hi)
KJI_HD uint32_t range_mask(uint64_t base, uint64_t lo, uint64_t hi) {
  uint32_t m = 0xffffu;
  if (lo > base) { const uint64_t d = lo - base; m = d >= kChunk ? 0u : (m << d) & 0xffffu; }
  if (hi < base + kChunk) { const uint64_t d = hi > base ? hi - base : 0; m &= (1u << d) - 1u; }
  return m;
}
// bit k set: byte k of the chunk is c
KJI_HD uint32_t eq_mask(const Chunk &v, uint32_t c) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < kChunk; k++) m |= (chunk_byte(v, k) == c ? 1u : 0u) << k;
  return m;
}
KJI_HD bool is_letter(uint32_t b) { return (uint32_t)((b | 32u) - 97u) < 26u; }      // (b >= 0x80: (b | 32) - 97 >= 63)
// bit k set: byte k of the chunk is in [A-Za-z]
KJI_HD uint32_t letter_mask(const Chunk &v) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < kChunk; k++) m |= (is_letter(chunk_byte(v, k)) ? 1u : 0u) << k;
  return m;
}
KJI_HD uint32_t popc16(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(m);
#else
  return (uint32_t)__builtin_popcount(m);
#endif
}
KJI_HD uint32_t ctz16(uint32_t m) { return (uint32_t)__builtin_ctz(m); }

// ---- lines --------------------------------------------------------------------------------------
// '\n' bytes of chunk c that belong to the text
KJI_HD uint32_t nl_mask(const uint8_t *text, uint64_t bytes, uint64_t c) {
  const uint64_t base = c * kChunk;
  if (base >= bytes) return 0;
  return eq_mask(load_chunk(text, c), '\n') & range_mask(base, 0, bytes);
}
// of those, the ones that end a line of length 0: the byte in front is a '\n' too, or there is none
KJI_HD uint32_t empty_line_mask(const uint8_t *text, uint64_t c, uint32_t nl) {
  const uint64_t base = c * kChunk;
  const uint32_t prev = (base == 0 || text[base - 1] == '\n') ? 1u : 0u;
  return nl & ((nl << 1) | prev);
}
// number of lines of a text with n_nl '\n' bytes, and the sentinel behind the last line start:
// line_start[n_lines] - 1 is the end of the last line in either case
KJI_HD uint32_t line_count(const uint8_t *text, uint64_t bytes, uint32_t n_nl, uint32_t *sentinel) {
  if (bytes == 0) { *sentinel = 0; return 0; }
  const bool closed = text[bytes - 1] == '\n';
  *sentinel = (uint32_t)(closed ? bytes : bytes + 1);
  return closed ? n_nl : n_nl + 1;
}
KJI_HD uint32_t line_len(const uint32_t *line_start, uint32_t i) { return line_start[i + 1] - 1 - line_start[i]; }

// ---- FASTQ: the four-state machine as functions on {expect header, sequence, separator, quality} --------------
// a function is four 2-bit entries, entry s in bits 2s, 2s + 1
constexpr uint32_t kFqIdent = 0xe4u;     // 0 -> 0, 1 -> 1, 2 -> 2, 3 -> 3
constexpr uint32_t kFqLine = 0x39u;      // a line of some length:  0 -> 1, 1 -> 2, 2 -> 3, 3 -> 0
constexpr uint32_t kFqEmpty = 0x38u;     // a line of length 0:     0 -> 0 (skipped), 1 -> 2, 2 -> 3, 3 -> 0
KJI_HD uint32_t fq_func(bool empty) { return empty ? kFqEmpty : kFqLine; }
KJI_HD uint32_t fq_apply(uint32_t f, uint32_t s) { return (f >> (2 * s)) & 3u; }
// first f, then g: associative, not commutative
KJI_HD uint32_t fq_compose(uint32_t f, uint32_t g) {
  uint32_t h = 0;
#pragma unroll
  for (uint32_t s = 0; s < 4; s++) h |= fq_apply(g, fq_apply(f, s)) << (2 * s);
  return h;
}
// a line met in state s opens a record iff the machine expects a header and the line is not empty
KJI_HD bool fq_is_header(uint32_t state_before, bool empty) { return state_before == 0 && !empty; }

// ---- FASTA ----------------------------------------------------------------------------------------
KJI_HD bool fa_is_header(const uint8_t *text, const uint32_t *line_start, uint32_t i, uint32_t first_nonempty) {
  if (line_len(line_start, i) == 0) return false;
  return text[line_start[i]] == '>' || i == first_nonempty;
}

// ---- records --------------------------------------------------------------------------------------
struct Span { uint64_t a, e; };          // bytes [a, e) of the text
// header line of record r without its '\n'
KJI_HD Span header_span(const uint32_t *line_start, const uint32_t *rec_line, uint32_t r) {
  const uint32_t h = rec_line[r];
  return Span{line_start[h], (uint64_t)line_start[h + 1] - 1};
}
// sequence span of record r (n_records: of the text; rec_line[r + 1] exists for r + 1 < n_records)
KJI_HD Span seq_span(const uint32_t *line_start, const uint32_t *rec_line, uint32_t r, uint32_t n_records, uint32_t n_lines,
                     uint64_t bytes, bool fastq) {
  const uint32_t h = rec_line[r];
  if (fastq) {
    if (h + 1 >= n_lines) return Span{bytes, bytes};
    return Span{line_start[h + 1], (uint64_t)line_start[h + 2] - 1};
  }
  const uint64_t a = line_start[h + 1] < bytes ? line_start[h + 1] : bytes;
  const uint64_t e = r + 1 < n_records ? line_start[rec_line[r + 1]] : bytes;
  return Span{a, e > a ? e : a};
}
KJI_HD bool name_stop(uint32_t b) { return b == ' ' || b == '/' || b == '\t' || b == '\r'; }

// a team walks a span in steps of kTeam chunks, starting at the chunk that holds its first byte
KJI_HD uint64_t span_chunks(const Span &s) { return s.e > s.a ? (s.e - (s.a & ~(uint64_t)(kChunk - 1)) + kChunk - 1) / kChunk : 0; }
// letters of chunk k of the span (k < span_chunks); *v receives the chunk
KJI_HD uint32_t span_letters(const uint8_t *text, const Span &s, uint64_t k, Chunk *v) {
  const uint64_t c = s.a / kChunk + k;
  *v = load_chunk(text, c);
  return letter_mask(*v) & range_mask(c * kChunk, s.a, s.e);
}
// the bytes of chunk v selected by m, in order, to dst; a chunk of sixteen letters goes out as it is
KJI_HD void put_letters(uint8_t *dst, const Chunk &v, uint32_t m) {
  if (m == 0xffffu) { __builtin_memcpy(dst, &v, kChunk); return; }
  while (m) { *dst++ = (uint8_t)chunk_byte(v, ctz16(m)); m &= m - 1; }
}

}  // namespace kji

// what ingest.hip offers capi_text.hip (the entry points of include/kaiju_gpu.h are defined there)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
struct kaiju_gpu_name_span;
struct kaiju_gpu_parse_info;
namespace kjl { struct Scratch; }   // kj_lines.h
// queues every pass on `stream`; grows scratch.  Returns 0, or a kaiju_gpu_status with *err set.
int kj_ingest_launch(kjl::Scratch &scratch, hipStream_t stream, const void *d_text1, uint64_t bytes1, const void *d_text2,
                     uint64_t bytes2, int fastq, int keep_names, uint32_t rec_cap, void *d_seqs, uint64_t *d_off,
                     kaiju_gpu_name_span *d_names, kaiju_gpu_parse_info *d_info, const char **err);
#endif

#endif  // KJ_INGEST_H
