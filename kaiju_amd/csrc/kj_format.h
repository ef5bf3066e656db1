// kj_format.h — 16-byte records to the lines of the output file: the per-lane logic, for the device (format.hip) and for the
// host (tests/emu/format_emu.cpp drives the same functions work unit by work unit).
//
// The rules are those of stage 4 of csrc/host/kaiju_main.cpp for kaiju / kaiju-multi without -v:
//   decision  kaiju_finalize_compact's (taxonomy.cpp): a read is classified iff (info & 255) != 0, best != 0, in Greedy mode
//             with use_evalue !(Evalue > min_evalue), and lca > 0.  The taxon of a read that is not classified is 0
//   E-value   db_length * query_len * pow(2, -bitscore) in double, the products in that order.  query_len is
//             (double)len1 / 3.0 (+ (double)len2 / 3.0 for pairs; (double)len1 for protein input), every operation correctly
//             rounded and none contracted.  pow(2, -bitscore) depends on nothing but the integer `best`: the host tabulates
//             it for best < kPowK with its own pow (pow_factor below: the expression of taxonomy.cpp) and the device reads the
//             table, so no second implementation of pow exists.  The table stands for every score only if the factor of
//             every best >= kPowK is exactly +0.0; build_pow_table checks that and the callers refuse to go on otherwise
//             (the factor underflows to +0.0 near best = 2340)
//   line      "C\t" name "\t" taxon "\n" for a classified read, "U\t" name "\t0\n" for any other: 2 + name_len + 1 + digits + 1
//   name      text1[names[r].pos, + names[r].len), byte for byte (a span that leaves the text is cut at its end)
//   number    a uint64 in decimal, 1 to 20 digits, no leading zeros; no division by a variable
//
// Passes (every one works on independent units; the units of a pass may run in any order):
//   lengths   per record: the decision (the taxon to print, 0 = 'U') and the length of the line
//   offsets   64-bit exclusive prefix sum of the lengths in blocks of kScanBlock: line_off[0 .. n], line_off[n] = the text's size
//   write     per 16 aligned bytes of the output: the record that covers the first byte by a search in line_off[] (a block of
//             kBlockLanes such chunks first narrows the search to the records its 4096 bytes touch), then byte by byte through
//             the lines that follow.  A line is written iff it ends at or in front of out_cap: a chunk that lies inside such
//             lines goes out as one aligned 16-byte store, the chunk at the end of the text or at the edge of the capacity
//             byte by byte, so no byte at or behind out_cap (or behind the text) is touched
//   finish    kaiju_gpu_format_info
#ifndef KJ_FORMAT_H
#define KJ_FORMAT_H

#include <stdint.h>

#include "../../include/kaiju_gpu.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KJF_HD __host__ __device__ __forceinline__
#else
#define KJF_HD inline
#endif

namespace kjf {

constexpr uint32_t kChunk = 16;                          // bytes of output per lane and step: one aligned 16-byte store
constexpr uint32_t kBlockLanes = 256;
constexpr uint32_t kBlockBytes = kBlockLanes * kChunk;   // 4096
constexpr uint32_t kScanBlock = 256;                     // records per block of the prefix sum
constexpr uint32_t kPowK = 4096;                         // entries of the table of pow(2, -bitscore)
constexpr uint64_t kMaxBytes = 0xffffffe0ull;            // of text 1: name_len + 24 fits 32 bits
constexpr uint32_t kMaxRecords = 0x7ffffff0u;
constexpr uint32_t kLineExtra = 24;                      // a line is at most its name + "C\t" "\t" 20 digits "\n"

struct Params {
  double db_length, min_evalue;
  int32_t gate;                                          // Greedy mode with use_evalue
  int32_t protein, paired;
  uint32_t pad;
};

struct alignas(16) Chunk { uint32_t w[4]; };

// ---- the E-value gate -------------------------------------------------------------------------------
KJF_HD double mul_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
KJF_HD double add_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}
KJF_HD double div_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}
KJF_HD double query_len(uint64_t len1, uint64_t len2, const Params &P) {
  double q = div_rn(static_cast<double>(len1), 3.0);
  if (P.paired) q = add_rn(q, div_rn(static_cast<double>(len2), 3.0));
  if (P.protein) q = static_cast<double>(len1);
  return q;
}
KJF_HD double evalue(uint32_t best, uint64_t len1, uint64_t len2, const Params &P, const double *pw) {
  const double factor = best < kPowK ? pw[best] : 0.0;
  return mul_rn(mul_rn(P.db_length, query_len(len1, len2, P)), factor);
}
// the taxon the line of record h shows: 0 = not classified
KJF_HD uint64_t decide(const kaiju_gpu_compact &h, uint64_t len1, uint64_t len2, const Params &P, const double *pw) {
  if ((h.info & 255u) == 0 || h.best == 0) return 0;
  if (P.gate && evalue(h.best, len1, len2, P, pw) > P.min_evalue) return 0;
  return h.lca;
}

// ---- the number -------------------------------------------------------------------------------------
KJF_HD uint32_t digits_u64(uint64_t v) {
  uint32_t d = 1;
  uint64_t p = 10;
#pragma unroll
  for (uint32_t k = 1; k < 20; k++) {
    if (v >= p) d = k + 1;
    if (k < 19) p *= 10;
  }
  return d;
}
// the twenty decimal digits of v, four bits each: digit j (of 10^j) in bits 4j .. 4j + 3 of lo (j < 16) or of hi
struct Bcd { uint64_t lo; uint32_t hi; };
KJF_HD Bcd to_bcd(uint64_t v) {
  Bcd b{0, 0};
#pragma unroll
  for (uint32_t j = 0; j < 20; j++) {
    const uint64_t q = v / 10;
    const uint64_t d = v - q * 10;
    if (j < 16) b.lo |= d << (4 * j); else b.hi |= (uint32_t)d << (4 * (j - 16));
    v = q;
  }
  return b;
}
KJF_HD uint32_t bcd_digit(const Bcd &b, uint32_t j) { return j < 16 ? (uint32_t)(b.lo >> (4 * j)) & 15u : (b.hi >> (4 * (j - 16))) & 15u; }

// ---- lengths ----------------------------------------------------------------------------------------
KJF_HD kaiju_gpu_name_span name_of(const kaiju_gpu_name_span *names, uint32_t r, uint64_t bytes1) {
  kaiju_gpu_name_span s = names[r];
  if (s.pos > bytes1) { s.pos = (uint32_t)bytes1; s.len = 0; }
  if (s.len > bytes1 - s.pos) s.len = (uint32_t)(bytes1 - s.pos);
  return s;
}
KJF_HD uint32_t line_len(uint32_t name_len, uint32_t digits) { return 2 + name_len + 1 + digits + 1; }
// length of the line of record r; *taxon: what pass `write` prints (0: a 'U' line)
KJF_HD uint32_t record_line(const kaiju_gpu_compact *recs, const uint64_t *off, const kaiju_gpu_name_span *names, uint32_t r, uint64_t bytes1,
                            const Params &P, const double *pw, uint64_t *taxon) {
  const uint64_t a = off[2 * (uint64_t)r], b = off[2 * (uint64_t)r + 1], c = off[2 * (uint64_t)r + 2];
  const uint64_t t = decide(recs[r], b - a, c - b, P, pw);
  *taxon = t;
  return line_len(name_of(names, r, bytes1).len, digits_u64(t));
}

// ---- write ------------------------------------------------------------------------------------------
// the largest r in [lo, hi) with line_off[r] <= o (line_off[lo] <= o; lines are never empty, so line_off[] rises strictly)
KJF_HD uint32_t find_record(const uint64_t *line_off, uint32_t lo, uint32_t hi, uint64_t o) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (line_off[mid] <= o) lo = mid; else hi = mid;
  }
  return lo;
}
// the records the bytes of block b of the output touch: [*r_lo, *r_hi).  lim: bytes the pass writes at most (> b * kBlockBytes)
KJF_HD void block_records(const uint64_t *line_off, uint32_t n, uint64_t b, uint64_t lim, uint32_t *r_lo, uint32_t *r_hi) {
  const uint64_t o0 = b * kBlockBytes, o1 = o0 + kBlockBytes < lim ? o0 + kBlockBytes : lim;
  *r_lo = find_record(line_off, 0, n, o0);
  *r_hi = find_record(line_off, 0, n, o1 - 1) + 1;
}
struct Line {
  uint64_t off, taxon;
  uint32_t len, name_pos, name_len, digits;
  Bcd bcd;
  bool fits;
};
KJF_HD Line load_line(const uint64_t *line_off, const uint64_t *tax, const kaiju_gpu_name_span *names, uint32_t r, uint64_t bytes1, uint64_t out_cap) {
  Line L;
  const uint64_t next = line_off[r + 1];
  const kaiju_gpu_name_span s = name_of(names, r, bytes1);
  L.off = line_off[r];
  L.len = (uint32_t)(next - L.off);
  L.taxon = tax[r];
  L.name_pos = s.pos; L.name_len = s.len;
  L.digits = L.len - s.len - 4;
  L.bcd = L.taxon ? to_bcd(L.taxon) : Bcd{0, 0};
  L.fits = next <= out_cap;
  return L;
}
// byte p of the line (p < L.len)
KJF_HD uint32_t line_byte(const uint8_t *text, const Line &L, uint32_t p) {
  if (p == 0) return L.taxon ? 'C' : 'U';
  if (p == 1) return '\t';
  p -= 2;
  if (p < L.name_len) return text[(uint64_t)L.name_pos + p];
  p -= L.name_len;
  if (p == 0) return '\t';
  p -= 1;
  if (p < L.digits) return '0' + bcd_digit(L.bcd, L.digits - 1 - p);
  return '\n';
}
// the bytes of chunk c of the output (bytes [16 c, 16 c + 16) of a text of `total` bytes); r_lo, r_hi: block_records of the
// chunk's block.  Returns the mask of the bytes to write: those of lines that end at or in front of out_cap
KJF_HD uint32_t format_chunk(uint64_t c, const uint8_t *text, uint64_t bytes1, const kaiju_gpu_name_span *names, const uint64_t *line_off,
                             const uint64_t *tax, uint32_t r_lo, uint32_t r_hi, uint64_t total, uint64_t out_cap, Chunk *v) {
  const uint64_t o = c * kChunk;
  *v = Chunk{{0, 0, 0, 0}};
  if (o >= total) return 0;
  uint32_t r = find_record(line_off, r_lo, r_hi, o);
  Line L = load_line(line_off, tax, names, r, bytes1, out_cap);
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < kChunk; k++) {
    const uint64_t pos = o + k;
    if (pos >= total) break;
    if (pos - L.off >= L.len) L = load_line(line_off, tax, names, ++r, bytes1, out_cap);
    if (L.fits) {
      v->w[k >> 2] |= line_byte(text, L, (uint32_t)(pos - L.off)) << (8 * (k & 3));
      m |= 1u << k;
    }
  }
  return m;
}
// out: 16-byte aligned
KJF_HD void store_chunk(uint8_t *out, uint64_t c, const Chunk &v, uint32_t m) {
  uint8_t *dst = out + c * kChunk;
  if (m == 0xffffu) { *reinterpret_cast<Chunk *>(dst) = v; return; }
#pragma unroll
  for (uint32_t k = 0; k < kChunk; k++)
    if ((m >> k) & 1u) dst[k] = (uint8_t)(v.w[k >> 2] >> (8 * (k & 3)));
}

// ---- finish -----------------------------------------------------------------------------------------
KJF_HD kaiju_gpu_format_info make_info(uint64_t total, uint32_t n, uint32_t n_classified, uint32_t n_inexact, uint64_t out_cap) {
  kaiju_gpu_format_info o;
  o.text_bytes = total;
  o.n_records = n;
  o.n_classified = n_classified;
  o.overflow = total > out_cap ? 1u : 0u;
  o.n_inexact = n_inexact;
  return o;
}

}  // namespace kjf

// ---- host only: the table of pow(2, -bitscore) ------------------------------------------------------------------------
#include <math.h>
namespace kjf {
// the factor of the E-value that depends on the score: the expression of kaiju_finalize_compact (taxonomy.cpp), with its pow
inline double pow_factor(uint32_t best) {
  const double LN_2 = 0.6931471805, LAMBDA = 0.3176, LN_K = -2.009915479;   // ConsumerThread.hpp:41-44
  const double bitscore = (LAMBDA * best - LN_K) / LN_2;
  return pow(2, -1 * bitscore);
}
inline bool is_plus_zero(double x) { return x == 0.0 && !signbit(x); }
// pw[0 .. k).  false: a score at or beyond k has a factor other than +0.0 and the table must not be used.  The factor falls
// as best rises, so once it has reached +0.0 it stays there: the first entries behind the table, every power of two up to
// 2^31 and the largest score are looked at
inline bool build_pow_table(double *pw, uint32_t k) {
  for (uint32_t b = 0; b < k; b++) pw[b] = pow_factor(b);
  bool ok = k > 0 && is_plus_zero(pw[k - 1]);
  for (uint32_t b = k; b < k + 64 && b >= k; b++) ok = ok && is_plus_zero(pow_factor(b));
  for (uint32_t b = 1; b; b <<= 1) if (b >= k) ok = ok && is_plus_zero(pow_factor(b));
  return ok && is_plus_zero(pow_factor(0xffffffffu));
}
}  // namespace kjf

// what format.hip offers capi_text.hip (the entry points of include/kaiju_gpu.h are defined there)
#if defined(__HIPCC__)
namespace kjl { struct Lines; }   // kj_lines.h: what a formatter keeps between calls
// queues every pass on `stream`; grows st.mem, and leaves in st.written the device address of the number of bytes the passes
// write (= text_bytes unless it overflows).  d_pw: the table of build_pow_table on the device.  Returns 0, or a
// kaiju_gpu_status with *err set.
int kj_format_launch(kjl::Lines &st, hipStream_t stream, const kjf::Params &P, const double *d_pw,
                     const kaiju_gpu_compact *d_recs, const uint64_t *d_off, uint32_t n, const void *d_text1, uint64_t bytes1,
                     const kaiju_gpu_name_span *d_names, void *d_out, uint64_t out_cap, kaiju_gpu_format_info *d_info, const char **err);
#endif

#endif  // KJ_FORMAT_H
