// ingest_emu.cpp — the passes of kaiju_amd/csrc/ingest.hip on the host: the per-lane functions of kj_ingest.h, driven tile by
// tile; what a block of the device does with a wavefront scan is a loop over its lanes here.  The tiles of a pass run in the
// order the caller asks for (forward, reversed, shuffled): no pass may depend on it.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_ingest.h"
#include "lines_emu.h"

using namespace kji;
using emu::Order;

namespace {

struct Hdr { uint32_t n_lines = 0, any_empty = 0, first_nonempty = kNone, n_records = 0; };

struct File {
  std::vector<uint8_t> store;
  const uint8_t *text = nullptr;
  uint64_t bytes = 0;
  uint32_t n_tiles = 0;
  std::vector<uint32_t> tile_cnt, tile_base, line_start, blk, blk_base, rec_line;
  std::vector<uint8_t> lflag;
  Hdr hdr;
};

// out[i] = in[0] + .. + in[i - 1], i <= n (k_ing_top_u32)
void top_u32(const std::vector<uint32_t> &in, std::vector<uint32_t> &out, uint32_t n, uint32_t *total) {
  uint32_t carry = 0;
  for (uint32_t i = 0; i < n; i++) { out[i] = carry; carry += in[i]; }
  out[n] = carry;
  if (total) *total = carry;
}

void lines(File &f, Order &o) {
  for (uint64_t t : o.units(f.n_tiles)) {                                     // k_ing_lines_count
    uint32_t tot = 0;
    for (uint32_t l = 0; l < kTileLanes; l++) tot += popc16(nl_mask(f.text, f.bytes, t * kTileLanes + l));
    f.tile_cnt[t] = tot;
  }
  top_u32(f.tile_cnt, f.tile_base, f.n_tiles, nullptr);
  for (uint64_t t : o.units(std::max(1u, f.n_tiles))) {                       // k_ing_lines_fill
    uint32_t ex = 0;
    for (uint32_t l = 0; l < kTileLanes && t < f.n_tiles; l++) {
      const uint64_t c = t * kTileLanes + l;
      const uint32_t m = nl_mask(f.text, f.bytes, c);
      if (m) {
        const uint32_t empty = empty_line_mask(f.text, c, m);
        uint32_t j = f.tile_base[t] + ex;
        for (uint32_t mm = m; mm; mm &= mm - 1, j++) {
          const uint32_t k = ctz16(mm);
          f.line_start[j + 1] = (uint32_t)(c * kChunk + k + 1);
          if (!((empty >> k) & 1u)) f.hdr.first_nonempty = std::min(f.hdr.first_nonempty, j);
        }
        if (empty) f.hdr.any_empty |= 1;
      }
      ex += popc16(m);
    }
    if (t == 0) {
      uint32_t sentinel;
      const uint32_t n_lines = line_count(f.text, f.bytes, f.tile_base[f.n_tiles], &sentinel);
      f.line_start[0] = 0;
      f.line_start[n_lines] = sentinel;
      f.hdr.n_lines = n_lines;
      if (f.bytes && f.text[f.bytes - 1] != '\n') f.hdr.first_nonempty = std::min(f.hdr.first_nonempty, n_lines - 1);
    }
  }
}

void records(File &f, Order &o, int fastq, uint32_t rec_cap) {
  const uint32_t L = f.hdr.n_lines, nb = (L + kScanBlock - 1) / kScanBlock;
  if (fastq && !f.hdr.any_empty) {                                            // k_ing_rec_fast
    const uint32_t n = (L + 3) / 4;
    for (uint32_t r = 0; r < std::min(n, rec_cap); r++) f.rec_line[r] = 4 * r;
    f.hdr.n_records = n;
    return;
  }
  if (fastq) {
    for (uint64_t b : o.units(nb)) {                                          // k_ing_fq_func
      uint32_t tot = kFqIdent;
      for (uint32_t l = 0; l < kScanBlock; l++) {
        const uint32_t i = (uint32_t)b * kScanBlock + l;
        tot = fq_compose(tot, i < L ? fq_func(line_len(f.line_start.data(), i) == 0) : kFqIdent);
      }
      f.blk[b] = tot;
    }
    uint32_t carry = kFqIdent;                                                // k_ing_fq_top
    for (uint32_t b = 0; b < nb; b++) { f.blk_base[b] = fq_apply(carry, 0); carry = fq_compose(carry, f.blk[b]); }
    for (uint64_t b : o.units(nb)) {                                          // k_ing_fq_flag
      uint32_t ex = kFqIdent, cnt = 0;
      for (uint32_t l = 0; l < kScanBlock; l++) {
        const uint32_t i = (uint32_t)b * kScanBlock + l;
        if (i >= L) break;
        const bool empty = line_len(f.line_start.data(), i) == 0;
        const bool h = fq_is_header(fq_apply(ex, f.blk_base[b]), empty);
        f.lflag[i] = h; cnt += h;
        ex = fq_compose(ex, fq_func(empty));
      }
      f.blk[b] = cnt;
    }
  } else {
    for (uint64_t b : o.units(nb)) {                                          // k_ing_fa_flag
      uint32_t cnt = 0;
      for (uint32_t l = 0; l < kScanBlock; l++) {
        const uint32_t i = (uint32_t)b * kScanBlock + l;
        if (i >= L) break;
        const bool h = fa_is_header(f.text, f.line_start.data(), i, f.hdr.first_nonempty);
        f.lflag[i] = h; cnt += h;
      }
      f.blk[b] = cnt;
    }
  }
  top_u32(f.blk, f.blk_base, nb, &f.hdr.n_records);
  for (uint64_t b : o.units(nb)) {                                            // k_ing_rec_scatter
    uint32_t r = f.blk_base[b];
    for (uint32_t l = 0; l < kScanBlock; l++) {
      const uint32_t i = (uint32_t)b * kScanBlock + l;
      if (i >= L) break;
      if (f.lflag[i]) { if (r <= rec_cap) f.rec_line[r] = i; r++; }
    }
  }
}

void prepare(File &f, const uint8_t *text, uint64_t bytes, uint32_t rec_cap) {
  f.store.assign(bytes + 2 * kChunk, 0xaa);                                   // (what lies behind the text is not 0, not '\n', no letter)
  uint8_t *p = f.store.data();
  p += (kChunk - (uintptr_t)p % kChunk) % kChunk;
  if (bytes) memcpy(p, text, bytes);
  f.text = p; f.bytes = bytes;
  f.n_tiles = (uint32_t)((bytes + kTileBytes - 1) / kTileBytes);
  const size_t nblk = (bytes + 1) / kScanBlock + 2;
  f.tile_cnt.assign(f.n_tiles + 1, 0); f.tile_base.assign(f.n_tiles + 1, 0);
  f.line_start.assign(bytes + 2, 0xdeadbeef); f.lflag.assign(bytes + 1, 0);
  f.blk.assign(nblk, 0); f.blk_base.assign(nblk + 1, 0);
  f.rec_line.assign((size_t)rec_cap + 1, 0xdeadbeef);
}

uint32_t count_letters(const uint8_t *text, const Span &s) {
  uint32_t cnt = 0;
  for (uint64_t k = 0; k < span_chunks(s); k++) { Chunk v; cnt += popc16(span_letters(text, s, k, &v)); }
  return cnt;
}
void copy_letters(const uint8_t *text, const Span &s, uint8_t *dst) {
  for (uint64_t k = 0; k < span_chunks(s); k++) { Chunk v; const uint32_t m = span_letters(text, s, k, &v); if (m) put_letters(dst, v, m); dst += popc16(m); }
}
void name_of(const uint8_t *text, const Span &h, int keep_names, uint32_t *pos, uint32_t *len) {
  *pos = (uint32_t)(h.a + 1);
  const uint32_t maxlen = (uint32_t)(h.e - *pos);
  *len = maxlen;
  if (!keep_names) for (uint32_t i = 0; i < maxlen; i++) if (name_stop(text[*pos + i])) { *len = i; break; }
}

}  // namespace

extern "C" void ingest_emu_constants(uint32_t *out) { out[0] = kTileBytes; out[1] = kScanBlock; out[2] = kTeam; out[3] = kChunk; }

// info: the eight 32-bit words of kaiju_gpu_parse_info.  order: 0 forward, 1 reversed, 2 shuffled (seed).
extern "C" int ingest_emu(const uint8_t *t1, uint64_t b1, const uint8_t *t2, uint64_t b2, int paired, int fastq, int keep_names, uint32_t rec_cap,
                          uint8_t *seqs, uint64_t *off, uint32_t *names, uint32_t *info, int order, uint32_t seed) {
  if (b1 > kMaxBytes || b2 > kMaxBytes) return -1;
  Order o{order, std::mt19937(seed)};
  File f1, f2;
  prepare(f1, t1, b1, rec_cap);
  prepare(f2, t2, paired ? b2 : 0, rec_cap);
  lines(f1, o); records(f1, o, fastq, rec_cap);
  if (paired) { lines(f2, o); records(f2, o, fastq, rec_cap); }
  const uint32_t n1 = f1.hdr.n_records, n2 = paired ? f2.hdr.n_records : n1, n = std::min(std::min(n1, n2), rec_cap);
  std::vector<uint32_t> mlen(2 * (size_t)n + 1, 0);
  uint32_t max_mate = 0, mismatch = kNone;
  for (uint64_t r64 : o.units(n)) {                                           // k_ing_span_len
    const uint32_t r = (uint32_t)r64;
    const uint32_t c1 = count_letters(f1.text, seq_span(f1.line_start.data(), f1.rec_line.data(), r, n1, f1.hdr.n_lines, f1.bytes, fastq != 0));
    uint32_t p1, l1, c2 = 0;
    name_of(f1.text, header_span(f1.line_start.data(), f1.rec_line.data(), r), keep_names, &p1, &l1);
    if (paired) {
      c2 = count_letters(f2.text, seq_span(f2.line_start.data(), f2.rec_line.data(), r, n2, f2.hdr.n_lines, f2.bytes, fastq != 0));
      uint32_t p2, l2;
      name_of(f2.text, header_span(f2.line_start.data(), f2.rec_line.data(), r), keep_names, &p2, &l2);
      if (l1 != l2 || memcmp(f1.text + p1, f2.text + p2, l1) != 0) mismatch = std::min(mismatch, r);
    }
    mlen[2 * (size_t)r] = c1; mlen[2 * (size_t)r + 1] = c2;
    names[2 * (size_t)r] = p1; names[2 * (size_t)r + 1] = l1;
    max_mate = std::max(max_mate, std::max(c1, c2));
  }
  emu::scan_offsets(o, mlen.data(), 2 * (uint64_t)n, kScanBlock, off);        // kjl::k_scan_sums / _top / _apply
  for (uint64_t r64 : o.units(n)) {                                           // k_ing_span_copy
    const uint32_t r = (uint32_t)r64;
    copy_letters(f1.text, seq_span(f1.line_start.data(), f1.rec_line.data(), r, n1, f1.hdr.n_lines, f1.bytes, fastq != 0), seqs + off[2 * (size_t)r]);
    if (paired)
      copy_letters(f2.text, seq_span(f2.line_start.data(), f2.rec_line.data(), r, n2, f2.hdr.n_lines, f2.bytes, fastq != 0), seqs + off[2 * (size_t)r + 1]);
  }
  const uint64_t seq_bytes = off[2 * (size_t)n];                              // k_ing_finish
  info[0] = n1; info[1] = paired ? n2 : 0; info[2] = max_mate; info[3] = mismatch;
  info[4] = (uint32_t)seq_bytes; info[5] = (uint32_t)(seq_bytes >> 32);
  info[6] = std::min(n1, n2) > rec_cap ? 1u : 0u; info[7] = 0;
  return 0;
}
