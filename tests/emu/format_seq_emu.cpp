// format_seq_emu.cpp — the passes of kaiju_amd/csrc/format_seq.hip on the host: the per-lane and per-team functions of
// kj_format_seq.h, driven work unit by work unit.  What a team of the device does with shuffles is a round over the rows of its
// 32 lanes here (a lane sees the values its team mates had at the end of the round before); what a block does with a wavefront
// scan is a loop.  The units of a pass - records, the lanes of a team, the lanes of every step of the fragment scan, blocks,
// chunks - run in the order the caller asks for (forward, reversed, shuffled): no pass may depend on it.  The strides of the
// fragment scan of ONE read follow each other, on the device as here: the run of the last lane is the carry into the next.
//
// With -DFORMAT_SEQ_EMU_MAIN the file is a program of its own: it reads the cases tests/format_seq_inputs.py dumps (name table,
// inputs, capacity, the expected bytes and info) and runs every one of them in the three orders - what the sanitizer build runs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_format_seq.h"
#include "lines_emu.h"

using namespace kjq;
using emu::Order;

namespace {

// lane k of the team as the rows hold it (the lane's own copy is not looked at)
struct TeamRows {
  const Lane *lane;
  uint64_t id(uint64_t, uint32_t k) const { return lane[k].id; }
  uint32_t piece(uint32_t, uint32_t k) const { return lane[k].piece; }
};
struct TeamState { Lane lane[kTeam]; uint32_t id_off[kTeam], ids_len[kTeam]; };

// the round of a team on record r; false: the lanes disagree on the length of the column
bool team_round(const Job &J, uint32_t r, const Head &h, Order &o, TeamState &T) {
  for (uint64_t i : o.units(kTeam)) T.lane[i] = load_lane(J, r, (uint32_t)i, h);
  const TeamRows x{T.lane};
  for (uint64_t i : o.units(kTeam)) round_ids(x, T.lane[i], (uint32_t)i, &T.id_off[i], &T.ids_len[i]);
  for (uint32_t i = 1; i < kTeam; i++) if (T.ids_len[i] != T.ids_len[0]) return false;
  return true;
}

// team_has_fragment of format_seq.hip
bool team_has_fragment(const Job &J, uint32_t r, uint64_t l1, Order &o) {
  Seg carry{0, 0, 0};
  bool hit = false;
  uint32_t d[kTeam];
  Seg cur[kTeam], nxt[kTeam];
  for (uint64_t s = 0; s < frag_steps(l1); s++) {
    for (uint64_t i : o.units(kTeam)) { d[i] = frag_letter(J, r, s * kTeam + i, l1); cur[i] = frag_init(d[i]); }
    for (uint32_t delta = 1; delta < kTeam; delta <<= 1) {
      for (uint64_t i : o.units(kTeam)) nxt[i] = frag_round(cur[i], cur[i >= delta ? i - delta : i], (uint32_t)i, delta);
      memcpy(cur, nxt, sizeof cur);
    }
    for (uint64_t i : o.units(kTeam)) { nxt[i] = frag_close(cur[i], carry); hit = hit || frag_hit(J, d[i], nxt[i]); }
    carry = nxt[kTeam - 1];
  }
  return hit;
}

}  // namespace

extern "C" void format_seq_emu_constants(uint32_t *out) { out[0] = kBlockBytes; out[1] = kScanBlock; out[2] = kChunk; out[3] = kjf::kPowK; out[4] = kTeam; out[5] = kMaxSeqName; }

// a[]: 0 pw, 1 hits, 2 off, 3 n, 4 paired, 5 seqs, 6 text_pos, 7 text_len, 8 trunc, 9 pep (0: no peptide column), 10 text_cap, 11 names_text,
// 12 names_bytes, 13 names, 14 sn_blob, 15 sn_off, 16 sn_len, 17 nseq, 18 out, 19 out_cap, 20 info (32 bytes), 21 gate, 22 protein, 23 u_rule,
// 24 min_frag, 25 min_score, 26 greedy - pointers and numbers as uint64; d[]: db_length, min_evalue.  out: out_cap bytes, changed only
// where lines are written.  order: 0 forward, 1 reversed, 2 shuffled (seed).
extern "C" int format_seq_emu(const uint64_t *a, const double *d, int order, uint32_t seed) {
  Job J{};
  const uint32_t n = (uint32_t)a[3];
  J.pw = reinterpret_cast<const double *>(a[0]);
  J.hits = reinterpret_cast<const kaiju_gpu_hit *>(a[1]); J.off = reinterpret_cast<const uint64_t *>(a[2]);
  J.seqs = reinterpret_cast<const uint8_t *>(a[5]); J.text_pos = reinterpret_cast<const uint64_t *>(a[6]);
  J.text_len = reinterpret_cast<const uint32_t *>(a[7]); J.trunc = reinterpret_cast<const uint32_t *>(a[8]);
  J.pep = reinterpret_cast<const uint8_t *>(a[9]); J.text_cap = (uint32_t)a[10];
  J.names_text = reinterpret_cast<const uint8_t *>(a[11]); J.names_bytes = a[12]; J.names = reinterpret_cast<const kaiju_gpu_name_span *>(a[13]);
  J.sn_blob = reinterpret_cast<const uint8_t *>(a[14]); J.sn_off = reinterpret_cast<const uint64_t *>(a[15]);
  J.sn_len = reinterpret_cast<const uint32_t *>(a[16]); J.nseq = (uint32_t)a[17];
  uint8_t *out = reinterpret_cast<uint8_t *>(a[18]);
  J.out_cap = a[19];
  J.P.db_length = d[0]; J.P.min_evalue = d[1]; J.P.gate = (int32_t)a[21]; J.P.protein = (int32_t)a[22]; J.P.paired = (int32_t)a[4];
  J.u_rule = (uint32_t)a[23]; J.min_frag = (uint32_t)a[24]; J.min_score = (uint32_t)a[25]; J.greedy = (uint32_t)a[26];
  if (J.names_bytes > kjf::kMaxBytes || n > kjf::kMaxRecords) return -1;
  Order o{order, std::mt19937(seed)};
  std::vector<uint64_t> llen((size_t)n + 1, 0xdeadbeefdeadbeefull), line_off((size_t)n + 1, 0xdeadbeefdeadbeefull), code((size_t)n + 1, 0xdeadbeefdeadbeefull);
  J.llen = llen.data(); J.line_off = line_off.data(); J.code = code.data();
  Hdr hdr{0, n, 0, 0, 0};
  TeamState T;
  for (uint64_t r64 : o.units(n)) {                                           // k_fs_len
    const uint32_t r = (uint32_t)r64;
    const Head h = record_head(J, r);
    if (h.classified) {
      if (!team_round(J, r, h, o, T)) return -20;
      llen[r] = line_len_c(h, T.ids_len[0]);
      code[r] = kCodeC;
    } else {
      bool scan;
      bool gated = u_gated(J, h, &scan);
      if (scan) gated = !team_has_fragment(J, r, h.l1, o);
      llen[r] = line_len_u(h, gated);
      code[r] = gated ? kCodeGated : kCodeU;
    }
    hdr.n_classified += h.classified;
    hdr.n_inexact += h.inexact;
    hdr.n_truncated += h.truncated;
  }
  emu::scan_offsets(o, llen.data(), n, kScanBlock, line_off.data());          // kjl::k_scan_sums / _top / _apply
  const uint64_t total = line_off[n];
  // the output and its shadow as the device sees them: 16-byte aligned, and not one byte longer than out_cap
  void *mem = nullptr;
  if (posix_memalign(&mem, kChunk, std::max<uint64_t>(J.out_cap, 1)) != 0) return -6;
  J.out = static_cast<uint8_t *>(mem);
  if (J.out_cap) memcpy(J.out, out, J.out_cap);
  uint8_t *shadow = static_cast<uint8_t *>(malloc(std::max<uint64_t>(J.out_cap, 1)));
  if (!shadow) { free(mem); return -6; }
  memset(shadow, 0xEE, std::max<uint64_t>(J.out_cap, 1));
  J.shadow = shadow;
  for (uint64_t r64 : o.units(n)) {                                           // k_fs_mid
    const uint32_t r = (uint32_t)r64;
    if (code[r] != kCodeC || line_off[r + 1] > J.out_cap) continue;
    const Head h = record_head(J, r);
    if (!team_round(J, r, h, o, T)) { free(mem); free(shadow); return -20; }
    for (uint64_t i : o.units(kTeam)) mid_lane(J, h, T.lane[i], (uint32_t)i, T.id_off[i], T.ids_len[i], shadow + line_off[r] + 3 + h.name.len);
  }
  emu::write_blocks(o, line_off.data(), n, J.out, J.out_cap,                  // k_fs_write
                    [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) { return format_schunk(J, c, lo, hi, total, v); });
  if (J.out_cap) memcpy(out, J.out, J.out_cap);
  hdr.written = kjv::written_bytes(line_off.data(), n, J.out_cap);            // k_fs_finish
  const kaiju_gpu_format_verbose_info fi = kjv::make_info(total, hdr, J.out_cap);
  memcpy(reinterpret_cast<void *>(a[20]), &fi, sizeof fi);
  free(mem); free(shadow);
  return 0;
}

#ifdef FORMAT_SEQ_EMU_MAIN
// case file: the table of the E-value gate (kPowK doubles); nseq, bytes of the blob, sn_off[nseq + 1], sn_len[nseq], the blob; then
// per case sixteen uint64 (n, paired, names_bytes, gate, protein, out_cap, bytes of expected text, text_cap, bytes of peptides, 1 if
// there is a peptide column, u_rule, min_frag, min_score, greedy, bytes of reads, 0), two doubles (db_length, min_evalue), the 32
// bytes of the expected info, then hits, off, the kaiju_gpu_verbose records, text_pos, names, the names' text, the peptides, the
// reads and the expected text; the output starts as 0xA5.  Every array is read into a buffer of exactly its size.
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  unsigned n_cases = 0, bad = 0;
  std::vector<double> pw(kjf::kPowK);
  uint64_t th[2];
  if (fread(pw.data(), sizeof(double), kjf::kPowK, f) != kjf::kPowK || fread(th, sizeof th, 1, f) != 1) return 2;
  const size_t nseq = (size_t)th[0];
  std::vector<uint64_t> soff(nseq + 1);
  std::vector<uint32_t> slen(nseq);
  std::vector<uint8_t> blob(th[1]);
  if (fread(soff.data(), 8, nseq + 1, f) != nseq + 1 || fread(slen.data(), 4, nseq, f) != nseq || (th[1] && fread(blob.data(), 1, th[1], f) != th[1])) return 2;
  uint64_t h[16];
  while (fread(h, sizeof h, 1, f) == 1) {
    double d[2];
    kaiju_gpu_format_verbose_info want;
    if (fread(d, sizeof d, 1, f) != 1 || fread(&want, sizeof want, 1, f) != 1) return 2;
    const uint32_t n = (uint32_t)h[0];
    std::vector<kaiju_gpu_hit> hits(n);
    std::vector<uint64_t> off(2 * (size_t)n + 1), tpos(n);
    std::vector<kaiju_gpu_verbose> v(n);
    std::vector<kaiju_gpu_name_span> names(n);
    std::vector<uint8_t> text(h[2]), pep(h[8]), seqs(h[14]), expect(h[6]);
    if ((n && fread(hits.data(), sizeof(kaiju_gpu_hit), n, f) != n) || fread(off.data(), 8, off.size(), f) != off.size() ||
        (n && (fread(v.data(), sizeof(kaiju_gpu_verbose), n, f) != n || fread(tpos.data(), 8, n, f) != n || fread(names.data(), 8, n, f) != n)) ||
        (h[2] && fread(text.data(), 1, h[2], f) != h[2]) || (h[8] && fread(pep.data(), 1, h[8], f) != h[8]) ||
        (h[14] && fread(seqs.data(), 1, h[14], f) != h[14]) || (h[6] && fread(expect.data(), 1, h[6], f) != h[6])) return 2;
    std::vector<uint32_t> tlen(n), trunc(n);
    for (uint32_t r = 0; r < n; r++) { tlen[r] = v[r].text_len; trunc[r] = v[r].truncated; }
    uint8_t none = 0;
    for (int order = 0; order < 3; order++) {
      std::vector<uint8_t> out(h[5], 0xA5);
      kaiju_gpu_format_verbose_info got;
      const uint64_t a[27] = {(uint64_t)pw.data(), (uint64_t)hits.data(), (uint64_t)off.data(), n, h[1], (uint64_t)seqs.data(), (uint64_t)tpos.data(),
                              (uint64_t)tlen.data(), (uint64_t)trunc.data(), h[9] ? (uint64_t)(pep.empty() ? &none : pep.data()) : 0, h[7],
                              (uint64_t)text.data(), h[2], (uint64_t)names.data(), (uint64_t)blob.data(), (uint64_t)soff.data(), (uint64_t)slen.data(), nseq,
                              (uint64_t)out.data(), h[5], (uint64_t)&got, h[3], h[4], h[10], h[11], h[12], h[13]};
      const int rc = format_seq_emu(a, d, order, 11 + order);
      bool ok = rc == 0 && memcmp(&got, &want, sizeof got) == 0 && h[6] <= h[5] && (h[6] == 0 || memcmp(out.data(), expect.data(), h[6]) == 0);
      for (uint64_t i = h[6]; ok && i < h[5]; i++) ok = out[i] == 0xA5;
      if (!ok) { bad++; fprintf(stderr, "case %u order %d: differs (rc %d)\n", n_cases, order, rc); }
    }
    n_cases++;
  }
  fclose(f);
  printf("format_seq_emu: %u cases in three orders, %u differ\n", n_cases, bad);
  return bad || !n_cases ? 1 : 0;
}
#endif
