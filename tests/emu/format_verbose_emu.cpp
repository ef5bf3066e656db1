// format_verbose_emu.cpp — the passes of kaiju_amd/csrc/format_verbose.hip on the host: the per-lane and per-team functions of
// kj_format_verbose.h, driven work unit by work unit.  What a team of the device does with shuffles is three rounds over the
// rows of its 32 lanes here (a lane sees the values its team mates had at the end of the round before); what a block does
// with a wavefront scan is a loop.  The units of a pass - records, the lanes of a team, blocks, chunks - run in the order the
// caller asks for (forward, reversed, shuffled): no pass may depend on it.
//
// With -DFORMAT_VERBOSE_EMU_MAIN the file is a program of its own: it reads the cases tests/format_verbose_inputs.py dumps
// (accession table, inputs, capacity, the expected bytes and info) and runs every one of them in the three orders - what the
// sanitizer build runs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_format_verbose.h"
#include "lines_emu.h"

using namespace kjv;
using emu::Order;

namespace {

// lane k of the team as the rows hold it (the lane's own copy is not looked at)
struct TeamRows {
  const Lane *lane; const uint32_t *kl;
  uint64_t id(uint64_t, uint32_t k) const { return lane[k].id; }
  uint32_t id_len(uint32_t, uint32_t k) const { return lane[k].id_len; }
  uint32_t rank(uint32_t, uint32_t k) const { return lane[k].rank; }
  uint32_t klen(uint32_t, uint32_t k) const { return kl[k]; }
};
struct TeamState { Lane lane[kTeam]; uint32_t id_off[kTeam], ids_len[kTeam], klen[kTeam], acc_off[kTeam], accs_len[kTeam]; };

// the three rounds of a team on record r; false: the lanes disagree on the length of a column
bool team_rounds(const Job &J, uint32_t r, const Head &h, Order &o, TeamState &T) {
  for (uint64_t i : o.units(kTeam)) T.lane[i] = load_lane(J, r, (uint32_t)i, h);
  const TeamRows x{T.lane, T.klen};
  for (uint64_t i : o.units(kTeam)) round_ids(x, T.lane[i], (uint32_t)i, &T.id_off[i], &T.ids_len[i], &T.klen[i]);      // (reads no klen)
  for (uint64_t i : o.units(kTeam)) round_accs(x, T.lane[i], T.klen[i], &T.acc_off[i], &T.accs_len[i]);
  for (uint32_t i = 1; i < kTeam; i++) if (T.ids_len[i] != T.ids_len[0] || T.accs_len[i] != T.accs_len[0]) return false;
  return true;
}

}  // namespace

extern "C" void format_verbose_emu_constants(uint32_t *out) { out[0] = kBlockBytes; out[1] = kScanBlock; out[2] = kChunk; out[3] = kjf::kPowK; out[4] = kTeam; }

// a[]: 0 pw, 1 hits, 2 recs, 3 off, 4 n, 5 paired, 6 n_acc, 7 acc_iseq, 8 text_pos, 9 text_len, 10 trunc, 11 pep, 12 text_cap, 13 names_text,
// 14 names_bytes, 15 names, 16 acc_blob, 17 acc_off, 18 acc_len, 19 acc_rank, 20 nseq, 21 out, 22 out_cap, 23 info (32 bytes), 24 gate,
// 25 protein - pointers and numbers as uint64; d[]: db_length, min_evalue.  out: out_cap bytes, changed only where lines are
// written.  order: 0 forward, 1 reversed, 2 shuffled (seed).
extern "C" int format_verbose_emu(const uint64_t *a, const double *d, int order, uint32_t seed) {
  Job J{};
  const uint32_t n = (uint32_t)a[4];
  J.pw = reinterpret_cast<const double *>(a[0]);
  J.hits = reinterpret_cast<const kaiju_gpu_hit *>(a[1]); J.recs = reinterpret_cast<const kaiju_gpu_compact *>(a[2]);
  J.off = reinterpret_cast<const uint64_t *>(a[3]); J.n_acc = reinterpret_cast<const uint32_t *>(a[6]);
  J.acc_iseq = reinterpret_cast<const uint32_t *>(a[7]); J.text_pos = reinterpret_cast<const uint64_t *>(a[8]);
  J.text_len = reinterpret_cast<const uint32_t *>(a[9]); J.trunc = reinterpret_cast<const uint32_t *>(a[10]);
  J.pep = reinterpret_cast<const uint8_t *>(a[11]); J.text_cap = (uint32_t)a[12];
  J.names_text = reinterpret_cast<const uint8_t *>(a[13]); J.names_bytes = a[14]; J.names = reinterpret_cast<const kaiju_gpu_name_span *>(a[15]);
  J.acc_blob = reinterpret_cast<const uint8_t *>(a[16]); J.acc_off = reinterpret_cast<const uint64_t *>(a[17]);
  J.acc_len = reinterpret_cast<const uint32_t *>(a[18]); J.acc_rank = reinterpret_cast<const uint32_t *>(a[19]); J.nseq = (uint32_t)a[20];
  uint8_t *out = reinterpret_cast<uint8_t *>(a[21]);
  J.out_cap = a[22];
  J.P.db_length = d[0]; J.P.min_evalue = d[1]; J.P.gate = (int32_t)a[24]; J.P.protein = (int32_t)a[25]; J.P.paired = (int32_t)a[5];
  if (J.names_bytes > kjf::kMaxBytes || n > kjf::kMaxRecords) return -1;
  Order o{order, std::mt19937(seed)};
  std::vector<uint64_t> llen((size_t)n + 1, 0xdeadbeefdeadbeefull), line_off((size_t)n + 1, 0xdeadbeefdeadbeefull), tax((size_t)n + 1, 0xdeadbeefdeadbeefull);
  J.llen = llen.data(); J.line_off = line_off.data(); J.tax = tax.data();
  Hdr hdr{0, n, 0, 0, 0};
  TeamState T;
  for (uint64_t r64 : o.units(n)) {                                           // k_fv_len
    const uint32_t r = (uint32_t)r64;
    const Head h = record_head(J, r);
    if (!h.taxon) llen[r] = line_len_u(h);
    else {
      if (!team_rounds(J, r, h, o, T)) return -20;
      llen[r] = line_len_c(h, T.ids_len[0], T.accs_len[0]);
    }
    tax[r] = h.taxon;
    hdr.n_classified += h.taxon ? 1 : 0;
    hdr.n_inexact += (J.recs[r].info & KAIJU_HIT_INEXACT) ? 1 : 0;
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
  for (uint64_t r64 : o.units(n)) {                                           // k_fv_mid
    const uint32_t r = (uint32_t)r64;
    if (!tax[r] || line_off[r + 1] > J.out_cap) continue;
    const Head h = record_head(J, r);
    if (!team_rounds(J, r, h, o, T)) { free(mem); free(shadow); return -20; }
    for (uint64_t i : o.units(kTeam))
      mid_lane(J, h, T.lane[i], (uint32_t)i, T.id_off[i], T.ids_len[i], T.klen[i], T.acc_off[i], T.accs_len[i], shadow + line_off[r] + 3 + h.name.len);
  }
  emu::write_blocks(o, line_off.data(), n, J.out, J.out_cap,                  // k_fv_write
                    [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) { return format_vchunk(J, c, lo, hi, total, v); });
  if (J.out_cap) memcpy(out, J.out, J.out_cap);
  hdr.written = written_bytes(line_off.data(), n, J.out_cap);                 // k_fv_finish
  const kaiju_gpu_format_verbose_info fi = make_info(total, hdr, J.out_cap);
  memcpy(reinterpret_cast<void *>(a[23]), &fi, sizeof fi);
  free(mem); free(shadow);
  return 0;
}

#ifdef FORMAT_VERBOSE_EMU_MAIN
// case file: the table of the E-value gate (kPowK doubles); nseq, bytes of the blob, acc_off[nseq + 1], acc_len[nseq], acc_rank[nseq],
// the blob; then per case ten uint64 (n, paired, names_bytes, gate, protein, out_cap, bytes of expected text, text_cap, bytes of
// peptides, 0), two doubles (db_length, min_evalue), the 32 bytes of the expected info, then hits, recs, off, the kaiju_gpu_verbose
// records, text_pos, names, the names' text, the peptides and the expected text; the output starts as 0xA5
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  unsigned n_cases = 0, bad = 0;
  std::vector<double> pw(kjf::kPowK);
  uint64_t th[2];
  if (fread(pw.data(), sizeof(double), kjf::kPowK, f) != kjf::kPowK || fread(th, sizeof th, 1, f) != 1) return 2;
  const size_t nseq = (size_t)th[0];
  std::vector<uint64_t> aoff(nseq + 1);
  std::vector<uint32_t> alen(nseq), arank(nseq);
  std::vector<uint8_t> blob(th[1]);
  if (fread(aoff.data(), 8, nseq + 1, f) != nseq + 1 || fread(alen.data(), 4, nseq, f) != nseq || fread(arank.data(), 4, nseq, f) != nseq ||
      (th[1] && fread(blob.data(), 1, th[1], f) != th[1])) return 2;
  uint64_t h[10];
  while (fread(h, sizeof h, 1, f) == 1) {
    double d[2];
    kaiju_gpu_format_verbose_info want;
    if (fread(d, sizeof d, 1, f) != 1 || fread(&want, sizeof want, 1, f) != 1) return 2;
    const uint32_t n = (uint32_t)h[0];
    std::vector<kaiju_gpu_hit> hits(n);
    std::vector<kaiju_gpu_compact> recs(n);
    std::vector<uint64_t> off(2 * (size_t)n + 1), tpos(n);
    std::vector<kaiju_gpu_verbose> v(n);
    std::vector<kaiju_gpu_name_span> names(n);
    std::vector<uint8_t> text(h[2]), pep(h[8]), expect(h[6]);
    if ((n && (fread(hits.data(), sizeof(kaiju_gpu_hit), n, f) != n || fread(recs.data(), 16, n, f) != n)) || fread(off.data(), 8, off.size(), f) != off.size() ||
        (n && (fread(v.data(), sizeof(kaiju_gpu_verbose), n, f) != n || fread(tpos.data(), 8, n, f) != n || fread(names.data(), 8, n, f) != n)) ||
        (h[2] && fread(text.data(), 1, h[2], f) != h[2]) || (h[8] && fread(pep.data(), 1, h[8], f) != h[8]) || (h[6] && fread(expect.data(), 1, h[6], f) != h[6])) return 2;
    std::vector<uint32_t> nacc(n), tlen(n), trunc(n), acc((size_t)n * kMaxAcc);
    for (uint32_t r = 0; r < n; r++) {
      nacc[r] = v[r].n_acc; tlen[r] = v[r].text_len; trunc[r] = v[r].truncated;
      memcpy(&acc[(size_t)r * kMaxAcc], v[r].acc_iseq, sizeof v[r].acc_iseq);
    }
    for (int order = 0; order < 3; order++) {
      std::vector<uint8_t> out(h[5], 0xA5);
      kaiju_gpu_format_verbose_info got;
      const uint64_t a[26] = {(uint64_t)pw.data(), (uint64_t)hits.data(), (uint64_t)recs.data(), (uint64_t)off.data(), n, h[1], (uint64_t)nacc.data(),
                              (uint64_t)acc.data(), (uint64_t)tpos.data(), (uint64_t)tlen.data(), (uint64_t)trunc.data(), (uint64_t)pep.data(), h[7],
                              (uint64_t)text.data(), h[2], (uint64_t)names.data(), (uint64_t)blob.data(), (uint64_t)aoff.data(), (uint64_t)alen.data(),
                              (uint64_t)arank.data(), nseq, (uint64_t)out.data(), h[5], (uint64_t)&got, h[3], h[4]};
      const int rc = format_verbose_emu(a, d, order, 11 + order);
      bool ok = rc == 0 && memcmp(&got, &want, sizeof got) == 0 && h[6] <= h[5] && (h[6] == 0 || memcmp(out.data(), expect.data(), h[6]) == 0);
      for (uint64_t i = h[6]; ok && i < h[5]; i++) ok = out[i] == 0xA5;
      if (!ok) { bad++; fprintf(stderr, "case %u order %d: differs (rc %d)\n", n_cases, order, rc); }
    }
    n_cases++;
  }
  fclose(f);
  printf("format_verbose_emu: %u cases in three orders, %u differ\n", n_cases, bad);
  return bad || !n_cases ? 1 : 0;
}
#endif
