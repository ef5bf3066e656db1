// format_emu.cpp — the passes of kaiju_amd/csrc/format.hip on the host: the per-lane functions of kj_format.h, driven work unit
// by work unit; what a block of the device does with a wavefront scan is a loop over its lanes here.  The units of a pass run
// in the order the caller asks for (forward, reversed, shuffled): no pass may depend on it.
//
// With -DFORMAT_EMU_MAIN the file is a program of its own: it reads the cases tests/format_inputs.py dumps (inputs, capacity,
// the expected bytes and info) and runs every one of them in the three orders - what the sanitizer build runs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_format.h"
#include "lines_emu.h"

using namespace kjf;
using emu::Order;

extern "C" void format_emu_constants(uint32_t *out) { out[0] = kBlockBytes; out[1] = kScanBlock; out[2] = kChunk; out[3] = kPowK; }
// pw[0 .. k); returns 1 when the table stands for every score (kjf::build_pow_table)
extern "C" int format_emu_table(double *pw, uint32_t k) { return build_pow_table(pw, k) ? 1 : 0; }
extern "C" double format_emu_pow_factor(uint32_t best) { return pow_factor(best); }

// info: the six 32-bit words of kaiju_gpu_format_info.  out: out_cap bytes, changed only where lines are written.  pw_in: the
// table of the E-value gate, kPowK entries (the library's: kaiju_gpu_format_evalue_table), NULL: the one this build makes.
// order: 0 forward, 1 reversed, 2 shuffled (seed).
extern "C" int format_emu(const double *pw_in, const kaiju_gpu_compact *recs, const uint64_t *off, uint32_t n, int paired, const uint8_t *text1, uint64_t bytes1,
                          const kaiju_gpu_name_span *names, double db_length, double min_evalue, int gate, int protein, uint8_t *out,
                          uint64_t out_cap, uint32_t *info, int order, uint32_t seed) {
  if (bytes1 > kMaxBytes || n > kMaxRecords) return -1;
  Order o{order, std::mt19937(seed)};
  std::vector<double> pw(kPowK);
  if (pw_in) pw.assign(pw_in, pw_in + kPowK);
  else if (!build_pow_table(pw.data(), kPowK)) return -7;
  Params P{};
  P.db_length = db_length; P.min_evalue = min_evalue; P.gate = gate; P.protein = protein; P.paired = paired;
  std::vector<uint32_t> llen((size_t)n + 1, 0xdeadbeefu);
  std::vector<uint64_t> line_off((size_t)n + 1, 0xdeadbeefdeadbeefull), tax((size_t)n + 1, 0xdeadbeefdeadbeefull);
  uint32_t n_classified = 0, n_inexact = 0;
  for (uint64_t r64 : o.units(n)) {                                           // k_fmt_len
    const uint32_t r = (uint32_t)r64;
    uint64_t t;
    llen[r] = record_line(recs, off, names, r, bytes1, P, pw.data(), &t);
    tax[r] = t;
    n_classified += t ? 1 : 0;
    n_inexact += (recs[r].info & KAIJU_HIT_INEXACT) ? 1 : 0;
  }
  emu::scan_offsets(o, llen.data(), n, kScanBlock, line_off.data());          // kjl::k_scan_sums / _top / _apply
  const uint64_t total = line_off[n];
  // the output as the device sees it: 16-byte aligned, and not one byte longer than out_cap
  void *mem = nullptr;
  if (posix_memalign(&mem, kChunk, std::max<uint64_t>(out_cap, 1)) != 0) return -6;
  uint8_t *dev_out = static_cast<uint8_t *>(mem);
  if (out_cap) memcpy(dev_out, out, out_cap);
  emu::write_blocks(o, line_off.data(), n, dev_out, out_cap,                  // k_fmt_write
                    [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) { return format_chunk(c, text1, bytes1, names, line_off.data(), tax.data(), lo, hi, total, out_cap, v); });
  if (out_cap) memcpy(out, dev_out, out_cap);
  free(mem);
  const kaiju_gpu_format_info fi = make_info(total, n, n_classified, n_inexact, out_cap);      // k_fmt_finish
  memcpy(info, &fi, sizeof fi);
  return 0;
}

#ifdef FORMAT_EMU_MAIN
// case file: the table of the E-value gate (kPowK doubles), then per case seven uint64 (n, paired, bytes1, gate, protein, out_cap, bytes of expected text), two doubles (db_length,
// min_evalue), the 24 bytes of the expected info, then recs, off, names, text1 and the expected text; the output starts as 0xA5
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint64_t h[7];
  unsigned n_cases = 0, bad = 0;
  std::vector<double> pw(kPowK);
  if (fread(pw.data(), sizeof(double), kPowK, f) != kPowK) return 2;
  while (fread(h, sizeof h, 1, f) == 1) {
    double d[2];
    kaiju_gpu_format_info want;
    if (fread(d, sizeof d, 1, f) != 1 || fread(&want, sizeof want, 1, f) != 1) return 2;
    const uint32_t n = (uint32_t)h[0];
    std::vector<kaiju_gpu_compact> recs(n);
    std::vector<uint64_t> off(2 * (size_t)n + 1);
    std::vector<kaiju_gpu_name_span> names(n);
    std::vector<uint8_t> text(h[2]), expect(h[6]);
    if ((n && (fread(recs.data(), 16, n, f) != n || fread(names.data(), 8, n, f) != n)) || fread(off.data(), 8, off.size(), f) != off.size() ||
        (h[2] && fread(text.data(), 1, h[2], f) != h[2]) || (h[6] && fread(expect.data(), 1, h[6], f) != h[6])) return 2;
    for (int order = 0; order < 3; order++) {
      std::vector<uint8_t> out(h[5], 0xA5);
      kaiju_gpu_format_info got;
      const int rc = format_emu(pw.data(), recs.data(), off.data(), n, (int)h[1], text.data(), h[2], names.data(), d[0], d[1], (int)h[3], (int)h[4], out.data(),
                                h[5], reinterpret_cast<uint32_t *>(&got), order, 11 + order);
      bool ok = rc == 0 && memcmp(&got, &want, sizeof got) == 0 && h[6] <= h[5] && (h[6] == 0 || memcmp(out.data(), expect.data(), h[6]) == 0);
      for (uint64_t i = h[6]; ok && i < h[5]; i++) ok = out[i] == 0xA5;
      if (!ok) { bad++; fprintf(stderr, "case %u order %d: differs (rc %d)\n", n_cases, order, rc); }
    }
    n_cases++;
  }
  fclose(f);
  printf("format_emu: %u cases in three orders, %u differ\n", n_cases, bad);
  return bad || !n_cases ? 1 : 0;
}
#endif
