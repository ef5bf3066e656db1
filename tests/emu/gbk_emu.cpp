// gbk_emu.cpp — kaiju_amd/csrc/kj_gbk.h on the host: the per-lane functions of gbk.hip driven pass by pass, the units of every
// pass in the order the caller asks for (lines_emu.h).  What a kernel does with an atomic is a plain read-modify-write here; the
// order of the lanes stands in for the races.  The maximum-scans run in the three steps of the device: the maxima of blocks of
// 256 lines, the block on top, the lines of a block.  tests/test_gbk_emu.py compares with tests/gbk_expect.py.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kaiju_amd/csrc/kj_gbk.h"
#include "lines_emu.h"

using namespace kjg;

namespace {

// a text as the device sees it: 16-byte aligned, 16 readable bytes behind it
struct Text {
  std::vector<uint8_t> store;
  uint8_t *p = nullptr;
  uint64_t bytes = 0;
  std::vector<uint32_t> line_start;
  uint32_t n_lines = 0;
  Text(const uint8_t *src, uint64_t n) : store(n + 48, 0x22), bytes(n) {      // ('"' behind the text: nothing may look at it)
    p = store.data() + ((16 - ((uintptr_t)store.data() & 15)) & 15);
    if (n) memcpy(p, src, n);
    line_start.assign(n + 2, 0);
    uint32_t nl = 0;
    for (uint64_t c = 0; c * kChunk < n; c++)
      for (uint32_t m = kji::nl_mask(p, n, c); m; m &= m - 1) line_start[++nl] = (uint32_t)(c * kChunk + kji::ctz16(m) + 1);
    uint32_t sentinel;
    n_lines = kji::line_count(p, n, nl, &sentinel);
    line_start[n_lines] = sentinel;
  }
};

struct EmuGbk {
  Carry carry{};
  std::vector<uint8_t> tax, pid;       // the carried strings
};

}  // namespace

extern "C" {

void *gbemu_create() { return new EmuGbk(); }
void gbemu_free(void *h) { delete static_cast<EmuGbk *>(h); }
void gbemu_reset(void *h) { static_cast<EmuGbk *>(h)->carry = Carry{}; }
// the carried state: lengths and flag into st[3], the strings into tax / pid (cap bytes each)
void gbemu_state(const void *h, uint32_t *st, uint8_t *tax, uint8_t *pid, uint64_t cap) {
  const EmuGbk *G = static_cast<const EmuGbk *>(h);
  st[0] = G->carry.tax_len; st[1] = G->carry.pid_len; st[2] = G->carry.in_t;
  memcpy(tax, G->tax.data(), std::min<uint64_t>(cap, G->carry.tax_len));
  memcpy(pid, G->pid.data(), std::min<uint64_t>(cap, G->carry.pid_len));
}

// the kind byte and the capture of one line (text[0, n) is the line)
uint32_t gbemu_classify(const uint8_t *line, uint64_t n, uint32_t *cap) {
  const Text X(line, n);
  const LineKind L = classify(X.p, 0, n);
  cap[0] = L.cap_a; cap[1] = L.cap_e;
  return L.kind;
}

// the passes of gbk.hip; out: out_cap bytes, 16-byte aligned
int gbemu_convert(void *h, const uint8_t *text, uint64_t n, uint8_t *out, uint64_t out_cap, kaiju_gpu_gbk_info *info, int order, uint32_t seed) {
  EmuGbk *G = static_cast<EmuGbk *>(h);
  emu::Order o{order, std::mt19937(seed)};
  const Text X(text, n);
  const uint32_t nl = X.n_lines;
  if (G->tax.size() < n + 1) { G->tax.resize(n + 1); G->pid.resize(n + 1); }              // grow_carry
  Totals T{};                                                                              // k_gb_init
  T.no_tax_line = kNone;
  std::vector<uint8_t> kind(nl + 1, 0), in_t(nl + 1, 0);
  std::vector<uint32_t> cap_a(nl + 1, 0), cap_e(nl + 1, 0), tax_src(nl + 1, 0), pid_src(nl + 1, 0);
  for (uint64_t i : o.units(nl)) {                                                         // k_gb_kinds
    const LineKind L = classify(X.p, X.line_start[i], (uint64_t)X.line_start[i + 1] - 1);
    kind[i] = (uint8_t)L.kind; cap_a[i] = L.cap_a; cap_e[i] = L.cap_e;
    T.kinds[(L.kind & kKindMask) - 1]++;
  }
  const uint64_t block = 256, nb = (nl + block - 1) / block;
  std::vector<uint32_t> sb_tax(nb + 1, 0), sb_pid(nb + 1, 0), sbb_tax(nb + 1, 0), sbb_pid(nb + 1, 0);
  std::vector<uint64_t> sb_ev(nb + 1, 0), sbb_ev(nb + 1, 0);
  for (uint64_t b : o.units(nb)) {                                                         // k_gb_scan_sums
    for (uint64_t i = b * block; i < std::min<uint64_t>(nl, (b + 1) * block); i++) {
      uint32_t tax, pid; uint64_t ev;
      scan_values(kind[i], (uint32_t)i, &tax, &pid, &ev);
      sb_tax[b] = std::max(sb_tax[b], tax); sb_pid[b] = std::max(sb_pid[b], pid); sb_ev[b] = std::max(sb_ev[b], ev);
    }
  }
  for (uint64_t b = 0; b < nb; b++) {                                                      // k_gb_scan_top
    sbb_tax[b] = T.fin_tax; sbb_pid[b] = T.fin_pid; sbb_ev[b] = T.fin_ev;
    T.fin_tax = std::max(T.fin_tax, sb_tax[b]); T.fin_pid = std::max(T.fin_pid, sb_pid[b]); T.fin_ev = std::max(T.fin_ev, sb_ev[b]);
  }
  for (uint64_t b : o.units(nb)) {                                                         // k_gb_scan_apply
    uint32_t x_tax = sbb_tax[b], x_pid = sbb_pid[b];
    uint64_t x_ev = sbb_ev[b];
    for (uint64_t i = b * block; i < std::min<uint64_t>(nl, (b + 1) * block); i++) {
      tax_src[i] = x_tax; pid_src[i] = x_pid; in_t[i] = (uint8_t)inside(x_ev, G->carry);
      uint32_t tax, pid; uint64_t ev;
      scan_values(kind[i], (uint32_t)i, &tax, &pid, &ev);
      x_tax = std::max(x_tax, tax); x_pid = std::max(x_pid, pid); x_ev = std::max(x_ev, ev);
    }
  }
  const View V{X.p, X.line_start.data(), kind.data(), cap_a.data(), cap_e.data(), tax_src.data(), pid_src.data(), in_t.data(), &G->carry, G->tax.data(), G->pid.data(), nl};
  std::vector<uint64_t> olen(nl + 1, 0), line_off(nl + 1, 0);
  for (uint64_t i : o.units(nl)) {                                                         // k_gb_len
    if (lacks_taxon(V, (uint32_t)i) && (uint32_t)i + 1 < T.no_tax_line) T.no_tax_line = (uint32_t)i + 1;
    const Out q = line_out(V, (uint32_t)i);
    olen[i] = q.hdr + q.seq;
    if (q.hdr) T.records++;
    if (q.seq) { T.kept += q.seq - 1; T.dropped += q.span - (q.seq - 1); }
  }
  emu::scan_offsets(o, olen.data(), nl, 256, line_off.data());
  const uint64_t cap = T.no_tax_line != kNone ? 0 : out_cap;                               // k_gb_write
  emu::write_blocks(o, line_off.data(), nl, out, cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) {
    return gbk_chunk(c, V, line_off.data(), lo, hi, total, cap, v);
  });
  *info = finish(V, line_off.data(), out_cap, T, G->carry);                                // k_gb_finish
  if (T.advance) {                                                                         // k_gb_carry
    if (T.fin_tax) for (uint64_t p : o.units(cap_e[T.fin_tax - 1] - cap_a[T.fin_tax - 1])) G->tax[p] = X.p[cap_a[T.fin_tax - 1] + p];
    if (T.fin_pid) for (uint64_t p : o.units(cap_e[T.fin_pid - 1] - cap_a[T.fin_pid - 1])) G->pid[p] = X.p[cap_a[T.fin_pid - 1] + p];
  }
  return 0;
}

}  // extern "C"
