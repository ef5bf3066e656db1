// format_names_emu.cpp — the passes of kaiju_amd/csrc/format_names.hip on the host: the per-lane functions of kj_format_names.h,
// driven work unit by work unit as tests/emu/format_emu.cpp does for kj_format.h.  The units of a pass run in the order the
// caller asks for (forward, reversed, shuffled): no pass may depend on it.  It is compiled together with
// kaiju_amd/csrc/taxon_names.cpp, whose tables it reads; the tables the device builds at upload (k_fn_tables) are built here
// by the same functions, one slot at a time.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/kj_format_names.h"
#include "../../kaiju_amd/csrc/taxon_names.h"
#include "lines_emu.h"

using namespace kjn;
using emu::Order;

namespace {

struct Built {
  Tab T{};
  std::vector<uint32_t> path_len, rank_src, rank_len;
  uint64_t max_annotation = 0;
};

// k_fn_tables
void build(const kaiju_taxon_names &N, Built &B, Order &o) {
  Tab &T = B.T;
  const uint32_t cap = (uint32_t)N.key.size();
  T.key = N.key.data(); T.parent = N.parent.data(); T.name_pos = N.name_pos.data(); T.name_len = N.name_len.data();
  T.rank = N.rank.data(); T.blob = N.blob.data();
  T.cap_mask = cap - 1; T.mode = (uint32_t)N.mode; T.n_ranks = (uint32_t)N.ranks.size(); T.n_list = (uint32_t)N.list.size();
  for (uint32_t j = 0; j < T.n_list; j++) T.list[j] = N.list[j];
  B.path_len.assign(cap, 0xdeadbeefu); B.rank_len.assign(cap, 0xdeadbeefu); B.rank_src.assign((size_t)cap * std::max(1u, T.n_ranks), 0xdeadbeefu);
  for (uint64_t s64 : o.units(cap)) {
    const uint32_t s = (uint32_t)s64;
    uint64_t len = 0;
    if (T.mode == KAIJU_NAMES_PATH) { len = build_path_len(T, s); B.path_len[s] = clamp32(len); }
    else if (T.mode == KAIJU_NAMES_RANKS) { len = build_ranks(T, s, B.rank_src.data() + (size_t)s * T.n_ranks); B.rank_len[s] = clamp32(len); }
    else if (T.key[s] != ~0ull && !(T.name_len[s] & kGenerated)) len = T.name_len[s];
    B.max_annotation = std::max(B.max_annotation, len);
  }
  T.path_len = B.path_len.data(); T.rank_src = B.rank_src.data(); T.rank_len = B.rank_len.data();
}

}  // namespace

extern "C" void format_names_emu_constants(uint32_t *out) { out[0] = kBlockBytes; out[1] = kScanBlock; out[2] = kChunk; out[3] = kjf::kPowK; }

// the tables of `names` as the upload builds them.  which: 4 path_len, 5 rank_len, 6 rank_src (as kaiju_gpu_taxon_names_read); 0 .. 3, 7:
// the host's own.  Returns the number of slots, *max_annotation as the upload reads it back; out may be NULL
extern "C" int64_t format_names_emu_table(const kaiju_taxon_names *names, int which, void *out, uint64_t out_bytes, uint64_t *max_annotation, int order,
                                          uint32_t seed) {
  if (!names) return -1;
  Order o{order, std::mt19937(seed)};
  Built B;
  build(*names, B, o);
  if (max_annotation) *max_annotation = B.max_annotation;
  const void *src = nullptr;
  size_t bytes = 0;
  switch (which) {
    case 0: src = names->key.data(); bytes = names->key.size() * 8; break;
    case 1: src = names->parent.data(); bytes = names->parent.size() * 4; break;
    case 2: src = names->name_pos.data(); bytes = names->name_pos.size() * 4; break;
    case 3: src = names->name_len.data(); bytes = names->name_len.size() * 4; break;
    case 4: if (names->mode != KAIJU_NAMES_PATH) return -1; src = B.path_len.data(); bytes = B.path_len.size() * 4; break;
    case 5: if (names->mode != KAIJU_NAMES_RANKS) return -1; src = B.rank_len.data(); bytes = B.rank_len.size() * 4; break;
    case 6: if (names->mode != KAIJU_NAMES_RANKS) return -1; src = B.rank_src.data(); bytes = (size_t)names->key.size() * B.T.n_ranks * 4; break;
    case 7: src = names->rank.data(); bytes = names->rank.size(); break;
    default: return -1;
  }
  if (out && out_bytes) memcpy(out, src, std::min<size_t>(bytes, out_bytes));
  return (int64_t)names->key.size();
}

// the annotation of `taxon` read byte by byte through the tables (locate / entry_byte): what the write pass prints.  Returns its
// length, -1: none
extern "C" int64_t format_names_emu_annotation(const kaiju_taxon_names *names, uint64_t taxon, uint8_t *buf, uint64_t cap) {
  if (!names) return -2;
  Order o{0, std::mt19937(1)};
  Built B;
  build(*names, B, o);
  uint32_t len, why;
  const uint32_t s = annotation_of(B.T, taxon, &len, &why);
  if (s == kNone) return -1;
  // every byte on its own (a lane that starts in the middle), and a second time in one sweep (the piece carried along)
  Entry E = make_entry(B.T, kNone, 0, 0);
  E.end = 0;
  for (uint32_t q = 0; q < len && q < cap; q++) {
    const Entry F = locate(B.T, s, q);
    if (q >= E.end || q < E.start) E = locate(B.T, s, q);
    const uint32_t a = entry_byte(B.T, F, q), b = entry_byte(B.T, E, q);
    if (a != b) return -3;
    buf[q] = (uint8_t)a;
  }
  return len;
}

// info: the ten 32-bit words of kaiju_gpu_format_names_info.  out: out_cap bytes, changed only where lines are written.
// order: 0 forward, 1 reversed, 2 shuffled (seed).
extern "C" int format_names_emu(const double *pw_in, const kaiju_gpu_compact *recs, const uint64_t *off, uint32_t n, int paired, const uint8_t *text1,
                                uint64_t bytes1, const kaiju_gpu_name_span *names, double db_length, double min_evalue, int gate, int protein,
                                const kaiju_taxon_names *tnames, int drop, uint8_t *out, uint64_t out_cap, uint32_t *info, int order, uint32_t seed) {
  if (!tnames || bytes1 > kjf::kMaxBytes - kMaxAnnotation || n > kjf::kMaxRecords) return -1;
  Order o{order, std::mt19937(seed)};
  std::vector<double> pw(kjf::kPowK);
  if (pw_in) pw.assign(pw_in, pw_in + kjf::kPowK);
  else if (!kjf::build_pow_table(pw.data(), kjf::kPowK)) return -7;
  Built B;
  build(*tnames, B, o);
  if (B.max_annotation >= kMaxAnnotation) return -8;
  const Tab &T = B.T;
  Params P{};
  P.db_length = db_length; P.min_evalue = min_evalue; P.gate = gate; P.protein = protein; P.paired = paired;
  std::vector<uint32_t> llen((size_t)n + 1, 0xdeadbeefu), aslot((size_t)n + 1, 0xdeadbeefu);
  std::vector<uint64_t> line_off((size_t)n + 1, 0xdeadbeefdeadbeefull), tax((size_t)n + 1, 0xdeadbeefdeadbeefull);
  uint32_t n_classified = 0, n_inexact = 0, count[4] = {0, 0, 0, 0};
  for (uint64_t r64 : o.units(n)) {                                           // k_fn_len
    const uint32_t r = (uint32_t)r64;
    uint64_t t;
    uint32_t slot, why;
    llen[r] = record_line(recs, off, names, r, bytes1, P, pw.data(), T, drop, &t, &slot, &why);
    tax[r] = t; aslot[r] = slot;
    n_classified += t ? 1 : 0;
    n_inexact += (recs[r].info & KAIJU_HIT_INEXACT) ? 1 : 0;
    count[why]++;
  }
  emu::scan_offsets(o, llen.data(), n, kScanBlock, line_off.data());          // kjl::k_scan_sums / _top / _apply
  const uint64_t total = line_off[n];
  // the output as the device sees it: 16-byte aligned, and not one byte longer than out_cap
  void *mem = nullptr;
  if (posix_memalign(&mem, kChunk, std::max<uint64_t>(out_cap, 1)) != 0) return -6;
  uint8_t *dev_out = static_cast<uint8_t *>(mem);
  if (out_cap) memcpy(dev_out, out, out_cap);
  emu::write_blocks(o, line_off.data(), n, dev_out, out_cap,                  // k_fn_write
                    [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) { return format_chunk(c, text1, bytes1, names, line_off.data(), tax.data(), aslot.data(), T, lo, hi, total, out_cap, v); });
  if (out_cap) memcpy(out, dev_out, out_cap);
  free(mem);
  const kaiju_gpu_format_names_info fi = make_info(total, n, n_classified, n_inexact, out_cap, count[kWhyUnknown], count[kWhyUnnamed], count[kWhyDropped]);   // k_fn_finish
  memcpy(info, &fi, sizeof fi);
  return 0;
}
