// krona_emu.cpp — the passes of kaiju_amd/csrc/krona.hip on the host: the per-lane functions of kj_krona.h, driven work unit by
// work unit as tests/emu/tally_emu.cpp does for kj_tally.h.  The units of a pass run in the order the caller asks for (forward,
// reversed, shuffled): no pass may depend on it.  The counts come from the caller per taxon id, so any pattern of direct[] can
// be injected.  The output lies in a 16-byte aligned buffer of its own with guard bytes behind out_cap, which are looked at
// after the write pass.  krona_emu_check_tables reads the tables as the write pass reads them (kjk::locate, byte by byte) and
// compares with the tool's walk done with strings.  It is compiled together with kaiju_amd/csrc/taxon_names.cpp, whose loader
// and tables it uses.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kaiju_amd/csrc/kj_krona.h"
#include "../../kaiju_amd/csrc/taxon_names.h"
#include "../../kaiju_amd/csrc/host/table_rows.h"
#include "lines_emu.h"

using namespace kjk;
using emu::Order;

namespace {

constexpr uint32_t kGuard = 64;

struct Krona {
  const kaiju_taxon_names *names;
  Tab T;
  std::vector<uint8_t> keep, own_ok, listed;
  std::vector<uint32_t> anc_len;
  std::vector<std::string> list;
  uint64_t longest = 0;
};

std::string name_of(const kaiju_taxon_names &N, uint32_t a) { return std::string(reinterpret_cast<const char *>(N.blob.data()) + N.name_pos[a], N.name_len[a]); }

// the names above slot s as the tool collects them (kaiju2krona.cpp:171-182), each with its tab in front
std::string lineage_above(const Krona &K, uint32_t s) {
  const kaiju_taxon_names &N = *K.names;
  auto listed = [&](uint32_t a) { return !K.T.has_list || std::find(K.list.begin(), K.list.end(), N.rank_names[N.rank_of[a]]) != K.list.end(); };
  std::string text;
  for (uint32_t a = s; N.parent[a] != a;) {
    const uint32_t p = N.parent[a];
    if (p == kjn::kNone) {
      if (N.dang_len[a] && !K.T.has_list) text = "\t" + std::string(reinterpret_cast<const char *>(N.dang_blob.data()) + N.dang_pos[a], N.dang_len[a]) + text;
      break;
    }
    if (!(N.name_len[p] & kjn::kGenerated) && listed(p)) text = "\t" + name_of(N, p) + text;
    a = p;
  }
  return text;
}

}  // namespace

extern "C" void krona_emu_constants(uint32_t *out) { out[0] = kjf::kBlockBytes; out[1] = kChunk; out[2] = sizeof(kaiju_gpu_krona_info); out[3] = kMaxTallies; out[4] = kGuard; }

// ranks_csv: NULL: no list.  NULL: a lineage of kMaxLineage bytes or more, or too many items
extern "C" void *krona_emu_create(const kaiju_taxon_names *names, const char *ranks_csv, int order, uint32_t seed) {
  Order o{order, std::mt19937(seed)};
  const kaiju_taxon_names &N = *names;
  const uint32_t cap = (uint32_t)N.key.size();
  Krona *K = new Krona{names, {}, {}, {}, {}, {}, {}};
  K->list = kjtr::split_ranks(ranks_csv ? ranks_csv : "");
  if (K->list.size() > kjn::kMaxList) { delete K; return nullptr; }
  K->listed.assign(N.rank_names.size() + 1, 0);
  for (size_t r = 0; r < N.rank_names.size(); r++) K->listed[r] = std::find(K->list.begin(), K->list.end(), N.rank_names[r]) != K->list.end();
  K->keep.assign(cap, 0xa7); K->own_ok.assign(cap, 0xa7); K->anc_len.assign(cap, 0xdeadbeefu);
  Tab &T = K->T;
  T.key = N.key.data(); T.parent = N.parent.data(); T.name_pos = N.name_pos.data(); T.name_len = N.name_len.data(); T.blob = N.blob.data();
  T.dang_pos = N.dang_pos.data(); T.dang_len = N.dang_len.data(); T.dang_blob = N.dang_blob.data();
  T.keep = K->keep.data(); T.own_ok = K->own_ok.data(); T.anc_len = K->anc_len.data();
  T.cap = cap; T.has_list = ranks_csv ? 1 : 0;
  for (uint64_t s : o.units(cap)) K->keep[s] = build_keep(T, N.rank_of.data(), K->listed.data(), (uint32_t)s);      // k_kr_keep
  for (uint64_t s : o.units(cap)) {                                                                                   // k_kr_tables
    const uint64_t len = build_anc_len(T, (uint32_t)s);
    K->anc_len[s] = kjn::clamp32(len);
    K->own_ok[s] = build_own_ok(T, (uint32_t)s);
    K->longest = std::max(K->longest, len);
  }
  if (K->longest >= kMaxLineage) { delete K; return nullptr; }
  return K;
}
extern "C" void krona_emu_free(void *h) { delete static_cast<Krona *>(h); }
extern "C" uint64_t krona_emu_longest(void *h) { return static_cast<Krona *>(h)->longest; }

// every byte of the lineage above every node through kjk::locate - fresh for every byte, and with the piece of the byte
// before as the write pass keeps it - against the walk with strings.  Returns the bytes compared, -1 - slot for a mismatch
extern "C" int64_t krona_emu_check_tables(void *h) {
  const Krona &K = *static_cast<Krona *>(h);
  const kaiju_taxon_names &N = *K.names;
  int64_t seen = 0;
  for (uint32_t s = 0; s < K.T.cap; s++) {
    if (N.key[s] == ~0ull) { if (K.anc_len[s] || K.keep[s] || K.own_ok[s]) return -1 - (int64_t)s; continue; }
    const std::string want = lineage_above(K, s);
    if (above(K.T, s) != want.size()) return -1 - (int64_t)s;
    Piece kept{0, 0, nullptr};
    for (uint32_t q = 0; q < want.size(); q++) {
      const Piece P = locate(K.T, s, q);
      if (q >= kept.end || q < kept.start) kept = P;
      if (P.start > q || q >= P.end || kept.start != P.start || kept.end != P.end) return -1 - (int64_t)s;
      const uint8_t byte = q == P.start ? '\t' : P.name[q - P.start - 1];
      if (byte != (uint8_t)want[q]) return -1 - (int64_t)s;
      seen++;
    }
  }
  return seen;
}

// ids[i] holds counts[i] reads (an id that is no node counts nowhere; an id given twice adds up, as two tallies do).
// out: out_cap bytes of the caller.  order: 0 forward, 1 reversed, 2 shuffled (seed).  -3: a byte at or behind out_cap was touched
extern "C" int krona_emu_text(void *h, const uint64_t *ids, const uint64_t *counts, uint32_t n_ids, uint64_t n_unclassified, int count_unclassified, uint8_t *out,
                              uint64_t out_cap, kaiju_gpu_krona_info *info, int order, uint32_t seed) {
  const Krona &K = *static_cast<Krona *>(h);
  const Tab &T = K.T;
  Order o{order, std::mt19937(seed)};
  const uint32_t cap = T.cap;
  std::vector<uint64_t> direct(cap, 0);
  for (uint32_t i = 0; i < n_ids; i++) {
    const uint32_t s = kjn::find_slot(T.key, cap - 1, ids[i]);
    if (s != kNone) direct[s] += counts[i];
  }
  // ---- select (k_kr_select), compact (k_kr_compact), plan (k_kr_plan) ----
  std::vector<uint32_t> flag(cap, 0xdeadbeefu), sel((size_t)cap + 1, 0xdeadbeefu), llen((size_t)cap + 1, 0xdeadbeefu);
  std::vector<uint64_t> pos((size_t)cap + 1, 0xdeadbeefdeadbeefull), cnt((size_t)cap + 1, 0xdeadbeefdeadbeefull), line_off((size_t)cap + 2, 0xdeadbeefdeadbeefull);
  uint64_t taxa = 0, reads = 0;
  for (uint64_t s : o.units(cap)) {
    uint32_t unnamed;
    flag[s] = selects(T, (uint32_t)s, direct[s], &unnamed);
    taxa += unnamed;
    reads += unnamed ? direct[s] : 0;
  }
  emu::scan_offsets(o, flag.data(), cap, 256, pos.data());
  for (uint64_t s : o.units(cap))
    if (flag[s]) { sel[pos[s]] = (uint32_t)s; cnt[pos[s]] = direct[s]; }
  uint32_t n = (uint32_t)pos[cap];
  const uint64_t u = count_unclassified ? n_unclassified : 0;
  if (u) { sel[n] = kNone; cnt[n] = u; n++; }
  // ---- len (k_kr_len), offsets ----
  for (uint64_t r : o.units(n)) llen[r] = line_len(T, sel[r], cnt[r]);
  emu::scan_offsets(o, llen.data(), n, 256, line_off.data());
  // ---- write (k_kr_write) ----
  const uint64_t padded = (out_cap + kChunk - 1) / kChunk * kChunk + kGuard;
  void *mem = nullptr;
  if (posix_memalign(&mem, kChunk, padded) != 0) return -6;
  uint8_t *buf = static_cast<uint8_t *>(mem);
  memset(buf, 0x5a, padded);
  emu::write_blocks(o, line_off.data(), n, buf, out_cap, [&](uint64_t c, uint32_t lo, uint32_t hi, uint64_t total, Chunk *v) {
    return format_chunk(c, T, line_off.data(), sel.data(), cnt.data(), lo, hi, total, out_cap, v);
  });
  // ---- finish (k_kr_finish) ----
  *info = make_info(line_off.data(), n, out_cap, taxa, reads, u);
  int rc = 0;
  for (uint64_t i = info->written_bytes; i < padded; i++)
    if (buf[i] != 0x5a) rc = -3;                                  // (behind the lines that fit, not only behind out_cap)
  if (out_cap) memcpy(out, buf, out_cap);
  free(mem);
  return rc;
}
