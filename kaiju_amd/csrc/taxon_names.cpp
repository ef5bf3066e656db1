// taxon_names.cpp — host side of the fourth column: nodes.dmp and names.dmp as kaiju-addTaxonNames reads them
// (parseNodesDmpWithRank and parseNamesDmp, util.cpp:123-179 of the reference), laid out as the slot tables of kj_format_names.h.
//
// The node set is NOT that of taxonomy.cpp: here a line without a lower-case letter behind the parent is no node at all (the
// reference's substr throws and the line is skipped), there only the two numbers count.
//
//   nodes.dmp   per line: the leading run of digits is the id (none, or a number beyond 64 bits: the line is skipped), the
//               next run of digits the parent, the rank the run of [a-z ] from the first lower-case letter behind the parent
//               (none: skipped).  First line per id wins
//   names.dmp   only lines that contain "scientific name" anywhere.  The id is the first run of digits of the line, the name
//               starts at the first byte behind it that is neither tab nor '|' and ends in front of the next tab or '|'.  First
//               such line per id wins
// Lines end at '\n' only (getline); every other byte, '\r' and NUL included, is text.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/kaiju_gpu.h"
#include "kj_format_names.h"
#include "taxon_names.h"
#include "host/table_rows.h"

using namespace kjn;

// capi.hip keeps the text of kaiju_gpu_last_error(); a program linked without it has kaiju_taxon_names_last_error() alone
extern "C" __attribute__((weak)) void kj_set_last_error(const char *msg);

namespace {

thread_local std::string tl_names_error;
int fail(int code, const std::string &msg) {
  tl_names_error = msg;
  if (kj_set_last_error) kj_set_last_error(msg.c_str());
  return code;
}

bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
bool is_lower(uint8_t c) { return c >= 'a' && c <= 'z'; }
// digits [b, e) as a number; false beyond 64 bits (stoul throws out_of_range: the line is skipped)
bool number(const uint8_t *b, const uint8_t *e, uint64_t *out) {
  uint64_t v = 0;
  for (; b < e; b++) {
    const uint64_t d = (uint64_t)(*b - '0');
    if (v > (0xffffffffffffffffull - d) / 10) return false;
    v = v * 10 + d;
  }
  *out = v;
  return true;
}
int read_file(const char *path, std::vector<uint8_t> &out) {
  FILE *fp = fopen(path, "rb");
  if (!fp) return fail(KAIJU_GPU_ERR_IO, std::string("could not open ") + path);
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, fp)) > 0) out.insert(out.end(), buf, buf + n);
  const bool bad = ferror(fp) != 0;
  fclose(fp);
  return bad ? fail(KAIJU_GPU_ERR_IO, std::string("could not read ") + path) : KAIJU_GPU_OK;
}
template <class F>
void each_line(const std::vector<uint8_t> &text, F &&f) {
  const uint8_t *p = text.data(), *end = p + text.size();
  while (p < end) {
    const uint8_t *nl = static_cast<const uint8_t *>(memchr(p, '\n', (size_t)(end - p)));
    const uint8_t *e = nl ? nl : end;
    if (e > p) f(p, e);
    p = nl ? nl + 1 : end;
  }
}

struct Node { uint64_t parent; std::string rank; };

}  // namespace

extern "C" const char *kaiju_taxon_names_last_error(void) { return tl_names_error.c_str(); }

static int load(const char *nodes_dmp, const char *names_dmp, int mode, const char *ranks_csv, kaiju_taxon_names **out) {
  if (!nodes_dmp || !names_dmp || !out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  *out = nullptr;
  if (mode != KAIJU_NAMES_NAME && mode != KAIJU_NAMES_PATH && mode != KAIJU_NAMES_RANKS) return fail(KAIJU_GPU_ERR_ARG, "unknown mode");
  kaiju_taxon_names *raw = new kaiju_taxon_names();
  struct Guard { kaiju_taxon_names *p; ~Guard() { delete p; } } guard{raw};
  kaiju_taxon_names &N = *raw;
  N.mode = mode;
  // the list of ranks: items between commas, empty ones ignored; a rank listed twice is printed twice
  if (mode == KAIJU_NAMES_RANKS) {
    const std::string csv = ranks_csv ? ranks_csv : "";
    size_t b = 0;
    while (b <= csv.size()) {
      size_t c = csv.find(',', b);
      if (c == std::string::npos) c = csv.size();
      if (c > b) {
        const std::string item = csv.substr(b, c - b);
        size_t k = 0;
        while (k < N.ranks.size() && N.ranks[k] != item) k++;
        if (k == N.ranks.size()) {
          if (k == kMaxRanks) return fail(KAIJU_GPU_ERR_ARG, "more than 16 distinct ranks in the list");
          N.ranks.push_back(item);
        }
        if (N.list.size() == kMaxList) return fail(KAIJU_GPU_ERR_ARG, "more than 64 items in the list of ranks");
        N.list.push_back((uint8_t)k);
      }
      b = c + 1;
    }
  }

  std::vector<uint8_t> text;
  if (int rc = read_file(nodes_dmp, text)) return rc;
  std::unordered_map<uint64_t, Node> nodes;
  std::vector<uint64_t> order;                        // ids in file order: the table does not depend on the map's order
  each_line(text, [&](const uint8_t *p, const uint8_t *e) {
    const uint8_t *q = p;
    while (q < e && is_digit(*q)) q++;
    uint64_t id, parent;
    if (q == p || q == e || !number(p, q, &id)) return;
    while (q < e && !is_digit(*q)) q++;
    if (q == e) return;
    const uint8_t *s = q;
    while (q < e && is_digit(*q)) q++;
    if (!number(s, q, &parent)) return;
    while (q < e && !is_lower(*q)) q++;
    if (q == e) return;
    s = q;
    while (q < e && (is_lower(*q) || *q == ' ')) q++;
    if (nodes.emplace(id, Node{parent, std::string(reinterpret_cast<const char *>(s), (size_t)(q - s))}).second) order.push_back(id);
  });
  if (order.size() > 0x3fffffffull) return fail(KAIJU_GPU_ERR_ARG, "too many nodes");
  uint32_t cap = 16;
  while ((uint64_t)cap < 2 * (uint64_t)order.size() + 2) cap <<= 1;
  N.key.assign(cap, ~0ull);
  N.parent.assign(cap, kNone);
  N.name_pos.assign(cap, 0);
  N.name_len.assign(cap, kGenerated);
  N.rank.assign(cap, (uint8_t)kNoRank);
  N.n_nodes = order.size();
  N.rank_of.assign(cap, 0);
  N.dang_pos.assign(cap, 0);
  N.dang_len.assign(cap, 0);
  std::unordered_map<uint64_t, std::vector<uint32_t>> orphans;    // a parent id that is no node -> the slots below it
  std::unordered_map<std::string, uint16_t> rank_index;
  for (uint64_t id : order) {
    if (id == ~0ull) return fail(KAIJU_GPU_ERR_ARG, "taxon id 2^64 - 1 cannot be a node");
    uint32_t s = hash_id(id) & (cap - 1);
    while (N.key[s] != ~0ull) s = (s + 1) & (cap - 1);
    N.key[s] = id;
  }
  for (uint64_t id : order) {
    const uint32_t s = find_slot(N.key.data(), cap - 1, id);
    const Node &nd = nodes[id];
    N.parent[s] = find_slot(N.key.data(), cap - 1, nd.parent);
    if (N.parent[s] == kNone) orphans[nd.parent].push_back(s);
    N.name_len[s] = kGenerated | (8 + kjf::digits_u64(id));
    const auto ri = rank_index.emplace(nd.rank, (uint16_t)N.rank_names.size());
    if (ri.second) {
      if (N.rank_names.size() == 0xffff) return fail(KAIJU_GPU_ERR_ARG, "more than 65535 distinct ranks");
      N.rank_names.push_back(nd.rank);
    }
    N.rank_of[s] = ri.first->second;
    if (nd.rank != "no rank")
      for (size_t k = 0; k < N.ranks.size(); k++)
        if (N.ranks[k] == nd.rank) N.rank[s] = (uint8_t)k;
  }
  // a cycle other than a self-parent: the reference would never leave its walk
  {
    std::vector<uint8_t> state(cap, 0);               // 1: on the walk in progress, 2: known to end
    std::vector<uint32_t> walk;
    for (uint32_t s0 = 0; s0 < cap; s0++) {
      if (N.key[s0] == ~0ull || state[s0]) continue;
      walk.clear();
      for (uint32_t a = s0; a != kNone && state[a] != 2; a = N.parent[a]) {
        if (state[a] == 1) return fail(KAIJU_GPU_ERR_ARG, "the tree has a cycle through node " + std::to_string(N.key[a]));
        state[a] = 1;
        walk.push_back(a);
        if (N.parent[a] == a) break;
      }
      for (uint32_t a : walk) state[a] = 2;
    }
  }

  text.clear();
  if (int rc = read_file(names_dmp, text)) return rc;
  static const char kMark[] = "scientific name";
  bool too_long = false;
  each_line(text, [&](const uint8_t *p, const uint8_t *e) {
    if (!memmem(p, (size_t)(e - p), kMark, sizeof kMark - 1)) return;
    const uint8_t *q = p;
    while (q < e && !is_digit(*q)) q++;
    if (q == e) return;
    const uint8_t *s = q;
    while (q < e && is_digit(*q)) q++;
    uint64_t id;
    if (q == e || !number(s, q, &id)) return;
    while (q < e && (*q == '\t' || *q == '|')) q++;
    if (q == e) return;
    s = q++;
    while (q < e && *q != '\t' && *q != '|') q++;
    const uint32_t slot = find_slot(N.key.data(), cap - 1, id);
    if (slot == kNone) {                                                      // no node: kaiju2krona prints it above its orphans
      const auto o = orphans.find(id);
      if (o == orphans.end() || N.dang_len[o->second[0]]) return;
      if ((uint64_t)(q - s) >= kMaxAnnotation || N.dang_blob.size() + (size_t)(q - s) > 0xfffffff0ull) {   // (kaiju_gpu_krona_create refuses it)
        for (uint32_t below : o->second) N.dang_len[below] = kNone;
        return;
      }
      for (uint32_t below : o->second) { N.dang_pos[below] = (uint32_t)N.dang_blob.size(); N.dang_len[below] = (uint32_t)(q - s); }
      N.dang_blob.insert(N.dang_blob.end(), s, q);
      return;
    }
    if (!(N.name_len[slot] & kGenerated)) return;                             // it has its name
    if ((uint64_t)(q - s) >= kMaxAnnotation || N.blob.size() + (size_t)(q - s) > 0xfffffff0ull) { too_long = true; return; }
    N.name_pos[slot] = (uint32_t)N.blob.size();
    N.name_len[slot] = (uint32_t)(q - s);
    N.blob.insert(N.blob.end(), s, q);
    N.n_named++;
  });
  if (too_long) return fail(KAIJU_GPU_ERR_ARG, "a name of 2^24 bytes or more, or 4 GiB of names");
  N.blob.resize(N.blob.size() + 16, 0);               // (never read: room for an aligned load at the end)
  N.dang_blob.resize(N.dang_blob.size() + 16, 0);
  guard.p = nullptr;
  *out = raw;
  return KAIJU_GPU_OK;
}

extern "C" int kaiju_taxon_names_load(const char *nodes_dmp, const char *names_dmp, int mode, const char *ranks_csv, kaiju_taxon_names **out) {
  try { return load(nodes_dmp, names_dmp, mode, ranks_csv, out); }
  catch (const std::bad_alloc &) { return fail(KAIJU_GPU_ERR_NOMEM, "out of host memory"); }
  catch (const std::exception &e) { return fail(KAIJU_GPU_ERR_ARG, std::string("unexpected error: ") + e.what()); }
}

extern "C" void kaiju_taxon_names_free(kaiju_taxon_names *names) { delete names; }

extern "C" uint64_t kaiju_taxon_names_count(const kaiju_taxon_names *names, int named) { return !names ? 0 : named ? names->n_named : names->n_nodes; }

// the rules of kaiju-addTaxonNames.cpp:161-227 with strings, as the tool has them
extern "C" int64_t kaiju_taxon_names_annotation(const kaiju_taxon_names *names, uint64_t taxon, char *buf, uint64_t cap) {
  if (!names || (!buf && cap)) return -1;
  try {
    const kaiju_taxon_names &N = *names;
    const uint32_t mask = (uint32_t)N.key.size() - 1;
    const uint32_t s = find_slot(N.key.data(), mask, taxon);
    if (s == kNone || (N.name_len[s] & kGenerated)) return -1;
    auto name_of = [&](uint32_t a) {
      if (N.name_len[a] & kGenerated) return "taxonid:" + std::to_string(N.key[a]);
      return std::string(reinterpret_cast<const char *>(N.blob.data()) + N.name_pos[a], N.name_len[a]);
    };
    std::string text;
    if (N.mode == KAIJU_NAMES_NAME) text = name_of(s);
    else {
      std::vector<std::string> value(N.ranks.size(), "NA");
      for (uint32_t a = s; a != kNone && N.parent[a] != a; a = N.parent[a]) {
        if (N.mode == KAIJU_NAMES_PATH) text = name_of(a) + "; " + text;
        else if (N.rank[a] != kNoRank) value[N.rank[a]] = name_of(a);
      }
      if (N.mode == KAIJU_NAMES_RANKS)
        for (uint8_t k : N.list) text += value[k] + "; ";
    }
    if (cap && !text.empty()) memcpy(buf, text.data(), text.size() < cap ? text.size() : (size_t)cap);
    return (int64_t)text.size();
  } catch (const std::exception &) { return -1; }
}

// the rows of kaiju2table (host/table_rows.h) behind the C interface
extern "C" int kaiju_table_rows(const kaiju_taxon_names *names, const kaiju_gpu_tally_entry *entries, uint64_t n_entries, const kaiju_gpu_tally_info *totals,
                                const kaiju_table_options *opt, const char *label, char *buf, uint64_t cap, uint64_t *n_bytes) {
  if (!names || (!entries && n_entries) || !totals || !opt || !opt->rank || !label || (!buf && cap) || !n_bytes) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  try {
    kjtr::Options o;
    o.rank = opt->rank;
    o.has_list = opt->ranks_csv && *opt->ranks_csv;
    if (o.has_list) o.list = kjtr::split_ranks(opt->ranks_csv);
    o.min_percent = opt->min_percent;
    o.min_count = opt->min_count;
    o.expand_viruses = opt->flags & KAIJU_TABLE_EXPAND_VIRUSES;
    o.filter_unclassified = opt->flags & KAIJU_TABLE_FILTER_UNCLASSIFIED;
    o.full_path = opt->flags & KAIJU_TABLE_FULL_PATH;
    if (const char *why = kjtr::refusal(o)) return fail(KAIJU_GPU_ERR_ARG, why);
    const std::string text = kjtr::table_rows(*names, entries, n_entries, *totals, o, label);
    *n_bytes = text.size();
    if (cap && !text.empty()) memcpy(buf, text.data(), text.size() < cap ? text.size() : (size_t)cap);
    return KAIJU_GPU_OK;
  }
  catch (const std::bad_alloc &) { return fail(KAIJU_GPU_ERR_NOMEM, "out of host memory"); }
  catch (const std::exception &e) { return fail(KAIJU_GPU_ERR_ARG, std::string("unexpected error: ") + e.what()); }
}
