// table_rows.h — the rows of kaiju2table for one input file: no GPU, no I/O.  (entries and totals of kaiju_gpu_tally_result,
// options, the host tables of taxon_names.h, the label of the file column) -> the bytes the tool prints for that file.
// taxon_names.cpp exports it as kaiju_table_rows; table_main.cpp and api.table_text go through that entry.
//
// The rules are those of kaiju2table.cpp:238-360 of the reference, observed on the unmodified tool:
//   total     n_total, with -u less the unclassified reads
//   kept      every entry at or below 10239, whatever its rank and count.  Every other entry whose rank is -r's: with
//             (int)count >= -c and (float)count / (float)total * 100 >= -m it is kept, else its reads go to one of the two
//             "below threshold" sums; either way they count in the sum at the rank
//   above     total - unclassified (not with -u, where they are out of the total already) - sum at the rank - virus reads,
//             in 64 bits as the tool computes it
//   order     count descending, then id ascending (a multimap filled from a map)
//   rows      the kept entries (those at or below 10239 only with -e), "Viruses" (not with -e), "cannot be assigned ...",
//             the row of -c, the row of -m, "unclassified"
//   percent   the tool's own mixed arithmetic, kept line by line: a float division, then * 100.0f for the entries, * 100.0 in
//             double - rounded to float again for "Viruses" and "cannot be assigned", printed as it is for the last three.
//             An empty file gives 0 / 0 there, which printf spells "-nan" as it does for the tool
//   names     a node's own name or "taxonid:N".  -p: the names from below the root down to the node, ';' behind each.  -l: per
//             item of the list the name of the topmost node of that rank on the way up, "NA" without one, ';' behind each;
//             nodes of rank "no rank" never supply a value
// These are not the strings of kj_format_names.h ("; ", no "taxonid:" for the node itself), so they are composed here.
#ifndef KJ_TABLE_ROWS_H
#define KJ_TABLE_ROWS_H

#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../kj_tally.h"
#include "../taxon_names.h"

namespace kjtr {

struct Options {
  std::string rank;
  bool has_list = false;               // -l given (and not empty)
  std::vector<std::string> list;       // its items, empty ones left out
  float min_percent = 0.0f;
  int min_count = 0;
  bool expand_viruses = false, filter_unclassified = false, full_path = false;
};

// the items of -l between commas, empty ones ignored
inline std::vector<std::string> split_ranks(const std::string &csv) {
  std::vector<std::string> out;
  size_t b = 0;
  while (b <= csv.size()) {
    size_t c = csv.find(',', b);
    if (c == std::string::npos) c = csv.size();
    if (c > b) out.push_back(csv.substr(b, c - b));
    b = c + 1;
  }
  return out;
}

// why the tool refuses these options (it prints its usage and fails), nullptr: it does not.  In the tool's order
inline const char *refusal(const Options &o) {
  static const char *const kRanks[] = {"phylum", "class", "order", "family", "genus", "species"};
  if (o.rank.empty()) return "Please specify the rank (phylum, class, order, family, genus, or species) with the -r option.";
  if (o.has_list && o.full_path) return "Please use either option -p or -l, but not both of them.";
  if (std::find(std::begin(kRanks), std::end(kRanks), o.rank) == std::end(kRanks)) return "Rank must be one of: phylum, class, order, family, genus, species.";
  if (o.min_count < 0) return "Min required read count (-c) must be >= 0";
  if (!(o.min_percent >= 0.0f && o.min_percent <= 100.0f)) return "Min required percent (-m) must be between 0.0 and 100.0";
  if (o.min_percent > 0.0f && o.min_count > 0) return "Either specify minimum percent with -m or minimum read count with -c.";
  if (o.has_list && std::find(o.list.begin(), o.list.end(), o.rank) == o.list.end()) return "The rank of -r is not contained in the rank list supplied with option -l";
  return nullptr;
}

inline std::string name_of(const kaiju_taxon_names &N, uint32_t s) {
  if (N.name_len[s] & kjn::kGenerated) return "taxonid:" + std::to_string(N.key[s]);
  return std::string(reinterpret_cast<const char *>(N.blob.data()) + N.name_pos[s], N.name_len[s]);
}

inline void put(std::string &out, const std::string &label, double percent, uint64_t reads, const std::string &tail) {
  char num[400];                       // (%.6f of a float's largest value has 46 characters)
  snprintf(num, sizeof num, "\t%.6f\t%" PRIu64 "\t", percent, reads);
  out += label;
  out += num;
  out += tail;
  out += '\n';
}

inline std::string table_rows(const kaiju_taxon_names &N, const kaiju_gpu_tally_entry *entries, uint64_t n_entries, const kaiju_gpu_tally_info &totals,
                              const Options &o, const std::string &label) {
  const uint32_t mask = (uint32_t)N.key.size() - 1;
  const uint32_t vslot = kjn::find_slot(N.key.data(), mask, kjt::kVirusTaxon);
  const uint64_t unclassified = totals.n_unclassified, virus_reads = totals.n_virus;
  uint64_t totalreads = totals.n_total;
  if (o.filter_unclassified) totalreads -= unclassified;

  struct Kept { uint64_t count, id; uint32_t slot; bool virus; };
  std::vector<Kept> kept;
  uint64_t at_rank = 0, below_percent = 0, below_count = 0;
  for (uint64_t k = 0; k < n_entries; k++) {
    const uint64_t id = entries[k].taxon, count = entries[k].summed;
    const uint32_t s = kjn::find_slot(N.key.data(), mask, id);
    if (s == kjn::kNone || count == 0) continue;                   // (no entry of this tree)
    if (kjt::is_virus(N.parent.data(), vslot, s)) { kept.push_back(Kept{count, id, s, true}); continue; }
    if (N.rank_names[N.rank_of[s]] != o.rank) continue;
    if ((int)count >= o.min_count) {
      const float percent = (float)count / (float)totalreads * 100;
      if (percent >= o.min_percent) kept.push_back(Kept{count, id, s, false});
      else below_percent += count;
    } else {
      below_count += count;
    }
    at_rank += count;
  }
  uint64_t above = o.filter_unclassified ? totalreads - at_rank : totalreads - unclassified - at_rank;
  above -= virus_reads;
  std::sort(kept.begin(), kept.end(), [](const Kept &a, const Kept &b) { return a.count != b.count ? a.count > b.count : a.id < b.id; });

  std::string out;
  for (const Kept &e : kept) {
    if (!o.expand_viruses && e.virus) continue;
    const float percent = (float)e.count / (float)totalreads * 100.0f;
    std::string tail = std::to_string(e.id) + "\t";
    if (o.has_list) {
      std::vector<std::string> value(o.list.size(), "NA");
      for (uint32_t a = e.slot; a != kjn::kNone && N.parent[a] != a; a = N.parent[a]) {
        const std::string &r = N.rank_names[N.rank_of[a]];
        if (r == "no rank") continue;
        for (size_t i = 0; i < o.list.size(); i++)
          if (o.list[i] == r) value[i] = name_of(N, a);
      }
      for (const std::string &v : value) tail += v + ";";
    } else if (o.full_path) {
      std::string path;
      for (uint32_t a = e.slot; a != kjn::kNone && N.parent[a] != a; a = N.parent[a]) path = name_of(N, a) + ";" + path;
      tail += path;
    } else {
      tail += name_of(N, e.slot);
    }
    put(out, label, percent, e.count, tail);
  }
  if (!o.expand_viruses) {
    const float percent_viruses = virus_reads > 0 ? (float)virus_reads / (float)totalreads * 100.0 : 0.0;
    put(out, label, percent_viruses, virus_reads, std::to_string(kjt::kVirusTaxon) + "\tViruses");
  }
  {
    const float percent_above = above > 0 ? (float)above / (float)totalreads * 100.0 : 0.0;
    put(out, label, percent_above, above, "NA\tcannot be assigned to a (non-viral) " + o.rank);
  }
  if (o.min_count > 0)
    put(out, label, (float)below_count / (float)totalreads * 100.0, below_count,
        "NA\tbelong to a (non-viral) " + o.rank + " having less than " + std::to_string(o.min_count) + " reads");
  if (o.min_percent > 0.0) {
    char g[64];
    snprintf(g, sizeof g, "%g", o.min_percent);
    put(out, label, (float)below_percent / (float)totalreads * 100.0, below_percent, "NA\tbelong to a (non-viral) " + o.rank + " with less than " + g + "% of all reads");
  }
  if (o.filter_unclassified) put(out, label, (float)unclassified / (float)(totalreads + unclassified) * 100.0, unclassified, "NA\tunclassified");
  else put(out, label, (float)unclassified / (float)totalreads * 100.0, unclassified, "NA\tunclassified");
  return out;
}

}  // namespace kjtr

#endif  // KJ_TABLE_ROWS_H
