// table_main.cpp — kaiju2table: a drop-in for the reference's tool over the C-ABI (include/kaiju_gpu.h).
//
//   kaiju2table -t nodes.dmp -n names.dmp -r species -o kaiju.table [-m FLOAT | -c INT] [-e] [-u] [-p | -l rank,rank,...] [-v]
//               input1.tsv [input2.tsv ...]
//
// The options, the failure statuses and every byte of the -o file are the tool's; the wording of the messages on stderr is
// this program's own.  Every input file is read in blocks that end behind a '\n' (annotate_blocks.h) and every block is
// counted on the device (kaiju_gpu_tally_add_text, the rules: csrc/kj_tally.h) by one of two tallies - each with pinned
// staging and a stream of its own, so that the upload of a block overlaps the passes of the one before.  At the end of a file
// the entries of both are added by taxon and kaiju_table_rows (csrc/host/table_rows.h) makes the rows.
//   device               the first entry of KAIJU_GPU_DEVICES (or KAIJU_GPU_DEVICE), else 0
//   KAIJU_TABLE_BLOCK    bytes per block (default 32 MiB; tests force small ones)
// One divergence, on stderr only: where the tool prints a message for every line it cannot count, this prints one summary
// line per file and reason (bad taxon id, id not in the tree) with the number of lines.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <future>
#include <map>
#include <string>
#include <vector>

#include "../../../include/kaiju_gpu.h"
#include "annotate_blocks.h"
#include "table_rows.h"

namespace {

void usage(const char *prog) {
  fprintf(stderr,
          "usage: %s -t nodes.dmp -n names.dmp -r RANK -o FILE [-m FLOAT | -c INT] [-e] [-u] [-p | -l RANK,RANK,...] [-v] FILE [FILE ...]\n"
          "  -t FILE   nodes.dmp of the taxonomy           -n FILE   names.dmp of the taxonomy\n"
          "  -r RANK   phylum, class, order, family, genus or species\n"
          "  -o FILE   where to write the table            FILE ...  outputs of kaiju\n"
          "  -m FLOAT  least percentage of the reads for a taxon to be listed (not viruses), in [0, 100]\n"
          "  -c INT    least number of reads for a taxon to be listed (not viruses); not together with -m\n"
          "  -e        list the viral taxa instead of one row for all viruses\n"
          "  -u        percentages of the classified reads only\n"
          "  -p        print the whole lineage instead of the taxon's name\n"
          "  -l LIST   print the names at these ranks, e.g. -l superkingdom,phylum,genus; it must hold the rank of -r\n"
          "  -v        say what is being done\n",
          prog);
  exit(EXIT_FAILURE);
}

[[noreturn]] void die(const std::string &msg) {
  fprintf(stderr, "Error: %s\n", msg.c_str());
  exit(EXIT_FAILURE);
}

int first_device() {
  const char *e = getenv("KAIJU_GPU_DEVICES");
  if (!e || !strcmp(e, "all")) e = getenv("KAIJU_GPU_DEVICE");
  if (!e) return 0;
  char *end = nullptr;
  const long v = strtol(e, &end, 10);
  if (end == e || (*end && *end != ',') || v < 0) die(std::string("KAIJU_GPU_DEVICES: not a list of device numbers: ") + e);
  return (int)v;
}

struct Slot {
  kaiju_gpu_tally *tally = nullptr;
  std::vector<char> in;
  uint64_t newlines = 0;
  kaiju_gpu_tally_info info{};
  std::future<int> done;
  std::string err;
};

// everything a tally holds, added to sum / totals
void collect(kaiju_gpu_tally *t, std::vector<kaiju_gpu_tally_entry> &room, std::map<uint64_t, kaiju_gpu_tally_entry> &sum, kaiju_gpu_tally_info &totals) {
  kaiju_gpu_tally_info tot{};
  uint64_t n = 0;
  int rc = kaiju_gpu_tally_result(t, room.data(), room.size(), &n, &tot);
  if (rc == KAIJU_GPU_ERR_ARG && n > room.size()) {
    room.resize(n);
    rc = kaiju_gpu_tally_result(t, room.data(), room.size(), &n, &tot);
  }
  if (rc != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
  for (uint64_t k = 0; k < n; k++) {
    kaiju_gpu_tally_entry &e = sum.emplace(room[k].taxon, kaiju_gpu_tally_entry{room[k].taxon, 0, 0, room[k].virus, 0}).first->second;
    e.direct += room[k].direct;
    e.summed += room[k].summed;
  }
  totals.used += tot.used; totals.n_lines += tot.n_lines; totals.n_total += tot.n_total; totals.n_unclassified += tot.n_unclassified;
  totals.n_bad_id += tot.n_bad_id; totals.n_unknown_taxon += tot.n_unknown_taxon; totals.n_virus += tot.n_virus;
}

}  // namespace

int main(int argc, char **argv) {
  std::string nodes, names_file, out_name, rank, ranks;
  float min_percent = 0.0f;
  int min_count = 0;
  bool verbose = false, expand = false, filter = false, full_path = false;
  opterr = 0;
  int c;
  while ((c = getopt(argc, argv, "hpveur:n:t:o:m:c:l:")) != -1) {
    switch (c) {
      case 'v': verbose = true; break;
      case 'e': expand = true; break;
      case 'u': filter = true; break;
      case 'p': full_path = true; break;
      case 'r': rank = optarg; break;
      case 'o': out_name = optarg; break;
      case 'n': names_file = optarg; break;
      case 't': nodes = optarg; break;
      case 'l': ranks = optarg; break;
      case 'c': {                      // (the tool says so and goes on with 0)
        char *end = nullptr;
        errno = 0;
        const long v = strtol(optarg, &end, 10);
        if (end == optarg || errno == ERANGE || v < INT32_MIN || v > INT32_MAX) fprintf(stderr, "Invalid number in -c %s\n", optarg);
        else min_count = (int)v;
        break;
      }
      case 'm': {
        char *end = nullptr;
        errno = 0;
        const float v = strtof(optarg, &end);
        if (end == optarg || errno == ERANGE) fprintf(stderr, "Invalid number in -m %s\n", optarg);
        else min_percent = v;
        break;
      }
      default: usage(argv[0]);         // -h too
    }
  }
  std::vector<std::string> inputs(argv + optind, argv + argc);
  auto refuse = [&](const char *why) { fprintf(stderr, "Error: %s\n", why); usage(argv[0]); };
  if (inputs.empty()) refuse("Please specify at least one input file.");
  if (names_file.empty()) refuse("Please specify the location of the names.dmp file with the -n option.");
  if (nodes.empty()) refuse("Please specify the location of the nodes.dmp file with the -t option.");
  if (out_name.empty()) refuse("Please specify the name of the output file with the -o option.");

  // the tool's remaining checks, before anything is opened
  {
    kjtr::Options o;
    o.rank = rank;
    o.has_list = !ranks.empty();
    o.list = kjtr::split_ranks(ranks);
    o.min_percent = min_percent;
    o.min_count = min_count;
    o.full_path = full_path;
    if (const char *why = kjtr::refusal(o)) refuse(why);
  }
  kaiju_table_options opt{};
  opt.rank = rank.c_str();
  opt.ranks_csv = ranks.empty() ? nullptr : ranks.c_str();
  opt.min_percent = min_percent;
  opt.min_count = min_count;
  opt.flags = (expand ? KAIJU_TABLE_EXPAND_VIRUSES : 0) | (filter ? KAIJU_TABLE_FILTER_UNCLASSIFIED : 0) | (full_path ? KAIJU_TABLE_FULL_PATH : 0);

  for (const std::string *p : {&nodes, &names_file}) {
    FILE *t = fopen(p->c_str(), "rb");
    if (!t) { fprintf(stderr, "Error: Could not open file %s\n", p->c_str()); usage(argv[0]); }
    fclose(t);
  }
  if (verbose) fprintf(stderr, "Reading the tree of %s and the names of %s\n", nodes.c_str(), names_file.c_str());
  kaiju_taxon_names *names = nullptr;
  if (kaiju_taxon_names_load(nodes.c_str(), names_file.c_str(), KAIJU_NAMES_NAME, nullptr, &names) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());

  if (verbose) fprintf(stderr, "Writing to file %s\n", out_name.c_str());
  FILE *out = fopen(out_name.c_str(), "w");
  if (!out) { fprintf(stderr, "Could not open file %s for writing\n", out_name.c_str()); return EXIT_FAILURE; }
  fputs("file\tpercent\treads\ttaxon_id\ttaxon_name\n", out);

  size_t block = (size_t)32 << 20;
  if (const char *e = getenv("KAIJU_TABLE_BLOCK")) {
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end == e || *end || v == 0) die(std::string("KAIJU_TABLE_BLOCK: not a number of bytes: ") + e);
    block = (size_t)v;
  }

  kaiju_gpu_taxon_names *dnames = nullptr;
  Slot slot[2];
  std::vector<kaiju_gpu_tally_entry> room(4096), list;
  std::vector<char> rows;
  for (const std::string &file : inputs) {
    FILE *in = fopen(file.c_str(), "rb");
    if (!in) { fprintf(stderr, "Could not open file %s\n", file.c_str()); fclose(out); return EXIT_FAILURE; }   // (what is written stays, as with the tool)
    if (!dnames) {                     // (the tool fails for a missing first file without having touched anything else)
      if (kaiju_gpu_taxon_names_upload(names, first_device(), &dnames) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
      for (Slot &s : slot)
        if (kaiju_gpu_tally_create(dnames, &s.tally) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
    }
    if (verbose) fprintf(stderr, "Processing %s...\n", file.c_str());
    kjab::BlockCutter cutter(in, block);
    auto drain = [&](Slot &s) {
      if (s.done.valid() && s.done.get() != KAIJU_GPU_OK) die(s.err);
    };
    for (uint64_t b = 0;; b++) {
      Slot &s = slot[b & 1];
      drain(s);                                              // (the block two back; the one before is still in flight)
      if (!cutter.next(s.in, &s.newlines)) break;
      // (a block ends behind a '\n' unless it is the file's last: every block is whole lines)
      s.done = std::async(std::launch::async, [&s]() {
        const int rc = kaiju_gpu_tally_add_text(s.tally, s.in.data(), s.in.size(), 1, &s.info);
        if (rc != KAIJU_GPU_OK) s.err = kaiju_gpu_last_error();
        return rc;
      });
    }
    for (Slot &s : slot) drain(s);
    if (ferror(in)) die("could not read " + file);
    fclose(in);

    std::map<uint64_t, kaiju_gpu_tally_entry> sum;
    kaiju_gpu_tally_info totals{};
    for (Slot &s : slot) {
      collect(s.tally, room, sum, totals);
      if (kaiju_gpu_tally_reset(s.tally) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
    }
    list.clear();
    for (const auto &p : sum) list.push_back(p.second);
    uint64_t n = 0;
    if (kaiju_table_rows(names, list.data(), list.size(), &totals, &opt, file.c_str(), nullptr, 0, &n) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
    rows.resize(n + 1);
    if (kaiju_table_rows(names, list.data(), list.size(), &totals, &opt, file.c_str(), rows.data(), n, &n) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
    if (n && fwrite(rows.data(), 1, n, out) != n) die("could not write to " + out_name);
    if (totals.n_bad_id) fprintf(stderr, "Error: %llu classified lines of %s have no readable taxon id.\n", (unsigned long long)totals.n_bad_id, file.c_str());
    if (totals.n_unknown_taxon)
      fprintf(stderr, "Warning: %llu lines of %s have a taxon id that is not contained in %s.\n", (unsigned long long)totals.n_unknown_taxon, file.c_str(), nodes.c_str());
  }
  if (fclose(out) != 0) die("could not write to " + out_name);

  for (Slot &s : slot) kaiju_gpu_tally_free(s.tally);
  kaiju_gpu_taxon_names_free(dnames);
  kaiju_taxon_names_free(names);
  return 0;
}
