// krona_main.cpp — kaiju2krona: a drop-in for the reference's tool over the C-ABI (include/kaiju_gpu.h).
//
//   kaiju2krona -t nodes.dmp -n names.dmp -i kaiju.out -o kaiju.krona [-u] [-l rank,rank,...] [-v]
//
// The options, the failure statuses and the lines of the -o file are the tool's; the order of the lines - the tool's is
// that of a hash map and means nothing - and the wording of the messages on stderr are this program's own.  The input is
// read in blocks that end behind a '\n' (annotate_blocks.h) and every block is counted on the device
// (kaiju_gpu_tally_add_text, the rules: csrc/kj_tally.h) by one of two tallies - each with pinned staging and a stream of its
// own, so that the upload of a block overlaps the passes of the one before.  At the end kaiju_gpu_krona_text writes the
// lines from the counts of both where they lie (the rules: csrc/kj_krona.h): one call for the size, one for the text.
//   device               the first entry of KAIJU_GPU_DEVICES (or KAIJU_GPU_DEVICE), else 0
//   KAIJU_TABLE_BLOCK    bytes per block (default 32 MiB; tests force small ones)
// One divergence, on stderr only: where the tool prints a message for every line or taxon it leaves out, this prints one
// summary line per reason with the number of lines, taxa and reads.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <future>
#include <string>
#include <vector>

#include "../../../include/kaiju_gpu.h"
#include "annotate_blocks.h"

namespace {

void usage(const char *prog) {
  fprintf(stderr,
          "usage: %s -t nodes.dmp -n names.dmp -i FILE -o FILE [-u] [-l RANK,RANK,...] [-v]\n"
          "  -t FILE   nodes.dmp of the taxonomy           -n FILE   names.dmp of the taxonomy\n"
          "  -i FILE   output of kaiju                     -o FILE   where to write the text for Krona\n"
          "  -u        a last line with the number of unclassified reads\n"
          "  -l LIST   print only the names at these ranks, e.g. -l superkingdom,phylum,class,order,family,genus,species\n"
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
  uint64_t n_bad_id = 0, n_unknown = 0;
  std::future<int> done;
  std::string err;
};

}  // namespace

int main(int argc, char **argv) {
  std::string nodes, names_file, in_name, out_name, ranks;
  bool verbose = false, count_unclassified = false, has_list = false;
  opterr = 0;
  int c;
  while ((c = getopt(argc, argv, "huvn:t:i:o:l:")) != -1) {
    switch (c) {
      case 'v': verbose = true; break;
      case 'u': count_unclassified = true; break;
      case 'o': out_name = optarg; break;
      case 'n': names_file = optarg; break;
      case 't': nodes = optarg; break;
      case 'i': in_name = optarg; break;
      case 'l': has_list = true; ranks = optarg; break;
      default: usage(argv[0]);         // -h too
    }
  }
  auto refuse = [&](const char *why) { fprintf(stderr, "Error: %s\n", why); usage(argv[0]); };
  if (out_name.empty()) refuse("Please specify the name of the output file with the -o option.");
  if (names_file.empty()) refuse("Please specify the location of the names.dmp file with the -n option.");
  if (nodes.empty()) refuse("Please specify the location of the nodes.dmp file with the -t option.");
  if (in_name.empty()) refuse("Please specify the location of the input file with the -i option.");

  for (const std::string *p : {&nodes, &names_file}) {
    FILE *t = fopen(p->c_str(), "rb");
    if (!t) die("Could not open file " + *p);
    fclose(t);
  }
  if (verbose) fprintf(stderr, "Reading the tree of %s and the names of %s\n", nodes.c_str(), names_file.c_str());
  kaiju_taxon_names *names = nullptr;
  if (kaiju_taxon_names_load(nodes.c_str(), names_file.c_str(), KAIJU_NAMES_NAME, nullptr, &names) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());

  FILE *in = fopen(in_name.c_str(), "rb");
  if (!in) die("Could not open file " + in_name);
  // (the tool opens it at the end; here a file that cannot be written is said before the device is touched)
  FILE *out = fopen(out_name.c_str(), "w");
  if (!out) die("Could not open file " + out_name + " for writing");

  size_t block = (size_t)32 << 20;
  if (const char *e = getenv("KAIJU_TABLE_BLOCK")) {
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end == e || *end || v == 0) die(std::string("KAIJU_TABLE_BLOCK: not a number of bytes: ") + e);
    block = (size_t)v;
  }

  kaiju_gpu_taxon_names *dnames = nullptr;
  kaiju_gpu_krona *krona = nullptr;
  Slot slot[2];
  if (kaiju_gpu_taxon_names_upload(names, first_device(), &dnames) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
  // (the tool keeps a list whenever -l is given: an empty one prints no name at all)
  if (kaiju_gpu_krona_create(dnames, has_list ? ranks.c_str() : nullptr, &krona) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
  for (Slot &s : slot)
    if (kaiju_gpu_tally_create(dnames, &s.tally) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());

  if (verbose) fprintf(stderr, "Processing %s...\n", in_name.c_str());
  {
    kjab::BlockCutter cutter(in, block);
    auto drain = [&](Slot &s) {
      if (!s.done.valid()) return;
      if (s.done.get() != KAIJU_GPU_OK) die(s.err);
      s.n_bad_id += s.info.n_bad_id;
      s.n_unknown += s.info.n_unknown_taxon;
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
  }
  if (ferror(in)) die("could not read " + in_name);
  fclose(in);

  if (verbose) fprintf(stderr, "Writing to file %s\n", out_name.c_str());
  kaiju_gpu_tally *both[2] = {slot[0].tally, slot[1].tally};
  kaiju_gpu_krona_info info{};
  if (kaiju_gpu_krona_text(krona, both, 2, count_unclassified ? 1 : 0, nullptr, 0, &info) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
  std::vector<char> text(info.text_bytes + 1);
  if (kaiju_gpu_krona_text(krona, both, 2, count_unclassified ? 1 : 0, text.data(), info.text_bytes, &info) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
  if (info.overflow || info.written_bytes != info.text_bytes) die("the text changed between two calls");
  if (info.text_bytes && fwrite(text.data(), 1, info.text_bytes, out) != info.text_bytes) die("could not write to " + out_name);
  if (fclose(out) != 0) die("could not write to " + out_name);

  const uint64_t n_bad_id = slot[0].n_bad_id + slot[1].n_bad_id, n_unknown = slot[0].n_unknown + slot[1].n_unknown;
  if (n_bad_id) fprintf(stderr, "Found bad taxon id in %llu classified lines of %s.\n", (unsigned long long)n_bad_id, in_name.c_str());
  if (n_unknown)
    fprintf(stderr, "Warning: %llu lines of %s have a taxon id that is not contained in taxonomic tree file %s.\n", (unsigned long long)n_unknown, in_name.c_str(), nodes.c_str());
  if (info.n_unnamed_taxa)
    fprintf(stderr, "Warning: %llu taxon ids with %llu reads of %s are not contained in names.dmp file %s.\n", (unsigned long long)info.n_unnamed_taxa,
            (unsigned long long)info.n_unnamed_reads, in_name.c_str(), names_file.c_str());

  kaiju_gpu_krona_free(krona);
  for (Slot &s : slot) kaiju_gpu_tally_free(s.tally);
  kaiju_gpu_taxon_names_free(dnames);
  kaiju_taxon_names_free(names);
  return 0;
}
