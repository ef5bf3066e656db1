// annotate_main.cpp — kaiju-addTaxonNames: a drop-in for the reference's tool over the C-ABI (include/kaiju_gpu.h).
//
//   kaiju-addTaxonNames -t nodes.dmp -n names.dmp -i kaiju.out [-o out] [-u] [-p | -r rank,rank,...] [-v]
//
// The options, the failure statuses and every byte of the output (the -o file, or stdout) are the tool's; the wording of the
// messages on stderr is this program's own.  The file is read
// in blocks that end behind a '\n' (annotate_blocks.h); every block is annotated on the device (kaiju_gpu_annotate_text, the
// rules: csrc/kj_annotate.h) by one of two annotators - each with pinned staging buffers and a stream of its own, so that the
// upload of a block overlaps the passes of the one before - and the blocks are written in order.
//   device                 the first entry of KAIJU_GPU_DEVICES (or KAIJU_GPU_DEVICE), else 0
//   KAIJU_ANNOTATE_BLOCK   bytes per block (default 32 MiB; tests force small ones)
// One divergence, on stderr only: where the tool prints a message for every line it leaves unchanged, this prints one summary
// line per reason (bad taxon id, id not in the tree, id without a name) with the number of lines.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <future>
#include <string>
#include <vector>

#include "../../../include/kaiju_gpu.h"
#include "annotate_blocks.h"

namespace {

void usage(const char *prog) {
  fprintf(stderr,
          "usage: %s -t nodes.dmp -n names.dmp -i FILE [-o FILE] [-u] [-p | -r RANK,RANK,...] [-v]\n"
          "  -t FILE   nodes.dmp of the taxonomy           -n FILE   names.dmp of the taxonomy\n"
          "  -i FILE   output of kaiju to annotate         -o FILE   where to write (default: standard output)\n"
          "  -u        leave out lines of unclassified reads\n"
          "  -p        append the whole lineage instead of the taxon's name\n"
          "  -r LIST   append the names at these ranks, e.g. -r phylum,genus\n"
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
  kaiju_gpu_annotator *an = nullptr;
  std::vector<char> in, out;
  uint64_t newlines = 0;
  kaiju_gpu_annotate_info info{};
  std::future<int> done;
  std::string err;
};

}  // namespace

int main(int argc, char **argv) {
  const kjab::Options opt = kjab::parse_options(argc, argv);
  if (opt.help) usage(argv[0]);
  if (!opt.error.empty()) { fprintf(stderr, "Error: %s\n", opt.error.c_str()); usage(argv[0]); }

  const int mode = opt.full_path ? KAIJU_NAMES_PATH : !opt.ranks.empty() ? KAIJU_NAMES_RANKS : KAIJU_NAMES_NAME;
  for (const std::string *p : {&opt.nodes, &opt.names}) {
    FILE *t = fopen(p->c_str(), "rb");
    if (!t) { fprintf(stderr, "Error: cannot open %s\n", p->c_str()); usage(argv[0]); }
    fclose(t);
  }
  if (opt.verbose) fprintf(stderr, "Loading the tree of %s and the names of %s\n", opt.nodes.c_str(), opt.names.c_str());
  kaiju_taxon_names *names = nullptr;
  if (kaiju_taxon_names_load(opt.nodes.c_str(), opt.names.c_str(), mode, mode == KAIJU_NAMES_RANKS ? opt.ranks.c_str() : nullptr, &names) != KAIJU_GPU_OK)
    die(kaiju_gpu_last_error());

  FILE *in = fopen(opt.in.c_str(), "rb");
  if (!in) { fprintf(stderr, "Error: cannot open %s\n", opt.in.c_str()); return EXIT_FAILURE; }
  FILE *out = stdout;
  if (!opt.out.empty()) {
    if (opt.verbose) fprintf(stderr, "Writing to %s\n", opt.out.c_str());
    out = fopen(opt.out.c_str(), "wb");
    if (!out) { fprintf(stderr, "Error: cannot open %s for writing\n", opt.out.c_str()); return EXIT_FAILURE; }
  }

  kaiju_gpu_taxon_names *dnames = nullptr;
  if (kaiju_gpu_taxon_names_upload(names, first_device(), &dnames) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
  Slot slot[2];
  for (Slot &s : slot)
    if (kaiju_gpu_annotator_create(dnames, &s.an) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());

  size_t block = (size_t)32 << 20;
  if (const char *e = getenv("KAIJU_ANNOTATE_BLOCK")) {
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end == e || *end || v == 0) die(std::string("KAIJU_ANNOTATE_BLOCK: not a number of bytes: ") + e);
    block = (size_t)v;
  }
  if (opt.verbose) fprintf(stderr, "Annotating %s\n", opt.in.c_str());

  kjab::BlockCutter cutter(in, block);
  uint64_t bad = 0, unknown = 0, unnamed = 0;
  // wait for the block in flight on s and write its lines
  auto drain = [&](Slot &s) {
    if (!s.done.valid()) return;
    if (s.done.get() != KAIJU_GPU_OK) die(s.err);
    if (s.info.overflow) die("an annotated block is larger than its bound");
    if (s.info.text_bytes && fwrite(s.out.data(), 1, s.info.text_bytes, out) != s.info.text_bytes) die("could not write to " + (opt.out.empty() ? std::string("standard output") : opt.out));
    bad += s.info.n_bad_id; unknown += s.info.n_unknown_taxon; unnamed += s.info.n_unnamed_taxon;
  };
  const int drop = opt.drop_unclassified ? 1 : 0;
  for (uint64_t b = 0;; b++) {
    Slot &s = slot[b & 1];
    drain(s);                                              // (the block two back; the one before is still in flight)
    if (!cutter.next(s.in, &s.newlines)) break;
    s.out.resize(kaiju_gpu_annotate_bound(s.in.size(), s.newlines + 1, dnames));
    s.done = std::async(std::launch::async, [&s, drop]() {
      const int rc = kaiju_gpu_annotate_text(s.an, s.in.data(), s.in.size(), drop, s.out.data(), s.out.size(), &s.info);
      if (rc != KAIJU_GPU_OK) s.err = kaiju_gpu_last_error();
      return rc;
    });
  }
  // (the loop left at slot b & 1, already drained: the other one holds the last block)
  for (Slot &s : slot) drain(s);
  if (ferror(in)) die("could not read " + opt.in);
  fclose(in);
  if (fflush(out) != 0 || (out != stdout && fclose(out) != 0)) die("could not write to " + (opt.out.empty() ? std::string("standard output") : opt.out));

  if (bad) fprintf(stderr, "Warning: %llu classified lines without a readable taxon id were copied unchanged.\n", (unsigned long long)bad);
  if (unknown) fprintf(stderr, "Warning: %llu lines whose taxon id is no node of %s were copied unchanged.\n", (unsigned long long)unknown, opt.nodes.c_str());
  if (unnamed) fprintf(stderr, "Warning: %llu lines whose taxon id has no scientific name in %s were copied unchanged.\n", (unsigned long long)unnamed, opt.names.c_str());

  for (Slot &s : slot) kaiju_gpu_annotator_free(s.an);
  kaiju_gpu_taxon_names_free(dnames);
  kaiju_taxon_names_free(names);
  return 0;
}
