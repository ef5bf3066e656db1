// merge_main.cpp — kaiju-mergeOutputs: a drop-in for the reference's tool over the C-ABI (include/kaiju_gpu.h).
//
//   kaiju-mergeOutputs -i in1.tsv -j in2.tsv [-o out.tsv] [-c 1|2|lca|lowest] [-t nodes.dmp] [-s] [-v] [-d]
//
// The options, the exit statuses, every byte of the output (the -o file, or stdout) and the summary of -v are the tool's; the
// wording of the other messages on stderr is this program's own, and -d is taken and prints nothing.  The two files are read
// in pieces (merge_blocks.h); every piece is merged on the device (kaiju_gpu_merge_text, the rules: csrc/kj_merge.h) and the
// pieces are written in order.  As the tool does, the program ends with status 0 after the first pair of lines that cannot be
// merged, with everything in front of it written.  One status is its own: 3 when a pair of scores lies outside what the device
// compares exactly (KAIJU_GPU_MERGE_STOP_SCORE_WIDE) - the output up to that pair is written, nothing is guessed.
//   device               the first entry of KAIJU_GPU_DEVICES (or KAIJU_GPU_DEVICE), else 0
//   KAIJU_MERGE_BLOCK    bytes per side and piece (default 32 MiB; tests force small ones)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../../include/kaiju_gpu.h"
#include "merge_blocks.h"

namespace {

void usage(const char *prog) {
  fprintf(stderr,
          "usage: %s -i in1.tsv -j in2.tsv [-o outfile.tsv] [-c 1|2|lca|lowest] [-s] [-t nodes.dmp] [-v] [-d]\n"
          "  -i FILE   first input file                    -j FILE   second input file\n"
          "  -o FILE   where to write (default: standard output)\n"
          "  -c MODE   which taxon wins when the files disagree: 1, 2, lca or lowest (default: lca)\n"
          "  -t FILE   nodes.dmp of the taxonomy (needed for -c lca, used by -c lowest)\n"
          "  -s        the fourth column is a score and the taxon with the better score wins\n"
          "  -v        print a summary at the end           -d        accepted, prints nothing\n"
          "Both input files must be sorted alike by the read name in the second column.\n",
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

const char *why_text(uint32_t why) {
  switch (why) {
    case KAIJU_GPU_MERGE_STOP_1_CLASS: case KAIJU_GPU_MERGE_STOP_2_CLASS: return "does not start with C or U";
    case KAIJU_GPU_MERGE_STOP_1_TABS: case KAIJU_GPU_MERGE_STOP_2_TABS: return "has fewer than three columns";
    case KAIJU_GPU_MERGE_STOP_1_COLUMN: case KAIJU_GPU_MERGE_STOP_2_COLUMN: return "has no taxon id or, with -s, no score column";
    default: return "";
  }
}

}  // namespace

int main(int argc, char **argv) {
  const kjmb::Options opt = kjmb::parse_options(argc, argv);
  if (opt.help) usage(argv[0]);
  if (!opt.error.empty()) { fprintf(stderr, "Error: %s\n", opt.error.c_str()); usage(argv[0]); }

  kaiju_taxonomy *tax = nullptr;
  if (!opt.nodes.empty()) {
    FILE *t = fopen(opt.nodes.c_str(), "rb");
    if (!t) { fprintf(stderr, "Error: Could not open file %s\n", opt.nodes.c_str()); usage(argv[0]); }
    fclose(t);
    if (kaiju_taxonomy_load(opt.nodes.c_str(), &tax) != KAIJU_GPU_OK) die("could not read " + opt.nodes);
  }
  FILE *out = stdout;
  if (!opt.out.empty()) {
    out = fopen(opt.out.c_str(), "wb");
    if (!out) { fprintf(stderr, "Could not open file %s for writing\n", opt.out.c_str()); return EXIT_FAILURE; }
  }
  FILE *in1 = fopen(opt.in1.c_str(), "rb");
  if (!in1) { fprintf(stderr, "Could not open file %s\n", opt.in1.c_str()); return EXIT_FAILURE; }
  FILE *in2 = fopen(opt.in2.c_str(), "rb");
  if (!in2) { fprintf(stderr, "Could not open file %s\n", opt.in2.c_str()); return EXIT_FAILURE; }

  const int device = first_device();
  kaiju_gpu_taxonomy *dtax = nullptr;
  if (tax && kaiju_gpu_taxonomy_upload(tax, device, &dtax) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
  kaiju_gpu_merger *merger = nullptr;
  if (kaiju_gpu_merger_create(dtax, device, opt.mode, opt.use_score ? 1 : 0, &merger) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());

  size_t block = (size_t)32 << 20;
  if (const char *e = getenv("KAIJU_MERGE_BLOCK")) {
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end == e || *end || v == 0) die(std::string("KAIJU_MERGE_BLOCK: not a number of bytes: ") + e);
    block = (size_t)v;
  }

  kjmb::PairReader reader(in1, in2, block);
  kjmb::Piece p;
  std::vector<char> text;
  uint64_t count = 0, c1 = 0, c2 = 0, c12 = 0, c3 = 0, c1not2 = 0, c2not1 = 0;
  int status = EXIT_SUCCESS;
  const std::string out_name = opt.out.empty() ? std::string("standard output") : opt.out;
  while (reader.next(&p)) {
    kaiju_gpu_merge_info info{};
    text.resize(kaiju_gpu_merge_bound(p.bytes1, p.bytes2));
    if (kaiju_gpu_merge_text(merger, p.text1, p.bytes1, p.text2, p.bytes2, p.final ? 1 : 0, text.data(), text.size(), &info) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
    if (info.overflow) die("a merged piece is larger than its bound");
    if (info.text_bytes && fwrite(text.data(), 1, info.text_bytes, out) != info.text_bytes) die("could not write to " + out_name);
    const uint64_t line = count + info.stop_pair + 1;                  // (of a pair that stopped)
    count += info.count; c1 += info.count_c1; c2 += info.count_c2; c12 += info.count_c12; c3 += info.count_c3;
    c1not2 += info.count_c1_not_c2; c2not1 += info.count_c2_not_c1;
    if (info.more_in_2) fprintf(stderr, "Warning: File %s has more lines than file %s\n", opt.in2.c_str(), opt.in1.c_str());
    if (info.stop_why != KAIJU_GPU_MERGE_STOP_NONE) {
      const unsigned long long n = (unsigned long long)line;
      if (info.stop_why == KAIJU_GPU_MERGE_STOP_2_SHORT) fprintf(stderr, "Error: File %s has more lines than file %s\n", opt.in1.c_str(), opt.in2.c_str());
      else if (info.stop_why == KAIJU_GPU_MERGE_STOP_NAMES) fprintf(stderr, "Error: Read names are not identical between the two input files on line %llu\n", n);
      else if (info.stop_why == KAIJU_GPU_MERGE_STOP_SCORE_WIDE) {
        fprintf(stderr, "Error: a score on line %llu has more than 15 significant digits or lies outside [1e-300, 1e300): the scores of this line cannot be compared exactly on the device.  The output ends in front of it.\n", n);
        status = 3;
      } else
        fprintf(stderr, "Error: Line %llu in file %s %s\n", n, (info.stop_why < KAIJU_GPU_MERGE_STOP_2_SHORT ? opt.in1 : opt.in2).c_str(), why_text(info.stop_why));
      reader.stop();
      break;
    }
    reader.used(info.used1, info.used2);
  }
  if (ferror(in1) || ferror(in2)) die("could not read " + (ferror(in1) ? opt.in1 : opt.in2));
  fclose(in1);
  fclose(in2);
  if (fflush(out) != 0 || (out != stdout && fclose(out) != 0)) die("could not write to " + out_name);

  if (opt.verbose) {
    const double n = (double)count;
    fprintf(stderr, "Number of all reads in input:\t%10llu\n", (unsigned long long)count);
    fprintf(stderr, "         classified in file1:\t%10llu  %6.2f%%\n", (unsigned long long)c1, ((double)c1 / n * 100.0));
    fprintf(stderr, "            but not in file2:\t%10llu  %6.2f%%\n", (unsigned long long)c1not2, ((double)c1not2 / n * 100.0));
    fprintf(stderr, "         classified in file2:\t%10llu  %6.2f%%\n", (unsigned long long)c2, ((double)c2 / n * 100.0));
    fprintf(stderr, "            but not in file1:\t%10llu  %6.2f%%\n", (unsigned long long)c2not1, ((double)c2not1 / n * 100.0));
    fprintf(stderr, "          classified in both:\t%10llu  %6.2f%%\n", (unsigned long long)c12, ((double)c12 / n * 100.0));
    fprintf(stderr, "         combined classified:\t%10llu  %6.2f%%\n", (unsigned long long)c3, ((double)c3 / n * 100.0));
  }

  kaiju_gpu_merger_free(merger);
  if (dtax) kaiju_gpu_taxonomy_free(dtax);
  if (tax) kaiju_taxonomy_free(tax);
  return status;
}
