// convert_main.cpp — kaiju-convertNR: a drop-in for the reference's tool over the C-ABI (include/kaiju_gpu.h).
//
//   kaiju-convertNR -t nodes.dmp -m merged.dmp -g prot.accession2taxid -o out.faa [-i nr] [-a] [-l list] [-e excluded] [-v] [-d]
//
// The options, the messages and statuses for missing options and files that cannot be opened, and every byte of the output
// file are the tool's (the rules: csrc/kj_convert.h).  The map file - gzip-compressed or not (pargz.h) - is read in blocks that
// end behind a '\n' and goes into the accession map on the device (kaiju_gpu_accmap_add_text); the nr text, from -i or from
// standard input, is cut in front of header lines (convert_blocks.h) and converted by one of two converters - each with a
// stream of its own, so that the upload of a block overlaps the passes of the one before - and the blocks are written in order.
//   device                 the first entry of KAIJU_GPU_DEVICES (or KAIJU_GPU_DEVICE), else 0
//   KAIJU_CONVERT_BLOCK    bytes per block of either file (default 16 MiB; tests force small ones).  A record (or a line of
//                          the map file) that is larger is an error that names its size
// Deliberately different (also in the usage text): the chatter of -v / -d on stderr is not reproduced, -v prints a summary; and
// on a taxonomy that is no single tree a record whose taxa have no common ancestor is dropped and counted where the tool hangs.
//
// Compiled with -DKAIJU_CONVERT_REFSEQ this is kaiju-convertRefSeq, the same program under the other rule set of kj_convert.h:
//   kaiju-convertRefSeq -t nodes.dmp -m merged.dmp -g prot.accession2taxid.FULL -o out.faa [-a] [-l list] [-v] [-d]   < text
// The tool reads standard input only and has no excluded accessions: -i, -e and -r end in the usage (refseq_options.h).  Map
// and converters are made with KAIJU_GPU_CONVERT_RULES_REFSEQ; files, blocks, streams and the order of the output are the same.
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>

#include <future>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/kaiju_gpu.h"
#include "convert_blocks.h"
#include "pargz.h"
#include "refseq_options.h"

namespace {

#ifdef KAIJU_CONVERT_REFSEQ
constexpr bool kRefSeq = true;
#else
constexpr bool kRefSeq = false;
#endif
constexpr int kRules = kRefSeq ? KAIJU_GPU_CONVERT_RULES_REFSEQ : KAIJU_GPU_CONVERT_RULES_NR;

void usage_refseq(const char *prog) {
  fprintf(stderr,
          "Usage:\n   %s -t nodes.dmp -m merged.dmp -g prot.accession2taxid -o out.faa   < protein FASTA\n"
          "Mandatory arguments:\n"
          "   -t FILENAME   Name of nodes.dmp file.\n"
          "   -m FILENAME   Name of merged.dmp file.\n"
          "   -g FILENAME   Name of prot.accession2taxid.FULL file (may be gzip-compressed).\n"
          "   -o FILENAME   Name of output file.\n"
          "Optional arguments:\n"
          "   -a            Prefix taxon ID with the accession number.\n"
          "   -l FILENAME   Name of file with taxon IDs. Only records having one of these IDs as ancestor in the taxonomy will be used.\n"
          "   -v            Print a summary. (The per-accession messages of the reference tool are not reproduced.)\n"
          "   -d            Accepted; the debug messages of the reference tool are not reproduced.\n"
          "The text is read from standard input.\n",
          prog);
  exit(EXIT_FAILURE);
}

void usage(const char *prog) {
  if (kRefSeq) usage_refseq(prog);
  fprintf(stderr,
          "Usage:\n   %s -t nodes.dmp -m merged.dmp -g prot.accession2taxid -o out.faa [-i nr]\n"
          "Mandatory arguments:\n"
          "   -t FILENAME   Name of nodes.dmp file.\n"
          "   -m FILENAME   Name of merged.dmp file.\n"
          "   -g FILENAME   Name of prot.accession2taxid file (may be gzip-compressed).\n"
          "   -o FILENAME   Name of output file.\n"
          "Optional arguments:\n"
          "   -a            Prefix taxon ID in database names with the first accession number per record.\n"
          "   -i FILENAME   Name of NR file. If this option is not used, then the program will read from STDIN.\n"
          "   -l FILENAME   Name of file with taxon IDs. Only records having one of these IDs as ancestor in the taxonomy will be used.\n"
          "   -e FILENAME   Name of file with accession numbers that will be excluded.\n"
          "   -v            Print a summary. (The per-accession messages of the reference tool are not reproduced.)\n"
          "On a taxonomy that is no single tree, records whose taxa have no common ancestor are dropped and counted.\n",
          prog);
  exit(EXIT_FAILURE);
}

// the tool's error(): the message and an empty line
void error(const std::string &msg) { fprintf(stderr, "Error: %s\n\n", msg.c_str()); }
[[noreturn]] void die(const std::string &msg) { error(msg); exit(EXIT_FAILURE); }
[[noreturn]] void cannot_open(const std::string &name) { die("Could not open file " + name); }

int first_device() {
  const char *e = getenv("KAIJU_GPU_DEVICES");
  if (!e || !strcmp(e, "all")) e = getenv("KAIJU_GPU_DEVICE");
  if (!e) return 0;
  char *end = nullptr;
  const long v = strtol(e, &end, 10);
  if (end == e || (*end && *end != ',') || v < 0) die(std::string("KAIJU_GPU_DEVICES: not a list of device numbers: ") + e);
  return (int)v;
}

std::vector<char> slurp(const std::string &name) {
  FILE *f = fopen(name.c_str(), "rb");
  if (!f) cannot_open(name);
  std::vector<char> out;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
  fclose(f);
  return out;
}

// a file that may be gzip-compressed, as a source of bytes
struct MaybeGz {
  FILE *f = nullptr;
  std::unique_ptr<pargz::Reader> pz;
  explicit MaybeGz(const std::string &name) {
    f = fopen(name.c_str(), "rb");
    if (!f) cannot_open(name);
    unsigned char magic[2] = {0, 0};
    const size_t got = fread(magic, 1, 2, f);
    struct stat st;
    if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b && fstat(fileno(f), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
      void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fileno(f), 0);     // (stays mapped until the program ends)
      if (m == MAP_FAILED) cannot_open(name);
      pz.reset(new pargz::Reader());
      unsigned threads = std::min(16u, std::max(2u, std::thread::hardware_concurrency() / 2));
      if (const char *e = getenv("KAIJU_GPU_GZ_THREADS")) threads = (unsigned)std::max(2, atoi(e));
      if (!pz->open(static_cast<const uint8_t *>(m), (size_t)st.st_size, threads, [name](const std::string &msg) { die(msg + " (" + name + ")"); })) cannot_open(name);
    } else {
      rewind(f);
    }
  }
  size_t read(char *dst, size_t n) { return pz ? pz->read(dst, n) : fread(dst, 1, n, f); }
  ~MaybeGz() { if (f) fclose(f); }
};

struct Slot {
  kaiju_gpu_converter *cv = nullptr;
  std::vector<char> in, out;
  kaiju_gpu_convert_info info{};
  std::future<int> done;
  std::string err;
};

}  // namespace

int main(int argc, char **argv) {
  const kjcb::Options opt = kRefSeq ? kjrs::parse_options(argc, argv) : kjcb::parse_options(argc, argv);
  if (opt.help || opt.bad_option) usage(argv[0]);
  if (!opt.error.empty()) { error(opt.error); usage(argv[0]); }

  size_t block = (size_t)16 << 20;
  if (const char *e = getenv("KAIJU_CONVERT_BLOCK")) {
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end == e || *end || v == 0) die(std::string("KAIJU_CONVERT_BLOCK: not a number of bytes: ") + e);
    block = (size_t)v;
  }

  // the files in the order the tool opens them
  { FILE *t = fopen(opt.nodes.c_str(), "rb"); if (!t) cannot_open(opt.nodes); fclose(t); }
  kaiju_taxonomy *tax = nullptr;
  if (kaiju_taxonomy_load(opt.nodes.c_str(), &tax) != KAIJU_GPU_OK) cannot_open(opt.nodes);
  const std::vector<char> merged_text = slurp(opt.merged);
  const std::vector<uint64_t> pairs = kjcb::read_pairs(merged_text.data(), merged_text.size());
  std::vector<uint64_t> include;
  if (!opt.list.empty()) {
    const std::vector<char> list_text = slurp(opt.list);
    include = kjcb::read_list(list_text.data(), list_text.size());
    if (include.empty()) include.push_back(~0ull);           // a list without an id keeps nothing: an id that is never a node
  } else {
    fprintf(stderr, "No taxa list specified, using Archaea, Bacteria, and Viruses.\n");
  }

  const int device = first_device();
  kaiju_gpu_taxonomy *dtax = nullptr;
  if (kaiju_gpu_taxonomy_upload(tax, device, &dtax) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
  kaiju_gpu_accmap *map = nullptr, *excluded = nullptr;
  if (kaiju_gpu_accmap_create_rules(dtax, device, pairs.data(), pairs.size() / 2, kRules, 0, &map) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
  {
    MaybeGz src(opt.map);
    kjcb::Cutter cutter([&](char *dst, size_t n) { return src.read(dst, n); }, block, kjcb::Cutter::kLines);
    std::vector<char> text;
    int rc;
    for (bool first = true; (rc = cutter.next(text)) > 0; first = false)
      if (kaiju_gpu_accmap_add_text(map, text.data(), text.size(), first ? 1 : 0) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
    if (rc < 0) die(cutter.error + " (" + opt.map + "; KAIJU_CONVERT_BLOCK sets the size of a block)");
  }
  if (!opt.excluded.empty()) {
    if (kaiju_gpu_accmap_create(nullptr, device, nullptr, 0, 1, 2, 0, &excluded) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
    MaybeGz src(opt.excluded);
    kjcb::Cutter cutter([&](char *dst, size_t n) { return src.read(dst, n); }, block, kjcb::Cutter::kLines);
    std::vector<char> text;
    int rc;
    while ((rc = cutter.next(text)) > 0)
      if (kaiju_gpu_accmap_add_keys(excluded, text.data(), text.size(), 1) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
    if (rc < 0) die(cutter.error + " (" + opt.excluded + ")");
  }

  FILE *in = stdin;
  if (!opt.in.empty()) {
    in = fopen(opt.in.c_str(), "rb");
    if (!in) cannot_open(opt.in);
  }
  FILE *out = fopen(opt.out.c_str(), "wb");
  if (!out) die("Could not open file " + opt.out + " for writing.");

  Slot slot[2];
  for (Slot &s : slot) {
    const uint64_t *ids = include.empty() ? nullptr : include.data();
    const int rc = kRefSeq ? kaiju_gpu_converter_create_rules(dtax, ids, (uint32_t)include.size(), map, kRules, opt.add_acc ? 1 : 0, &s.cv)
                           : kaiju_gpu_converter_create(dtax, ids, (uint32_t)include.size(), map, excluded, opt.add_acc ? 1 : 0, &s.cv);
    if (rc != KAIJU_GPU_OK) die(kaiju_gpu_last_error());
  }

  kaiju_gpu_convert_info sum{};
  uint64_t written = 0;
  // wait for the block in flight on s and write its records
  auto drain = [&](Slot &s) {
    if (!s.done.valid()) return;
    if (s.done.get() != KAIJU_GPU_OK) die(s.err);
    if (s.info.written_bytes && fwrite(s.out.data(), 1, s.info.written_bytes, out) != s.info.written_bytes) die("could not write to " + opt.out);
    written += s.info.written_bytes;
    sum.n_records += s.info.n_records; sum.n_kept += s.info.n_kept; sum.dropped_excluded += s.info.dropped_excluded; sum.dropped_no_taxon += s.info.dropped_no_taxon;
    sum.dropped_not_included += s.info.dropped_not_included; sum.dropped_no_lca += s.info.dropped_no_lca; sum.n_entries += s.info.n_entries; sum.n_hits += s.info.n_hits;
  };
  kjcb::Cutter cutter([&](char *dst, size_t n) { return fread(dst, 1, n, in); }, block, kjcb::Cutter::kRecords);
  int rc = 0;
  for (uint64_t b = 0;; b++) {
    Slot &s = slot[b & 1];
    drain(s);                                              // (the block two back; the one before is still in flight)
    if ((rc = cutter.next(s.in)) <= 0) break;
    s.out.resize(s.in.size() + s.in.size() / 4 + 4096);
    s.done = std::async(std::launch::async, [&s]() {
      int r = kaiju_gpu_convert_text(s.cv, s.in.data(), s.in.size(), s.out.data(), s.out.size(), &s.info);
      if (r == KAIJU_GPU_OK && s.info.overflow) {          // (the info holds the true size: once more with room for it)
        s.out.resize(s.info.text_bytes);
        r = kaiju_gpu_convert_text(s.cv, s.in.data(), s.in.size(), s.out.data(), s.out.size(), &s.info);
      }
      if (r != KAIJU_GPU_OK) s.err = kaiju_gpu_last_error();
      return r;
    });
  }
  for (Slot &s : slot) drain(s);
  if (rc < 0) die(cutter.error + " (KAIJU_CONVERT_BLOCK sets the size of a block)");
  if (ferror(in)) die("could not read " + (opt.in.empty() ? std::string("standard input") : opt.in));
  if (in != stdin) fclose(in);
  if (!written && fputc('\n', out) == EOF) die("could not write to " + opt.out);      // the endl of a file of which nothing is kept
  if (fclose(out) != 0) die("could not write to " + opt.out);

  if (opt.verbose || sum.dropped_no_lca) {
    fprintf(stderr, "%llu records, %llu kept; dropped: %llu excluded, %llu without a taxon, %llu outside the list of taxa", (unsigned long long)sum.n_records,
            (unsigned long long)sum.n_kept, (unsigned long long)sum.dropped_excluded, (unsigned long long)sum.dropped_no_taxon, (unsigned long long)sum.dropped_not_included);
    if (sum.dropped_no_lca) fprintf(stderr, ", %llu whose taxa have no common ancestor (the taxonomy is no single tree)", (unsigned long long)sum.dropped_no_lca);
    fprintf(stderr, "; %llu of %llu accessions have a taxon\n", (unsigned long long)sum.n_hits, (unsigned long long)sum.n_entries);
  }
  for (Slot &s : slot) kaiju_gpu_converter_free(s.cv);
  kaiju_gpu_accmap_free(excluded);
  kaiju_gpu_accmap_free(map);
  kaiju_gpu_taxonomy_free(dtax);
  kaiju_taxonomy_free(tax);
  return 0;
}
