// gbk_main.cpp — kaiju-gbk2faa: a drop-in for the reference's util/kaiju-gbk2faa.pl over the C-ABI (include/kaiju_gpu.h).
//
//   kaiju-gbk2faa [-v] infile.gbff[.gz] outfile.faa
//
// The two arguments and every byte of the output file are the script's (the rules: csrc/kj_gbk.h).  The input - plain or
// gzip-compressed (pargz.h); bzip2, xz, zstd and the other formats the script's IO::Uncompress::AnyUncompress would open are
// refused by name - is read in blocks that end behind a '\n' and converted by ONE object, block behind block: what a line
// prints depends on the taxon, the protein id and the open translation of the lines in front of it, which the object carries
// on the device, so two objects on two streams would have nothing to work on in parallel.  What overlaps is the host's side:
// while the device converts a block, the next one is read and inflated, and the output of the one before is written.
//   device               the first entry of KAIJU_GPU_DEVICES (or KAIJU_GPU_DEVICE), else 0
//   KAIJU_GBK_BLOCK      bytes per block (default 16 MiB; tests force small ones).  A line that is larger is an error that
//                        names its size
// A /translation in front of which the file has no taxon ends the run as it ends the script: its message on stderr, an empty
// output file, status 255.  -v prints one summary line on stderr.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <future>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/kaiju_gpu.h"
#include "gbk_blocks.h"
#include "pargz.h"

namespace {

constexpr int kDied = 255;             // the status of perl's die

[[noreturn]] void die(const std::string &msg) { fprintf(stderr, "%s\n", msg.c_str()); exit(kDied); }

int first_device() {
  const char *e = getenv("KAIJU_GPU_DEVICES");
  if (!e || !strcmp(e, "all")) e = getenv("KAIJU_GPU_DEVICE");
  if (!e) return 0;
  char *end = nullptr;
  const long v = strtol(e, &end, 10);
  if (end == e || (*end && *end != ',') || v < 0) die(std::string("KAIJU_GPU_DEVICES: not a list of device numbers: ") + e);
  return (int)v;
}

// the input as a source of bytes
struct Input {
  FILE *f = nullptr;
  std::unique_ptr<pargz::Reader> pz;
  explicit Input(const std::string &name) {
    f = fopen(name.c_str(), "rb");
    if (!f) die("Opening input file failed: " + name + ": " + strerror(errno));
    unsigned char magic[8] = {0};
    const size_t got = fread(magic, 1, sizeof magic, f);
    const char *what = "";
    const kjgb::Format fmt = kjgb::sniff(magic, got, &what);
    if (fmt == kjgb::Format::kRefused) die("Opening input file failed: " + name + " is compressed with " + what + "; plain text and gzip are read");
    struct stat st;
    if (fmt == kjgb::Format::kGzip && fstat(fileno(f), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
      void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fileno(f), 0);     // (stays mapped until the program ends)
      if (m == MAP_FAILED) die("Opening input file failed: " + name);
      pz.reset(new pargz::Reader());
      unsigned threads = std::min(16u, std::max(2u, std::thread::hardware_concurrency() / 2));
      if (const char *e = getenv("KAIJU_GPU_GZ_THREADS")) threads = (unsigned)std::max(2, atoi(e));
      if (!pz->open(static_cast<const uint8_t *>(m), (size_t)st.st_size, threads, [name](const std::string &msg) { die(msg + " (" + name + ")"); }))
        die("Opening input file failed: " + name);
    } else {
      rewind(f);
    }
  }
  size_t read(char *dst, size_t n) { return pz ? pz->read(dst, n) : fread(dst, 1, n, f); }
  ~Input() { if (f) fclose(f); }
};

struct Slot {
  std::vector<char> in, out;
  kaiju_gpu_gbk_info info{};
  std::future<int> done;
  std::string err;
};

}  // namespace

int main(int argc, char **argv) {
  const kjgb::Options opt = kjgb::parse_options(argc, argv);
  if (!opt.error.empty()) die(opt.error + "\nUsage: " + argv[0] + " [-v] infile.gbk outfile.faa");
  if (opt.usage) die(std::string("Usage: ") + argv[0] + " [-v] infile.gbk outfile.faa");

  size_t block = (size_t)16 << 20;
  if (const char *e = getenv("KAIJU_GBK_BLOCK")) {
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end == e || *end || v == 0) die(std::string("KAIJU_GBK_BLOCK: not a number of bytes: ") + e);
    block = (size_t)v;
  }

  // the files in the order the script opens them
  FILE *out = fopen(opt.out.c_str(), "wb");
  if (!out) die("Could not open file " + opt.out + " for writing.");
  Input in(opt.in);

  kaiju_gpu_gbk *gbk = nullptr;
  if (kaiju_gpu_gbk_create(first_device(), &gbk) != KAIJU_GPU_OK) die(kaiju_gpu_last_error());

  kaiju_gpu_gbk_info sum{};
  uint64_t lines_before = 0;
  Slot slot[2];
  // wait for the block in flight on s, write what it gave
  auto drain = [&](Slot &s) {
    if (!s.done.valid()) return;
    if (s.done.get() != KAIJU_GPU_OK) die(s.err);
    if (s.info.no_taxon_line) {
      if (sum.written_bytes || ftruncate(fileno(out), 0) != 0) die("internal error: output in front of a translation without a taxon");
      fclose(out);
      fprintf(stderr, "No taxon id found in gbk file %s (line %llu)\n", opt.in.c_str(), (unsigned long long)(lines_before + s.info.no_taxon_line));
      exit(kDied);
    }
    if (s.info.written_bytes && fwrite(s.out.data(), 1, s.info.written_bytes, out) != s.info.written_bytes) die("could not write to " + opt.out);
    lines_before += s.info.n_lines;
    sum.written_bytes += s.info.written_bytes; sum.n_lines += s.info.n_lines; sum.n_records += s.info.n_records;
    sum.letters_kept += s.info.letters_kept; sum.letters_dropped += s.info.letters_dropped;
    for (int k = 0; k < 5; k++) sum.lines_kind[k] += s.info.lines_kind[k];
  };
  kjgb::Cutter cutter([&](char *dst, size_t n) { return in.read(dst, n); }, block, kjgb::Cutter::kLines);
  int rc = 0;
  for (uint64_t b = 0;; b++) {
    Slot &s = slot[b & 1], &prev = slot[(b & 1) ^ 1];
    if ((rc = cutter.next(s.in)) <= 0) break;                // (read and inflated while the block before is on the device)
    drain(prev);                                             // one call at a time: the state is carried from block to block
    s.out.resize(s.in.size() + 4096);
    s.done = std::async(std::launch::async, [&s, gbk]() {
      int r = kaiju_gpu_gbk_text(gbk, s.in.data(), s.in.size(), s.out.data(), s.out.size(), &s.info);
      if (r == KAIJU_GPU_OK && s.info.overflow) {            // (headers longer than their lines; the state did not advance: once more)
        s.out.resize(s.info.text_bytes);
        r = kaiju_gpu_gbk_text(gbk, s.in.data(), s.in.size(), s.out.data(), s.out.size(), &s.info);
      }
      if (r != KAIJU_GPU_OK) s.err = kaiju_gpu_last_error();
      return r;
    });
  }
  for (Slot &s : slot) drain(s);       // (at most one is in flight)
  if (rc < 0) die(cutter.error + " (" + opt.in + "; KAIJU_GBK_BLOCK sets the size of a block)");
  if (in.f && ferror(in.f)) die("could not read " + opt.in);
  if (fclose(out) != 0) die("could not write to " + opt.out);

  if (opt.verbose)
    fprintf(stderr, "%llu lines (%llu taxon, %llu protein id, %llu translations on one line, %llu over several), %llu records, %llu letters kept, %llu bytes dropped, %llu bytes written\n",
            (unsigned long long)sum.n_lines, (unsigned long long)sum.lines_kind[0], (unsigned long long)sum.lines_kind[1], (unsigned long long)sum.lines_kind[2],
            (unsigned long long)sum.lines_kind[3], (unsigned long long)sum.n_records, (unsigned long long)sum.letters_kept, (unsigned long long)sum.letters_dropped,
            (unsigned long long)sum.written_bytes);
  kaiju_gpu_gbk_free(gbk);
  return 0;
}
