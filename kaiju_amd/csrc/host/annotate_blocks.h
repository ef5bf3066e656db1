// annotate_blocks.h — the host side of kaiju-addTaxonNames (annotate_main.cpp) that needs no GPU: the options of the tool and
// the reader that cuts a file of lines into blocks.  Plain C++ in a header of its own, so that a stand-alone program can drive
// it under the sanitizers (tests/tools/annotate_blocks_san.cpp).
#ifndef KJ_ANNOTATE_BLOCKS_H
#define KJ_ANNOTATE_BLOCKS_H

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <cstddef>
#include <string>
#include <vector>

namespace kjab {

// ---- the options of the tool: -t nodes.dmp -n names.dmp -i in [-o out] [-u] [-p | -r LIST] [-v] --------------------------
struct Options {
  std::string nodes, names, in, out, ranks;
  bool verbose = false, drop_unclassified = false, full_path = false, help = false;
  std::string error;                   // not empty: what is wrong the caller prints it and the usage
};

inline Options parse_options(int argc, char **argv) {
  Options o;
  optind = 1;
  opterr = 0;
  int c;
  while ((c = getopt(argc, argv, "hvpur:n:t:i:o:")) != -1) {
    switch (c) {
      case 'h': o.help = true; return o;
      case 'v': o.verbose = true; break;
      case 'u': o.drop_unclassified = true; break;
      case 'p': o.full_path = true; break;
      case 'o': o.out = optarg; break;
      case 'n': o.names = optarg; break;
      case 't': o.nodes = optarg; break;
      case 'i': o.in = optarg; break;
      case 'r': o.ranks = optarg; break;
      default: o.error = std::string("unknown option or missing argument: -") + (char)optopt; return o;
    }
  }
  if (o.names.empty()) o.error = "no names.dmp given (-n)";
  else if (o.nodes.empty()) o.error = "no nodes.dmp given (-t)";
  else if (o.in.empty()) o.error = "no input file given (-i)";
  else if (!o.ranks.empty() && o.full_path) o.error = "-p and -r exclude each other";
  return o;
}

// ---- the reader ---------------------------------------------------------------------------------------------------------
// Cuts a stream into blocks of about `block` bytes that end behind a '\n': what lies behind the last '\n' read is carried into
// the next block, and a block grows by `block` bytes at a time while it holds no '\n' at all (a line longer than a block).
// The last block may end without '\n'.  The blocks behind each other are the stream.
struct BlockCutter {
  FILE *f;
  size_t block;
  std::vector<char> carry;
  bool eof = false;
  BlockCutter(FILE *file, size_t block_bytes) : f(file), block(block_bytes ? block_bytes : 1) {}

  // the next block into out (its old content is dropped), the '\n' in it into *newlines.  false: the stream is at its end
  bool next(std::vector<char> &out, uint64_t *newlines) {
    out.swap(carry);
    carry.clear();
    size_t searched = out.size();      // out[0, searched) holds no '\n' (the carry never does)
    for (;;) {
      if (!eof) {
        const size_t have = out.size(), want = have < block ? block - have : block;
        out.resize(have + want);
        const size_t got = fread(out.data() + have, 1, want, f);
        out.resize(have + got);
        if (got < want) eof = true;
      }
      if (eof) break;
      const void *nl = out.size() > searched ? memrchr(out.data() + searched, '\n', out.size() - searched) : nullptr;
      if (nl) {
        const size_t end = (size_t)(static_cast<const char *>(nl) - out.data()) + 1;
        carry.assign(out.begin() + (std::ptrdiff_t)end, out.end());
        out.resize(end);
        break;
      }
      searched = out.size();
    }
    uint64_t n = 0;
    for (const char *p = out.data(), *e = p + out.size(); p < e && (p = static_cast<const char *>(memchr(p, '\n', (size_t)(e - p)))); p++) n++;
    *newlines = n;
    return !out.empty();
  }
};

}  // namespace kjab

#endif  // KJ_ANNOTATE_BLOCKS_H
