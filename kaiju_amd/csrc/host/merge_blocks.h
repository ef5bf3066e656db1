// merge_blocks.h — the host side of kaiju-mergeOutputs (merge_main.cpp) that needs no GPU: the options of the tool and the
// reader that hands two files of lines out in pieces.  Plain C++ in a header of its own, so that a stand-alone program can
// drive it under the sanitizers (tests/tools/merge_blocks_san.cpp).
#ifndef KJ_MERGE_BLOCKS_H
#define KJ_MERGE_BLOCKS_H

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <cstddef>
#include <string>
#include <vector>

namespace kjmb {

// ---- the options of the tool: -i in1 -j in2 [-o out] [-c 1|2|lca|lowest] [-t nodes.dmp] [-s] [-v] [-d] --------------------
struct Options {
  std::string in1, in2, out, nodes, conflict = "lca";
  bool verbose = false, debug = false, use_score = false, help = false;
  int mode = 2;                        // KAIJU_GPU_MERGE_*: 0 "1", 1 "2", 2 "lca", 3 "lowest"
  std::string error;                   // not empty: what is wrong; the caller prints it and the usage
};

inline Options parse_options(int argc, char **argv) {
  Options o;
  optind = 1;
  opterr = 0;
  int c;
  while ((c = getopt(argc, argv, "hdvsc:n:t:i:j:o:")) != -1) {
    switch (c) {
      case 'h': o.help = true; return o;
      case 'v': o.verbose = true; break;
      case 'd': o.debug = true; break;
      case 's': o.use_score = true; break;
      case 'c': o.conflict = optarg; break;
      case 'o': o.out = optarg; break;
      case 't': o.nodes = optarg; break;
      case 'i': o.in1 = optarg; break;
      case 'j': o.in2 = optarg; break;
      case 'n': break;                 // (the tool takes it and never looks at it)
      default: o.error = std::string("unknown option or missing argument: -") + (char)optopt; return o;
    }
  }
  static const char *const kModes[] = {"1", "2", "lca", "lowest"};
  o.mode = -1;
  for (int k = 0; k < 4; k++) if (o.conflict == kModes[k]) o.mode = k;
  if (o.mode < 0) o.error = "Value of argument -c must be either 1, 2, lca, or lowest.";
  else if (o.mode == 2 && o.nodes.empty()) o.error = "LCA mode requires the name of the nodes.dmp file, using the -t option.";
  else if (o.in1.empty()) o.error = "Specify the name of the first input file, using the -i option.";
  else if (o.in2.empty()) o.error = "Specify the name of the second input file, using the -j option.";
  return o;
}

// ---- the reader ---------------------------------------------------------------------------------------------------------
// Hands two streams out piece by piece for kaiju_gpu_merge_text.  A side is topped up to `block` bytes in front of every piece -
// it is not given a block per round, or the side with the shorter lines, of which a round uses fewer bytes, would pile up - and
// what a call left unused (used()) stays at the front of the next piece.  A round that used nothing lets the side that holds
// no whole line grow by a block (a line longer than a block).  A piece is final when both streams are at their end; and when one stream is down to its
// last line (or to nothing) while the other goes on, the piece is that rest and the other side's next line alone, final: the
// one pair, or the finding that one file has more lines, without reading the longer file to its end.  The pieces' used parts
// behind each other are the streams.
struct Piece { const char *text1, *text2; size_t bytes1, bytes2; bool final; };

class PairReader {
  struct Side {
    FILE *f;
    std::vector<char> buf;
    size_t target;
    bool eof = false;
    void top_up() {
      while (!eof && buf.size() < target) {
        const size_t have = buf.size(), want = target - have;
        buf.resize(have + want);
        const size_t got = fread(buf.data() + have, 1, want, f);
        buf.resize(have + got);
        if (got < want) eof = true;
      }
    }
    // bytes up to and behind the first '\n'; 0: none
    size_t first_line() const { const void *nl = buf.empty() ? nullptr : memchr(buf.data(), '\n', buf.size()); return nl ? (size_t)(static_cast<const char *>(nl) - buf.data()) + 1 : 0; }
    void drop(size_t n) { buf.erase(buf.begin(), buf.begin() + (std::ptrdiff_t)(n < buf.size() ? n : buf.size())); }
  };
  Side s_[2];
  size_t block_;
  bool done_ = false, last_ = false, final_ = false;

 public:
  PairReader(FILE *f1, FILE *f2, size_t block_bytes) : block_(block_bytes ? block_bytes : 1) {
    s_[0].f = f1; s_[1].f = f2;
    s_[0].target = s_[1].target = block_;
  }
  // the next piece; false: both streams are used up (or stop() was called)
  bool next(Piece *p) {
    if (done_) return false;
    for (;;) {
      s_[0].top_up(); s_[1].top_up();
      const bool both = s_[0].eof && s_[1].eof;
      if (both && s_[0].buf.empty() && s_[1].buf.empty()) { done_ = true; return false; }
      size_t n[2] = {s_[0].buf.size(), s_[1].buf.size()};
      final_ = both;
      last_ = both;
      for (int k = 0; k < 2 && !both; k++) {
        Side &x = s_[k], &y = s_[1 - k];
        if (!x.eof || x.first_line()) continue;          // x is down to its last line, or to nothing; y goes on
        const size_t line = y.first_line();
        if (!line && !y.eof) { y.target = y.buf.size() + block_; n[0] = ~(size_t)0; break; }
        n[1 - k] = line ? line : y.buf.size();
        final_ = true;
        last_ = x.buf.empty();
        break;
      }
      if (n[0] == ~(size_t)0) continue;
      *p = Piece{s_[0].buf.data(), s_[1].buf.data(), n[0], n[1], final_};
      return true;
    }
  }
  // what the call on the piece used of either side
  void used(size_t used1, size_t used2) {
    s_[0].drop(used1); s_[1].drop(used2);
    if (last_) { done_ = true; return; }
    // a round that used nothing: the side without a whole line grows by a block
    const bool stuck = !used1 && !used2 && !final_, both = s_[0].first_line() && s_[1].first_line();
    for (Side &s : s_) s.target = stuck && (both || !s.first_line()) ? s.buf.size() + block_ : block_;
  }
  void stop() { done_ = true; }
};

}  // namespace kjmb

#endif  // KJ_MERGE_BLOCKS_H
