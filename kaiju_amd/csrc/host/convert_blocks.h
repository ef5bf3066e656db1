// convert_blocks.h — the host side of kaiju-convertNR (convert_main.cpp) that needs no GPU: the options of the tool, the readers
// of merged.dmp and of the list of taxa, and the cutter that makes blocks of a stream - at line ends for the map file, in
// front of header lines for the nr text.  Plain C++ in a header of its own, so that a stand-alone program can drive it under
// the sanitizers (tests/tools/convert_blocks_san.cpp).
#ifndef KJ_CONVERT_BLOCKS_H
#define KJ_CONVERT_BLOCKS_H

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <cstddef>
#include <functional>
#include <string>
#include <utility>
#include <vector>

namespace kjcb {

// ---- the options of the tool: -t nodes.dmp -m merged.dmp -g map -o out [-i nr] [-a] [-l list] [-e excluded] [-v] [-d] --------
struct Options {
  std::string nodes, merged, map, out, in, list, excluded;
  bool verbose = false, debug = false, add_acc = false, help = false;
  bool bad_option = false;             // getopt's '?': the usage, without a message
  std::string error;                   // not empty: the tool's message for a missing option (then the usage)
};

inline Options parse_options(int argc, char **argv) {
  Options o;
  optind = 1;
  opterr = 0;
  int c;
  while ((c = getopt(argc, argv, "ahdvrm:l:g:t:i:o:e:")) != -1) {
    switch (c) {
      case 'h': o.help = true; return o;
      case 'd': o.debug = true; break;
      case 'v': o.verbose = true; break;
      case 'a': o.add_acc = true; break;
      case 'e': o.excluded = optarg; break;
      case 'l': o.list = optarg; break;
      case 'm': o.merged = optarg; break;
      case 't': o.nodes = optarg; break;
      case 'g': o.map = optarg; break;
      case 'i': o.in = optarg; break;
      case 'o': o.out = optarg; break;
      default: o.bad_option = true; return o;                // ('r' too: the tool's option string has it, its switch does not)
    }
  }
  // the order and the words of kaiju-convertNR.cpp:80-83
  if (o.nodes.empty()) o.error = "Please specify the location of the nodes.dmp file, using the -t option.";
  else if (o.merged.empty()) o.error = "Please specify the location of the merged.dmp file, using the -m option.";
  else if (o.map.empty()) o.error = "Please specify the location of the prot.accession2taxid file, using the -g option.";
  else if (o.out.empty()) o.error = "Please specify the name of the output file, using the -o option.";
  return o;
}

// ---- merged.dmp, the list of taxa ---------------------------------------------------------------------------------------
// the run of digits at text[p, e): its value into *v, false when it is empty or above 2^64 - 1 (stoul throws)
inline bool digits_value(const char *text, size_t p, size_t e, uint64_t *v) {
  uint64_t acc = 0;
  if (p >= e) return false;
  for (; p < e; p++) {
    const uint64_t d = (uint64_t)(text[p] - '0');
    if (acc > 1844674407370955161ull || (acc == 1844674407370955161ull && d > 5)) return false;
    acc = acc * 10 + d;
  }
  *v = acc;
  return true;
}
inline bool is_digit(char c) { return c >= '0' && c <= '9'; }

// calls line(begin, end) for every line of data[0, n) as getline sees them: a trailing '\n' opens no line
template <class F>
void for_lines(const char *data, size_t n, F line) {
  size_t a = 0;
  while (a < n) {
    const char *nl = static_cast<const char *>(memchr(data + a, '\n', n - a));
    const size_t e = nl ? (size_t)(nl - data) : n;
    line(a, e);
    a = e + 1;
  }
}

// parseMergedDmp (util.cpp:101-121): per non-empty line the run of digits at its start and the next run of digits behind a
// byte that is none; a line without either is skipped.  The pairs in file order (the map keeps the first of an old id)
inline std::vector<uint64_t> read_pairs(const char *data, size_t n) {
  std::vector<uint64_t> out;
  for_lines(data, n, [&](size_t a, size_t e) {
    size_t p = a;
    while (p < e && is_digit(data[p])) p++;
    uint64_t from, to;
    if (p == e || !digits_value(data, a, p, &from)) return;  // (no byte behind the first run: find_first_of(.., npos) finds nothing)
    size_t q = p;
    while (q < e && !is_digit(data[q])) q++;
    size_t r = q;
    while (r < e && is_digit(data[r])) r++;
    if (!digits_value(data, q, r, &to)) return;
    out.push_back(from);
    out.push_back(to);
  });
  return out;
}

// the -l file (kaiju-convertNR.cpp:115-141): per non-empty line the first run of digits.  Whether an id is a node is asked later
inline std::vector<uint64_t> read_list(const char *data, size_t n) {
  std::vector<uint64_t> out;
  for_lines(data, n, [&](size_t a, size_t e) {
    size_t q = a;
    while (q < e && !is_digit(data[q])) q++;
    size_t r = q;
    while (r < e && is_digit(data[r])) r++;
    uint64_t id;
    if (digits_value(data, q, r, &id)) out.push_back(id);
  });
  return out;
}

// ---- the cutter ---------------------------------------------------------------------------------------------------------
// Makes blocks of at most `block` bytes of a stream.  kLines: a block ends behind a '\n'.  kRecords: a block ends behind a
// '\n' that a '>' follows, so the next one starts at a header line.  What lies behind the cut is carried into the next block;
// the last block is what is left.  A block in which no cut is found is an error that names its size (a line or a record larger
// than a block), never a block cut somewhere else.  The blocks behind each other are the stream.
struct Cutter {
  enum Mode { kLines, kRecords };
  std::function<size_t(char *, size_t)> read;     // fills up to n bytes; less than n: the stream is at its end
  size_t block;
  Mode mode;
  std::vector<char> carry;
  bool eof = false;
  std::string error;
  Cutter(std::function<size_t(char *, size_t)> source, size_t block_bytes, Mode m) : read(std::move(source)), block(block_bytes < 2 ? 2 : block_bytes), mode(m) {}

  // where to cut out[0, n): the length of the block, 0 if there is no cut
  size_t cut_of(const char *out, size_t n) const {
    for (size_t e = n; e > 0;) {
      const void *nl = memrchr(out, '\n', e);
      if (!nl) return 0;
      const size_t p = (size_t)(static_cast<const char *>(nl) - out);
      if (mode == kLines) return p + 1;
      if (p + 1 < n && out[p + 1] == '>') return p + 1;      // (a '\n' as the last byte: what follows it is not known yet)
      e = p;
    }
    return 0;
  }

  // the next block into out (its old content is dropped).  1: a block, 0: the stream is at its end, -1: error
  int next(std::vector<char> &out) {
    if (!error.empty()) return -1;
    out.swap(carry);
    carry.clear();
    if (!eof && out.size() < block) {
      const size_t have = out.size(), want = block - have;
      out.resize(block);
      const size_t got = read(out.data() + have, want);
      out.resize(have + got);
      if (got < want) eof = true;
    }
    if (eof) return out.empty() ? 0 : 1;
    const size_t end = cut_of(out.data(), out.size());
    if (!end) {
      error = std::string(mode == kLines ? "a line" : "a record") + " of more than " + std::to_string(out.size()) + " bytes: larger than a block";
      return -1;
    }
    carry.assign(out.begin() + (std::ptrdiff_t)end, out.end());
    out.resize(end);
    return 1;
  }
};

}  // namespace kjcb

#endif  // KJ_CONVERT_BLOCKS_H
