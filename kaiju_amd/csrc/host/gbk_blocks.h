// gbk_blocks.h — the host side of kaiju-gbk2faa (gbk_main.cpp) that needs no GPU: the arguments of the script, the look at the
// first bytes of the input that tells gzip from plain text and from what is refused, and the cutter that makes blocks of a
// stream at line ends (that of convert_blocks.h).  Plain C++ in a header of its own, so that a stand-alone program can drive it
// under the sanitizers (tests/tools/gbk_blocks_san.cpp).
#ifndef KJ_GBK_BLOCKS_H
#define KJ_GBK_BLOCKS_H

#include <stdint.h>
#include <string.h>

#include <string>

#include "convert_blocks.h"

namespace kjgb {

using kjcb::Cutter;

// ---- the arguments of the script: infile.gbk outfile.faa; here also -v -----------------------------------------------------
struct Options {
  std::string in, out;
  bool verbose = false;
  bool usage = false;                  // fewer than two names: the script dies with its usage line
  std::string error;                   // not empty: an argument this program does not know
};

inline Options parse_options(int argc, char **argv) {
  Options o;
  int names = 0;
  bool only_names = false;
  for (int k = 1; k < argc; k++) {
    const char *a = argv[k];
    if (!only_names && !strcmp(a, "--")) { only_names = true; continue; }
    if (!only_names && !strcmp(a, "-v")) { o.verbose = true; continue; }
    if (!only_names && a[0] == '-' && a[1]) { o.error = std::string("unknown option ") + a; return o; }
    if (names == 0) o.in = a;
    else if (names == 1) o.out = a;
    names++;                                                 // (the script ignores further arguments)
  }
  o.usage = names < 2;
  return o;
}

// ---- the first bytes of the input ---------------------------------------------------------------------------------------
enum class Format { kPlain, kGzip, kRefused };
// what[0] is set for kRefused: the name of the compression
inline Format sniff(const unsigned char *b, size_t n, const char **what) {
  struct Magic { const char *name; size_t len; unsigned char bytes[6]; };
  static const Magic kRefusedMagic[] = {{"bzip2", 3, {'B', 'Z', 'h'}},       {"xz", 6, {0xfd, '7', 'z', 'X', 'Z', 0x00}}, {"zstd", 4, {0x28, 0xb5, 0x2f, 0xfd}},
                                        {"zip", 4, {'P', 'K', 0x03, 0x04}},  {"lzip", 4, {'L', 'Z', 'I', 'P'}},           {"lzop", 4, {0x89, 'L', 'Z', 'O'}},
                                        {"lzma", 4, {0x5d, 0x00, 0x00, 0x80}}, {"compress (.Z)", 2, {0x1f, 0x9d}}};
  *what = "";
  if (n >= 2 && b[0] == 0x1f && b[1] == 0x8b) return Format::kGzip;
  for (const Magic &m : kRefusedMagic)
    if (n >= m.len && !memcmp(b, m.bytes, m.len)) { *what = m.name; return Format::kRefused; }
  return Format::kPlain;
}

}  // namespace kjgb

#endif  // KJ_GBK_BLOCKS_H
