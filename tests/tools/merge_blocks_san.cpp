// merge_blocks_san.cpp — kaiju_amd/csrc/host/merge_blocks.h under the sanitizers, as a program of its own:
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan tests/tools/merge_blocks_san.cpp -o merge_blocks_san
//   merge_blocks_san read FILE1 FILE2 BLOCK_BYTES OUT1 OUT2   drives the reader the way merge_main.cpp does, with a stand-in for the
//                                                   device call: a piece that is not final uses the lines a '\n' ends, as many
//                                                   of either side as the side with fewer has; a final one uses everything.
//                                                   What was used goes to OUT1 / OUT2; stdout: one line per piece,
//                                                   "<bytes1> <bytes2> <final> <used1> <used2>"
//   merge_blocks_san opts ARGS...                   the options parse_options reads from ARGS, or "error: ..."; status 1 on an error
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/host/merge_blocks.h"

// bytes of the first n lines of text[0, bytes) that a '\n' ends; *lines: how many there are when n is larger
static size_t lines_bytes(const char *text, size_t bytes, size_t n, size_t *lines) {
  size_t at = 0, k = 0;
  while (k < n) {
    const void *nl = at < bytes ? memchr(text + at, '\n', bytes - at) : nullptr;
    if (!nl) break;
    at = (size_t)(static_cast<const char *>(nl) - text) + 1;
    k++;
  }
  *lines = k;
  return at;
}

int main(int argc, char **argv) {
  if (argc >= 7 && !strcmp(argv[1], "read")) {
    FILE *f1 = fopen(argv[2], "rb"), *f2 = fopen(argv[3], "rb"), *o1 = fopen(argv[5], "wb"), *o2 = fopen(argv[6], "wb");
    if (!f1 || !f2 || !o1 || !o2) return 2;
    kjmb::PairReader reader(f1, f2, (size_t)strtoull(argv[4], nullptr, 10));
    kjmb::Piece p;
    for (unsigned long long round = 0; reader.next(&p); round++) {
      if (round > 10000000ull) return 3;               // the reader does not come to an end
      size_t n1, n2, u1 = p.bytes1, u2 = p.bytes2;
      if (!p.final) {
        lines_bytes(p.text1, p.bytes1, ~(size_t)0, &n1);
        lines_bytes(p.text2, p.bytes2, ~(size_t)0, &n2);
        const size_t n = n1 < n2 ? n1 : n2;
        u1 = lines_bytes(p.text1, p.bytes1, n, &n1);
        u2 = lines_bytes(p.text2, p.bytes2, n, &n2);
      }
      printf("%zu %zu %d %zu %zu\n", p.bytes1, p.bytes2, p.final ? 1 : 0, u1, u2);
      if (fwrite(p.text1, 1, u1, o1) != u1 || fwrite(p.text2, 1, u2, o2) != u2) return 2;
      reader.used(u1, u2);
    }
    if (reader.next(&p)) return 4;                     // the end stays the end
    fclose(f1);
    fclose(f2);
    return fclose(o1) == 0 && fclose(o2) == 0 ? 0 : 2;
  }
  if (argc >= 2 && !strcmp(argv[1], "opts")) {
    const kjmb::Options o = kjmb::parse_options(argc - 1, argv + 1);
    if (!o.error.empty()) { printf("error: %s\n", o.error.c_str()); return 1; }
    printf("i=%s j=%s o=%s t=%s c=%s mode=%d s=%d v=%d d=%d h=%d\n", o.in1.c_str(), o.in2.c_str(), o.out.c_str(), o.nodes.c_str(), o.conflict.c_str(), o.mode,
           o.use_score, o.verbose, o.debug, o.help);
    return 0;
  }
  return 2;
}
