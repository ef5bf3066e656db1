// annotate_blocks_san.cpp — kaiju_amd/csrc/host/annotate_blocks.h under the sanitizers, as a program of its own:
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan tests/tools/annotate_blocks_san.cpp -o annotate_blocks_san
//   annotate_blocks_san cut FILE BLOCK_BYTES OUT    the blocks of FILE behind each other to OUT; stdout: one line per block,
//                                                   "<bytes> <newlines> <1 if it ends in '\n'>"
//   annotate_blocks_san opts ARGS...                the options parse_options reads from ARGS, or "error: ..."; status 1 on an error
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/host/annotate_blocks.h"

int main(int argc, char **argv) {
  if (argc >= 5 && !strcmp(argv[1], "cut")) {
    FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[4], "wb");
    if (!f || !o) return 2;
    kjab::BlockCutter cutter(f, (size_t)strtoull(argv[3], nullptr, 10));
    std::vector<char> block;
    uint64_t nl;
    while (cutter.next(block, &nl)) {
      printf("%zu %llu %d\n", block.size(), (unsigned long long)nl, block.back() == '\n' ? 1 : 0);
      if (fwrite(block.data(), 1, block.size(), o) != block.size()) return 2;
    }
    if (cutter.next(block, &nl)) return 3;           // the end stays the end
    fclose(f);
    return fclose(o) == 0 ? 0 : 2;
  }
  if (argc >= 2 && !strcmp(argv[1], "opts")) {
    const kjab::Options o = kjab::parse_options(argc - 1, argv + 1);
    if (!o.error.empty()) { printf("error: %s\n", o.error.c_str()); return 1; }
    printf("t=%s n=%s i=%s o=%s r=%s v=%d u=%d p=%d h=%d\n", o.nodes.c_str(), o.names.c_str(), o.in.c_str(), o.out.c_str(), o.ranks.c_str(), o.verbose,
           o.drop_unclassified, o.full_path, o.help);
    return 0;
  }
  return 2;
}
