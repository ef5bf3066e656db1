// convert_blocks_san.cpp — kaiju_amd/csrc/host/convert_blocks.h under the sanitizers, as a program of its own:
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan tests/tools/convert_blocks_san.cpp -o convert_blocks_san
//   convert_blocks_san cut lines|records FILE BLOCK_BYTES   the blocks of FILE, one line "<bytes>" each, behind one another on stdout
//                                                 framed as "<bytes>\n<the bytes>"; status 1 and "error: ..." where a block
//                                                 holds no cut.  The source hands the cutter FILE in reads of uneven size
//   convert_blocks_san pairs FILE                 "<old> <new>" per pair of read_pairs
//   convert_blocks_san list FILE                  one id of read_list per line
//   convert_blocks_san opts ARGS...               the options parse_options reads from ARGS, or "error: ..." / "usage"; status 1 then
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/host/convert_blocks.h"

static std::vector<char> slurp(const char *name) {
  std::vector<char> out;
  FILE *f = fopen(name, "rb");
  if (!f) exit(2);
  char buf[4096];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
  fclose(f);
  return out;
}

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "cut")) {
    const std::vector<char> text = slurp(argv[3]);
    size_t at = 0;
    kjcb::Cutter cutter([&](char *dst, size_t n) {
      const size_t k = n < text.size() - at ? n : text.size() - at;
      if (k) memcpy(dst, text.data() + at, k);
      at += k;
      return k;
    }, (size_t)strtoull(argv[4], nullptr, 10), !strcmp(argv[2], "lines") ? kjcb::Cutter::kLines : kjcb::Cutter::kRecords);
    std::vector<char> block;
    int rc;
    for (unsigned long long round = 0; (rc = cutter.next(block)) > 0; round++) {
      if (round > 10000000ull) return 3;               // the cutter does not come to an end
      printf("%zu\n", block.size());
      fwrite(block.data(), 1, block.size(), stdout);
    }
    if (rc < 0) { fflush(stdout); fprintf(stderr, "error: %s\n", cutter.error.c_str()); return 1; }
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "pairs")) {
    const std::vector<char> text = slurp(argv[2]);
    const std::vector<uint64_t> p = kjcb::read_pairs(text.data(), text.size());
    for (size_t k = 0; k + 1 < p.size(); k += 2) printf("%llu %llu\n", (unsigned long long)p[k], (unsigned long long)p[k + 1]);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "list")) {
    const std::vector<char> text = slurp(argv[2]);
    for (uint64_t id : kjcb::read_list(text.data(), text.size())) printf("%llu\n", (unsigned long long)id);
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "opts")) {
    const kjcb::Options o = kjcb::parse_options(argc - 1, argv + 1);
    if (o.help || o.bad_option) { printf("usage\n"); return 1; }
    if (!o.error.empty()) { printf("error: %s\n", o.error.c_str()); return 1; }
    printf("t=%s m=%s g=%s o=%s i=%s l=%s e=%s a=%d v=%d d=%d\n", o.nodes.c_str(), o.merged.c_str(), o.map.c_str(), o.out.c_str(), o.in.c_str(), o.list.c_str(),
           o.excluded.c_str(), o.add_acc, o.verbose, o.debug);
    return 0;
  }
  return 2;
}
