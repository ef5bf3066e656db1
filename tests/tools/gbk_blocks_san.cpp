// gbk_blocks_san.cpp — kaiju_amd/csrc/host/gbk_blocks.h under the sanitizers, as a program of its own:
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan tests/tools/gbk_blocks_san.cpp -o gbk_blocks_san
//   gbk_blocks_san cut FILE BLOCK_BYTES   the blocks of FILE behind one another on stdout, framed as "<bytes>\n<the bytes>"; status 1
//                                         and "error: ..." where a block holds no line end
//   gbk_blocks_san sniff FILE             "plain", "gzip" or "refused <name>" by the first bytes of FILE
//   gbk_blocks_san opts ARGS...           what parse_options reads from ARGS, or "error: ..." / "usage"; status 1 then
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kaiju_amd/csrc/host/gbk_blocks.h"

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
  if (argc == 4 && !strcmp(argv[1], "cut")) {
    const std::vector<char> text = slurp(argv[2]);
    size_t at = 0;
    kjgb::Cutter cutter([&](char *dst, size_t n) {
      const size_t k = n < text.size() - at ? n : text.size() - at;      // (a short read is the end of the stream)
      if (k) memcpy(dst, text.data() + at, k);
      at += k;
      return k;
    }, (size_t)strtoull(argv[3], nullptr, 10), kjgb::Cutter::kLines);
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
  if (argc == 3 && !strcmp(argv[1], "sniff")) {
    const std::vector<char> text = slurp(argv[2]);
    const char *what = "";
    const kjgb::Format f = kjgb::sniff(reinterpret_cast<const unsigned char *>(text.data()), text.size() < 8 ? text.size() : 8, &what);
    if (f == kjgb::Format::kRefused) printf("refused %s\n", what);
    else printf("%s\n", f == kjgb::Format::kGzip ? "gzip" : "plain");
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "opts")) {
    const kjgb::Options o = kjgb::parse_options(argc - 1, argv + 1);
    if (!o.error.empty()) { printf("error: %s\n", o.error.c_str()); return 1; }
    if (o.usage) { printf("usage\n"); return 1; }
    printf("in=%s out=%s v=%d\n", o.in.c_str(), o.out.c_str(), o.verbose);
    return 0;
  }
  return 2;
}
