// refseq_options_san.cpp — kaiju_amd/csrc/host/refseq_options.h under the sanitizers, as a program of its own:
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan tests/tools/refseq_options_san.cpp -o refseq_options_san
//   refseq_options_san ARGS...      the options kjrs::parse_options reads from ARGS, or "error: ..." / "usage"; status 1 then
// (the cutter and the readers the tool shares with kaiju-convertNR: tests/tools/convert_blocks_san.cpp)
#include <cstdio>

#include "../../kaiju_amd/csrc/host/refseq_options.h"

int main(int argc, char **argv) {
  const kjcb::Options o = kjrs::parse_options(argc, argv);
  if (o.help || o.bad_option) { printf("usage\n"); return 1; }
  if (!o.error.empty()) { printf("error: %s\n", o.error.c_str()); return 1; }
  printf("t=%s m=%s g=%s o=%s i=%s l=%s e=%s a=%d v=%d d=%d\n", o.nodes.c_str(), o.merged.c_str(), o.map.c_str(), o.out.c_str(), o.in.c_str(), o.list.c_str(),
         o.excluded.c_str(), o.add_acc, o.verbose, o.debug);
  return 0;
}
