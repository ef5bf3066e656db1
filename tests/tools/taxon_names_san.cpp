// taxon_names_san.cpp — kaiju_amd/csrc/taxon_names.cpp under the sanitizers, as a program of its own:
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan tests/tools/taxon_names_san.cpp kaiju_amd/csrc/taxon_names.cpp -o taxon_names_san
//   taxon_names_san NODES NAMES [NODES NAMES ...]
// Every pair is loaded in the three modes and every annotation asked for twice (its length, then its bytes); then the loader
// is fed truncated and garbage files made from the first pair: every prefix length of the first 400 bytes, lines without their
// ends, NUL and high bytes, over-long numbers, a cycle.  Exit 0: every call returned (0 or an error status), nothing else.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#include "../../kaiju_amd/csrc/taxon_names.h"

namespace {

std::vector<char> slurp(const char *path) {
  std::vector<char> v;
  FILE *f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}
void spill(const std::string &path, const char *p, size_t n) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) { perror(path.c_str()); exit(2); }
  if (n) fwrite(p, 1, n, f);
  fclose(f);
}
unsigned long g_loaded = 0, g_refused = 0, g_annotations = 0;

// loads, asks for the annotation of every key and of some ids that are none, frees
int exercise(const char *nodes, const char *names, int mode, const char *ranks) {
  kaiju_taxon_names *t = nullptr;
  const int rc = kaiju_taxon_names_load(nodes, names, mode, ranks, &t);
  if (rc) { g_refused++; if (t) return 1; return 0; }
  g_loaded++;
  std::vector<uint64_t> ids(t->key.begin(), t->key.end());
  for (uint64_t extra : {0ull, 1ull, 2ull, 777777ull, ~0ull - 1}) ids.push_back(extra);
  std::vector<char> buf;
  for (uint64_t id : ids) {
    if (id == ~0ull) continue;
    const int64_t n = kaiju_taxon_names_annotation(t, id, nullptr, 0);
    if (n < 0) continue;
    buf.assign((size_t)n + 1, 0x5a);
    if (kaiju_taxon_names_annotation(t, id, buf.data(), (uint64_t)n) != n || buf[(size_t)n] != 0x5a) { kaiju_taxon_names_free(t); return 1; }
    // a buffer shorter than the text
    if (n > 1 && (kaiju_taxon_names_annotation(t, id, buf.data(), (uint64_t)n / 2) != n)) { kaiju_taxon_names_free(t); return 1; }
    g_annotations++;
  }
  kaiju_taxon_names_free(t);
  return 0;
}
int all_modes(const char *nodes, const char *names) {
  return exercise(nodes, names, KAIJU_NAMES_NAME, nullptr) | exercise(nodes, names, KAIJU_NAMES_PATH, nullptr) |
         exercise(nodes, names, KAIJU_NAMES_RANKS, "genus,species,,phylum,genus,no rank") | exercise(nodes, names, KAIJU_NAMES_RANKS, "") |
         exercise(nodes, names, KAIJU_NAMES_RANKS, nullptr) | exercise(nodes, names, KAIJU_NAMES_RANKS, ",,,");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3 || (argc & 1) == 0) { fprintf(stderr, "usage: %s NODES NAMES [NODES NAMES ...]\n", argv[0]); return 2; }
  int bad = 0;
  for (int i = 1; i + 1 < argc; i += 2) bad |= all_modes(argv[i], argv[i + 1]);
  const char *tmp = getenv("TMPDIR");
  const std::string dir = std::string(tmp && *tmp ? tmp : "/tmp") + "/taxon_names_san." + std::to_string((long)getpid());
  const std::string fn = dir + ".nodes", fm = dir + ".names";
  const std::vector<char> nodes = slurp(argv[1]), names = slurp(argv[2]);
  // every prefix of the first bytes, and prefixes spread over the rest: lines without their ends
  for (int which = 0; which < 2; which++) {
    const std::vector<char> &whole = which ? names : nodes;
    for (size_t n = 0; n <= whole.size(); n += n < 400 ? 1 : 997) {
      spill(which ? fm : fn, whole.data(), n);
      bad |= all_modes(which ? argv[1] : fn.c_str(), which ? fm.c_str() : argv[2]);
    }
  }
  // garbage
  static const char junk_nodes[] =
      "1\t|\t1\t|\tno rank\t|\n\n\n|||\n\t\t\n5\n5\t\n5\t|\t\n6\t|\t5\n6\t|\t5\t|\t\n7\t|\t5\t|\tRANK\t|\n8\t|\t5\t|\tx\n"
      "99999999999999999999\t|\t1\t|\tspecies\t|\n18446744073709551614\t|\t1\t|\tspecies\t|\n9\t|\t18446744073709551616\t|\tspecies\t|\n"
      "10\t|\t\0\t|\tspecies\t|\n\xff\xfe\n11 13 genus\r\n12\t|\t11\t|\tspecies";
  static const char junk_names[] =
      "scientific name\n1 scientific name\n|1|scientific name\n1\t|\t\t|\t|scientific name\n5\t|\tfive\t|\t\t|\tscientific name\t|\n"
      "x6y\t|\tsix|\tscientific name\n8\t|\t\0name\xff\t|\tscientific name\n99999999999999999999999\t|\tbig\t|\tscientific name\n"
      "11\t|\tscientific name\n12\t|\tlast without an end scientific name";
  spill(fn, junk_nodes, sizeof junk_nodes - 1);
  spill(fm, junk_names, sizeof junk_names - 1);
  bad |= all_modes(fn.c_str(), fm.c_str());
  bad |= all_modes(fn.c_str(), argv[2]) | all_modes(argv[1], fm.c_str());
  // a tree with a cycle, a list with too many ranks, files that are not there: refused, with a text
  static const char cycle[] = "1\t|\t1\t|\tno rank\t|\n20\t|\t21\t|\tgenus\t|\n21\t|\t22\t|\tgenus\t|\n22\t|\t20\t|\tgenus\t|\n23\t|\t22\t|\tspecies\t|\n";
  spill(fn, cycle, sizeof cycle - 1);
  kaiju_taxon_names *t = nullptr;
  if (kaiju_taxon_names_load(fn.c_str(), argv[2], KAIJU_NAMES_PATH, nullptr, &t) != KAIJU_GPU_ERR_ARG || t || !strstr(kaiju_taxon_names_last_error(), "cycle")) bad |= 1;
  if (kaiju_taxon_names_load(argv[1], argv[2], KAIJU_NAMES_RANKS, "a,b,c,d,e,f,g,h,i,j,k,l,m,n,o,p,q", &t) != KAIJU_GPU_ERR_ARG || t) bad |= 1;
  if (kaiju_taxon_names_load((fn + ".none").c_str(), argv[2], KAIJU_NAMES_NAME, nullptr, &t) != KAIJU_GPU_ERR_IO || t) bad |= 1;
  if (kaiju_taxon_names_load(argv[1], (fm + ".none").c_str(), KAIJU_NAMES_NAME, nullptr, &t) != KAIJU_GPU_ERR_IO || t) bad |= 1;
  if (kaiju_taxon_names_load(nullptr, nullptr, 0, nullptr, nullptr) != KAIJU_GPU_ERR_ARG) bad |= 1;
  remove(fn.c_str());
  remove(fm.c_str());
  printf("taxon_names_san: %lu loads, %lu refusals, %lu annotations, %s\n", g_loaded, g_refused, g_annotations, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
