// krona_san.cpp — the loader's names of parents that are no nodes (kaiju_amd/csrc/taxon_names.cpp) and the per-lane functions of
// kaiju_amd/csrc/kj_krona.h (through tests/emu/krona_emu.cpp) under the sanitizers, as a program of its own:
//   g++ -fsanitize=address,undefined -static-libasan -static-libubsan tests/tools/krona_san.cpp tests/emu/krona_emu.cpp kaiju_amd/csrc/taxon_names.cpp -o krona_san
//   krona_san NODES NAMES [NODES NAMES ...]
// Every pair is loaded in the three modes; per mode a line "dangling <mode> <child id> <name of its parent id>" for every node
// whose parent is no node but has a name.  Then, per list of ranks, the tables are built and read as the write pass reads them,
// and the text of "every node holds 3 reads" is written at several capacities; the whole text goes to stdout behind a line
// "text <pair> <list index> <bytes>".  At the end the first pair's names.dmp is cut at every prefix of its first bytes and at
// prefixes spread over the rest.  Exit 0: every call returned and every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#include "../../kaiju_amd/csrc/kj_format_names.h"
#include "../../kaiju_amd/csrc/taxon_names.h"

extern "C" void *krona_emu_create(const kaiju_taxon_names *names, const char *ranks_csv, int order, uint32_t seed);
extern "C" void krona_emu_free(void *h);
extern "C" int64_t krona_emu_check_tables(void *h);
extern "C" int krona_emu_text(void *h, const uint64_t *ids, const uint64_t *counts, uint32_t n_ids, uint64_t n_unclassified, int count_unclassified, uint8_t *out,
                              uint64_t out_cap, kaiju_gpu_krona_info *info, int order, uint32_t seed);

namespace {

const char *const kLists[] = {nullptr, "superkingdom,phylum,genus,species", "superkingdom,genus,,no rank", "tribe", "", ",,,"};
constexpr int kNLists = sizeof kLists / sizeof kLists[0];

// the tables and the text of one (tree, list); print: the pair's number, -1: nothing is printed
int exercise(const kaiju_taxon_names *t, int list, int print) {
  void *h = krona_emu_create(t, kLists[list], list % 3, 5);
  if (!h) return 1;
  int bad = krona_emu_check_tables(h) < 0;
  std::vector<uint64_t> ids, counts;
  for (uint64_t k : t->key) if (k != ~0ull) { ids.push_back(k); counts.push_back(3); }
  kaiju_gpu_krona_info info{}, again{};
  bad |= krona_emu_text(h, ids.data(), counts.data(), (uint32_t)ids.size(), 4, 1, nullptr, 0, &info, list % 3, 9) != 0;
  std::vector<uint8_t> out(info.text_bytes + 1, 0x33);
  for (uint64_t cap : {info.text_bytes, info.text_bytes / 2, info.text_bytes / 3 + 1}) {
    if (cap > info.text_bytes) continue;
    bad |= krona_emu_text(h, ids.data(), counts.data(), (uint32_t)ids.size(), 4, 1, out.data(), cap, &again, (list + 1) % 3, 9) != 0;
    bad |= again.text_bytes != info.text_bytes || again.written_bytes > cap || out[info.text_bytes] != 0x33;
    if (cap == info.text_bytes && print >= 0) {
      printf("text %d %d %llu\n", print, list, (unsigned long long)info.text_bytes);
      fwrite(out.data(), 1, info.text_bytes, stdout);
    }
  }
  krona_emu_free(h);
  return bad;
}

int pair(const char *nodes, const char *names, int print) {
  int bad = 0;
  const int modes[3] = {KAIJU_NAMES_NAME, KAIJU_NAMES_PATH, KAIJU_NAMES_RANKS};
  for (int m = 0; m < 3; m++) {
    kaiju_taxon_names *t = nullptr;
    if (kaiju_taxon_names_load(nodes, names, modes[m], m == 2 ? "genus,species" : nullptr, &t) != KAIJU_GPU_OK) return t ? 1 : 0;
    if (t->dang_len.size() != t->key.size() || t->dang_pos.size() != t->key.size()) bad = 1;
    for (size_t s = 0; s < t->key.size() && !bad; s++) {
      if (!t->dang_len[s]) continue;
      if (t->key[s] == ~0ull || t->parent[s] != kjn::kNone || (size_t)t->dang_pos[s] + t->dang_len[s] + 16 > t->dang_blob.size()) { bad = 1; break; }
      if (print >= 0) {
        printf("dangling %d %llu ", m, (unsigned long long)t->key[s]);
        fwrite(t->dang_blob.data() + t->dang_pos[s], 1, t->dang_len[s], stdout);
        printf("\n");
      }
    }
    if (m == 0)
      for (int l = 0; l < kNLists; l++) bad |= exercise(t, l, print);
    else bad |= exercise(t, m, -1);
    kaiju_taxon_names_free(t);
  }
  return bad;
}

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

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3 || (argc & 1) == 0) { fprintf(stderr, "usage: %s NODES NAMES [NODES NAMES ...]\n", argv[0]); return 2; }
  int bad = 0;
  for (int i = 1; i + 1 < argc; i += 2) bad |= pair(argv[i], argv[i + 1], i / 2);
  const char *tmp = getenv("TMPDIR");
  const std::string fm = std::string(tmp && *tmp ? tmp : "/tmp") + "/krona_san." + std::to_string((long)getpid()) + ".names";
  const std::vector<char> names = slurp(argv[2]);
  unsigned long cuts = 0;
  for (size_t n = 0; n <= names.size(); n += n < 300 || n + 120 > names.size() ? 1 : 97, cuts++) {
    FILE *f = fopen(fm.c_str(), "wb");
    if (!f) { perror(fm.c_str()); return 2; }
    if (n) fwrite(names.data(), 1, n, f);
    fclose(f);
    bad |= pair(argv[1], fm.c_str(), -1);
  }
  remove(fm.c_str());
  printf("krona_san: %lu cuts, %s\n", cuts, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
