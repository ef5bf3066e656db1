// emu_history_main.cpp — the fill patterns of tests/test_call_history_emu.py under the sanitizers, as a program of its own
// (an arbitrary pattern turns a read of stale memory into a wild index: here that is a report, not a silent wrong record):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -w -pthread -fsanitize=address,undefined -fno-sanitize=alignment \
//       -fno-sanitize-recover=undefined tests/tools/emu_history_main.cpp tests/emu/kernel_emu.cpp kaiju_amd/csrc/host_index.cpp \
//       kaiju_amd/csrc/host_tables.cpp kaiju_amd/csrc/taxonomy.cpp -o emu_history_san
//   emu_history_san tests/golden/db.fmi tests/golden/reads.fq
// (-fno-sanitize=alignment: the lanes load 16 bytes from any address on purpose, kj_core.h: u128_unaligned; about a minute)
// The golden reads of up to 150 nt (the fast stage 1, lazy SEG), all of them (the general stage 1) and long reads joined from
// them (400 nt and more, every second one on the other strand), MEM and Greedy, SEG on and off: every working array of the
// emulation starts as a pattern (zeros, FF, A5, one residue code repeated, a slice of the database text), the hit records as the
// call's own records rotated by one read and as records with the internal flags and lazy-SEG notes set.  Every run must equal the
// run on zeroed memory: the whole records where the plan clears them, best / n_ids / flags / the announced ids where it does
// not.  Status 0 and "EMU_HISTORY_OK <runs>" on stdout, or 1 and the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kaiju_gpu.h"

extern "C" {
void *emu_index_load(const char *path, char *err, int errlen);
void emu_index_free(void *h);
const uint8_t *emu_text(void *h, uint64_t *n);
void emu_set_fill(const uint8_t *pattern, uint32_t len);
void emu_set_hits(const kaiju_gpu_hit *recs, uint32_t n);
int emu_last_clear_out();
int emu_classify(void *h, const kaiju_gpu_params *gp, const char *seqs, const uint64_t *off, uint32_t n, int paired, kaiju_gpu_hit *out,
                 uint32_t si_cap, uint32_t pool_cap, uint32_t match_cap, uint32_t *n_retry_out, char *frag_dump, uint64_t frag_dump_cap);
}

struct Batch {
  std::string name, seqs;
  std::vector<uint64_t> off;
  uint32_t n = 0;
  void add(const std::string &s) { off.resize(2 * (size_t)n + 3); off[2 * n] = seqs.size(); seqs += s; off[2 * n + 1] = off[2 * n + 2] = seqs.size(); n++; }
};

static std::string revcomp(const std::string &s) {
  std::string r(s.rbegin(), s.rend());
  for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
  return r;
}

static bool same(const std::vector<kaiju_gpu_hit> &a, const std::vector<kaiju_gpu_hit> &b, bool whole, uint32_t *at) {
  for (uint32_t r = 0; r < a.size(); r++) {
    *at = r;
    if (whole) { if (memcmp(&a[r], &b[r], sizeof a[r])) return false; continue; }
    if (a[r].best != b[r].best || a[r].n_ids != b[r].n_ids || a[r].flags != b[r].flags) return false;
    for (uint32_t k = 0; k < a[r].n_ids; k++) if (a[r].taxid[k] != b[r].taxid[k]) return false;
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s db.fmi reads.fq\n", argv[0]); return 2; }
  char err[512] = "";
  void *h = emu_index_load(argv[1], err, (int)sizeof err);
  if (!h) { fprintf(stderr, "%s\n", err); return 2; }
  std::vector<std::string> reads;
  {
    FILE *f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    char *line = nullptr; size_t cap = 0; long k = 0;
    while (getline(&line, &cap, f) > 0) {
      if (k++ % 4 != 1) continue;
      std::string s(line);
      while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
      reads.push_back(s);
    }
    free(line);
    fclose(f);
  }
  Batch shorts, all, longs;
  shorts.name = "short"; all.name = "all"; longs.name = "long";
  for (size_t i = 0; i < reads.size() && all.n < 400; i++) all.add(reads[i]);
  for (size_t i = 0; i < reads.size() && shorts.n < 300; i++) if (reads[i].size() <= 150) shorts.add(reads[i]);
  for (size_t i = 0; i + 8 < reads.size() && longs.n < 100; i += 5) {
    std::string s;
    for (size_t k = 0; k < 3 + i % 6; k++) s += reads[i + k];
    s.resize(s.size() - i % 3);                            // odd lengths
    longs.add(longs.n % 2 ? revcomp(s) : s);
  }
  std::vector<std::vector<uint8_t>> patterns = {{0x00}, {0xff}, {0xa5}, {0x01}, {0x0a}, {0x13}, {0x14}};
  uint64_t tn = 0;
  const uint8_t *text = emu_text(h, &tn);
  if (text && tn > 5000) patterns.emplace_back(text + 70, text + 70 + 4099);
  long runs = 0;
  for (const Batch *b : {&shorts, &all, &longs}) {
    for (int mode = 0; mode < 2; mode++) {
      for (int seg = 1; seg >= 0; seg--) {
        kaiju_gpu_params gp;
        memset(&gp, 0, sizeof gp);
        gp.mode = mode; gp.min_fragment_length = 11; gp.mismatches = 3; gp.min_score = 65; gp.seed_length = 7; gp.seg = seg;
        gp.use_evalue = mode; gp.min_evalue = 0.01; gp.max_matches_SI = 20; gp.max_match_ids = 20;
        std::vector<kaiju_gpu_hit> zero(b->n), got(b->n), rotated(b->n), poison(b->n);
        uint32_t nretry0 = 0;
        emu_set_fill(nullptr, 0);
        emu_set_hits(nullptr, 0);
        if (emu_classify(h, &gp, b->seqs.data(), b->off.data(), b->n, 0, zero.data(), 16, 192, 64, &nretry0, nullptr, 0)) { printf("classify failed\n"); return 1; }
        uint64_t x = 88172645463325252ull;
        for (uint32_t r = 0; r < b->n; r++) {
          rotated[r] = zero[(r + b->n - 1) % b->n];
          auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
          static const uint32_t fl[] = {0x40000000u, 0x20000000u, 0x60000000u, 1u, 3u, 0xffffffffu};
          static const uint32_t rs[] = {0xffffffffu, 0x80000001u, 0x80000007u, 1u, 2u, 900u};
          poison[r].best = 11 + (uint32_t)(rnd() % 289); poison[r].n_ids = (uint32_t)(rnd() % 22);
          poison[r].flags = fl[rnd() % 6]; poison[r].reserved = rs[rnd() % 6];
          for (auto &t : poison[r].taxid) t = rnd() >> 24;
        }
        for (size_t pi = 0; pi < patterns.size(); pi++) {
          for (int res = 0; res < 3; res++) {
            emu_set_fill(patterns[pi].data(), (uint32_t)patterns[pi].size());
            emu_set_hits(res == 0 ? nullptr : res == 1 ? rotated.data() : poison.data(), res == 0 ? 0 : b->n);
            uint32_t nretry = 0, at = 0;
            const int rc = emu_classify(h, &gp, b->seqs.data(), b->off.data(), b->n, 0, got.data(), 16, 192, 64, &nretry, nullptr, 0);
            runs++;
            if (rc || nretry != nretry0 || !same(zero, got, emu_last_clear_out() != 0, &at)) {
              printf("MISMATCH batch %s mode %d seg %d pattern %zu residue %d: rc %d, retries %u / %u, read %u\n", b->name.c_str(), mode, seg, pi, res, rc,
                     nretry, nretry0, at);
              return 1;
            }
          }
        }
      }
    }
  }
  emu_set_fill(nullptr, 0);
  emu_set_hits(nullptr, 0);
  emu_index_free(h);
  printf("EMU_HISTORY_OK %ld runs (%u short, %u golden, %u long reads; %zu patterns x 3 residues of hit records x 2 modes x SEG on/off)\n", runs,
         shorts.n, all.n, longs.n, patterns.size());
  return 0;
}
