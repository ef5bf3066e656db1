// stage1_team_emu.cpp — TEST INFRASTRUCTURE ONLY.
//
// The team stage 1 of kaiju_amd/csrc/kj_core.h (build_fragments_team: sixteen lanes per read, run here phase by phase
// through S1TeamHost) against the one-lane fast stage 1 it replaces (build_fragments_fast<false, kS1Units>), on the same
// batch: peptide areas, fragment lists, ReadMeta and error flags must be the same bytes.  Built and loaded by
// tests/test_stage1_team.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../kaiju_amd/csrc/host_index.h"
#include "../../kaiju_amd/csrc/host_tables.h"
#include "../../kaiju_amd/csrc/kj_core.h"
#include "../../kaiju_amd/csrc/fmi_stream.h"

using namespace kj;

struct S1Tables {
  ConstTables ct;
  SegTables st;
  std::vector<double> lnfact;
  Stage1Tables s1;
};

extern "C" {

void *s1t_load(const char *path, char *err, int errlen) {
  FmiFile file;
  PackedIndex packed;
  std::string msg;
  S1Tables *t = new S1Tables();
  int rc = file.load(path, msg);
  if (rc == 0) rc = packed.build(file.view(), msg);
  if (rc == 0) rc = build_const_tables(packed.trans, t->ct, msg);
  if (rc == 0) rc = build_seg_tables(t->lnfact, t->st, msg);
  if (rc != 0) { snprintf(err, (size_t)errlen, "%s", msg.c_str()); delete t; return nullptr; }
  build_stage1_tables(t->ct, t->st, t->s1);
  return t;
}
void s1t_free(void *h) { delete (S1Tables *)h; }

// the nucleotide code table: nuc3[c] for every byte (the tests check the letters the reference knows)
void s1t_nuc3(void *h, uint8_t *out) { memcpy(out, ((S1Tables *)h)->s1.nuc3, 256); }

// both stage 1 variants over the batch; returns the number of reads whose bytes differ, the first of them in *first_bad
// (-1: none), the error flags of the two runs in err[0] (one lane per read) and err[1] (teams), the fragments in nfrag[0] (all reads) and nfrag[1] (most of one read)
int s1t_compare(void *h, uint32_t mode, uint32_t m, uint32_t min_score, const uint8_t *seqs, const uint64_t *off, uint32_t n,
                int paired, int64_t *first_bad, uint32_t *err, uint64_t *nfrag) {
  const S1Tables &T = *(S1Tables *)h;
  Params p{};
  p.mode = (int32_t)mode; p.m = m; p.min_score = min_score; p.seg = 0;
  const size_t pep_n = (size_t)pep_base(off, n) + 512, frag_n = (size_t)frag_base(off, n, m) + 8;
  std::vector<uint8_t> pep[2] = {std::vector<uint8_t>(pep_n, 0xa5), std::vector<uint8_t>(pep_n, 0xa5)};
  std::vector<Frag> frags[2];
  std::vector<ReadMeta> meta[2];
  for (int v = 0; v < 2; v++) {
    frags[v].resize(frag_n);
    memset(frags[v].data(), 0x5a, frag_n * sizeof(Frag));
    meta[v].resize(n);
    memset(meta[v].data(), 0x3c, n * sizeof(ReadMeta));
  }
  uint32_t e[2] = {0, 0};
  uint32_t seg_count = 0;
  SegQueue sq{nullptr, nullptr, &seg_count, 0};
  for (int v = 0; v < 2; v++) {
    Batch b{};
    b.seqs = seqs; b.off = off; b.n_reads = n; b.paired = paired;
    b.pep = pep[v].data(); b.frags = frags[v].data(); b.meta = meta[v].data();
    if (v == 0) {
      uint32_t codes[2 * kS1ListCap];
      S1Lane ln{codes, 1, nullptr, nullptr};
      for (uint32_t r = 0; r < n; r++) {
        for (auto &x : codes) x = 0xdeadbeefu;
        build_fragments_fast<false>(T.s1, p, b, sq, r, &e[0], ln);
      }
    } else {
      S1TeamLds lds;
      S1TeamHost tm{&lds};
      for (uint32_t r = 0; r < n; r++) {
        memset(&lds, 0xee, sizeof lds);
        build_fragments_team(T.s1, p, b, r, &e[1], tm);
      }
    }
  }
  err[0] = e[0]; err[1] = e[1];
  int bad = 0;
  *first_bad = -1;
  uint64_t nf = 0, nmax = 0;
  for (uint32_t r = 0; r < n; r++) {
    const size_t p0 = (size_t)pep_base(off, r), p1 = r + 1 < n ? (size_t)pep_base(off, r + 1) : pep_n;
    const size_t f0 = (size_t)frag_base(off, r, m), f1 = r + 1 < n ? (size_t)frag_base(off, r + 1, m) : frag_n;
    const bool same = memcmp(pep[0].data() + p0, pep[1].data() + p0, p1 - p0) == 0 &&
                      memcmp(frags[0].data() + f0, frags[1].data() + f0, (f1 - f0) * sizeof(Frag)) == 0 &&
                      memcmp(&meta[0][r], &meta[1][r], sizeof(ReadMeta)) == 0;
    nf += meta[0][r].nfrag;
    if (meta[0][r].nfrag > nmax) nmax = meta[0][r].nfrag;
    if (!same) { if (*first_bad < 0) *first_bad = r; bad++; }
  }
  // (the bytes in front of the first area as well)
  if (memcmp(pep[0].data(), pep[1].data(), (size_t)pep_base(off, 0)) != 0 && *first_bad < 0) { *first_bad = 0; bad++; }
  nfrag[0] = nf; nfrag[1] = nmax;
  return bad;
}

}  // extern "C"
