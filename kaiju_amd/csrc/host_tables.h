// host_tables.h — constant tables of the classification path, built on the host.
#pragma once
#include <string>
#include <vector>

#include "kj_core.h"

namespace kj {

// BLOSUM62 / substitution order / genetic code / nucleotide codes (ConsumerThread.cpp:6-187)
// and the mapping between the reference's aa2int order and the index alphabet.
// Returns 0 or a negative status (alphabet lacking one of the 20 amino acids).
int build_const_tables(const uint8_t trans[128], ConstTables &t, std::string &msg);

// SEG tables (blast_seg.c): ln(n!) table and the integer entropy classification, which is
// verified here against the reference's floating-point expression for all 77 partitions
// of the window.  lnfact_host receives the table the device copy is made from.  Also points st at the process-wide
// window-probability table (fails if two of its multisets share a key).
int build_seg_tables(std::vector<double> &lnfact_host, SegTables &st, std::string &msg);

// The window-probability table of s_Trim (kj_core.h: seg_prob_lookup): one entry per multiset of letter counts of a window of
// 1 .. kSegTabMax residues (the partitions of its length into at most 20 parts), the value computed by seg_prob_of_counts
// itself.  Built once per process by the first build_seg_tables and never changed; SegTables::ptab / ptab_T point into it.
struct SegProbTable {
  std::vector<SegProbEntry> slots;      // mask + 1 of them, key 0 = empty
  std::vector<uint64_t> reps;           // per slot: packed counts c0, c1 of the partition the entry was computed from
  std::vector<uint8_t> rep_len;         // per slot: its window length (0 = empty)
  uint64_t T[kSegKeyWords];
  uint32_t mask = 0, probe = 0, entries = 0;
  std::string error;                    // not empty: the build's self-check failed
};
const SegProbTable &seg_prob_table();

// tables of the fast stage 1 (kj_core.h: Stage1Tables) from the two above
void build_stage1_tables(const ConstTables &ct, const SegTables &st, Stage1Tables &t);

}  // namespace kj
