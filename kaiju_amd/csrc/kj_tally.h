// kj_tally.h — kaiju2table's reading of a text of output lines: the per-lane logic, for the device (tally.hip) and for the
// host (tests/emu/tally_emu.cpp drives the same functions pass by pass).  What the tool keeps in two std::map, this keeps
// per slot of the tree that kaiju_gpu_taxon_names_upload put on the device: direct[] while texts come in, summed[] at the end.
//
// The rules are those of kaiju2table.cpp:192-236 of the reference (getline, find('\t') twice, find_first_not_of of the
// digits, stoul, is_ancestor of 10239), observed on the unmodified tool:
//   lines     a line ends at '\n'; the last one may lack it; a line of length 0 counts nowhere.  Every other byte, '\r' and
//             NUL included, is a byte of the line
//   total     every line that is not empty
//   byte 0    not 'C': unclassified.  Only byte 0 is looked at ("c..." and "X" are unclassified)
//   id        t2 = the second tab of the line; the id is the run of [0-9] directly behind it, by value, whatever follows the
//             run ("22abc", "0022\r", "22\t..." of kaiju -v all read 22)
//   bad id    fewer than two tabs (the tool's substr throws), an empty run (" 22", "+22", "-3"), a value above 2^64 - 1: the
//             line counts in total and nowhere else
//   unknown   the id is no node of nodes.dmp: total, and nowhere else
//   else      direct[slot] += 1; and one more virus read when virus[slot]
// Per slot, once per tree:
//   virus     node 10239 is in the tree and the slot is 10239 or below it (is_ancestor, util.cpp:63-77: false for every node
//             when 10239 is none)
// At the end (:224-236):
//   summed    a slot with direct > 0 and virus set: summed[slot] = direct[slot], nothing goes to its ancestors.  Any other
//             slot adds direct to itself and to every ancestor; the walk stops in front of a node that is its own parent
//             and behind a node whose parent is no node.  (So reads of the root itself are in no sum.)  The loader refuses
//             cycles, so every walk ends
//
// Passes (every one works on independent units; the units of a pass may run in any order):
//   lines    that of kj_ingest.h as it is: line_start[0 .. n_lines], n_lines.  Without `final` only lines a '\n' ends
//   count    one lane per line: line_kind; the five counts, direct[].  A block of lanes sweeps its share of the lines
//            (count_blocks) and counts in a table of its own of kTableSlots slots - table_place: kTableProbes probes, a lane
//            that finds no room adds to direct[] for itself -, which it adds to direct[] at its end
//   sum      one lane per slot with direct > 0: sum_walk
//   compact  slots with summed > 0 to a dense list of kaiju_gpu_tally_entry, in ascending slot order (kj_scan.h)
//
// Sizes: a text is at most kji::kMaxBytes bytes per call; every count is 64 bit.
#ifndef KJ_TALLY_H
#define KJ_TALLY_H

#include "kj_annotate.h"

namespace kjt {

using kjn::kNone;

constexpr uint64_t kVirusTaxon = 10239;

// what a line is; the first five are also the indices of the scalar counts (kLineHit there: the virus reads)
enum { kLineEmpty = 0, kLineUnclassified = 1, kLineBadId = 2, kLineUnknown = 3, kLineHit = 4, kLineKinds = 5 };
enum { kCntTotal = 0, kCntUnclassified = 1, kCntBadId = 2, kCntUnknown = 3, kCntVirus = 4, kCounts = 5 };

// ---- lines --------------------------------------------------------------------------------------------------------
// lines to count of a text with n_nl '\n' bytes, the last of them in front of last_nl_end; *sentinel as in
// kji::line_count; *used: the bytes of those lines
KJF_HD uint32_t lines_counted(const uint8_t *text, uint64_t bytes, uint32_t n_nl, uint32_t last_nl_end, int final, uint32_t *sentinel, uint64_t *used) {
  if (final) { *used = bytes; return kji::line_count(text, bytes, n_nl, sentinel); }
  *sentinel = last_nl_end;
  *used = last_nl_end;
  return n_nl;
}

// ---- count --------------------------------------------------------------------------------------------------------
// the kind of the line text[a, a + len); *slot: its node (kLineHit only)
KJF_HD uint32_t line_kind(const uint8_t *text, uint64_t a, uint32_t len, const uint64_t *key, uint32_t cap_mask, uint32_t *slot) {
  *slot = kNone;
  if (len == 0) return kLineEmpty;
  if (text[a] != 'C') return kLineUnclassified;
  const uint64_t e = a + len, t2 = kja::second_tab(text, a, e);
  uint64_t id;
  if (t2 == e || !kja::parse_id(text, t2 + 1, e, &id)) return kLineBadId;
  *slot = kjn::find_slot(key, cap_mask, id);
  return *slot == kNone ? kLineUnknown : kLineHit;
}

// the table of a block: which slots of the tree it counts for, and how many lines each
constexpr uint32_t kTableSlots = 2048;
constexpr int kTableProbes = 4;
constexpr uint32_t kCountBlocks = 1024;      // at most
constexpr uint64_t kCountShare = 32768;      // bytes of text per block at least: a table is worth its flush
KJF_HD uint32_t count_blocks(uint64_t bytes) {
  const uint64_t b = bytes / kCountShare + 1;
  return b < kCountBlocks ? (uint32_t)b : kCountBlocks;
}
// where `slot` is counted in the table, kNone: nowhere (the lane adds for itself).  cas(i, slot): what table slot i held
// before "if it is free (kNone), it is slot's"
template <class Cas>
KJF_HD uint32_t table_place(uint32_t slot, Cas cas) {
  const uint32_t h = (slot * 0x9e3779b1u) >> 21;                    // 11 bits: kTableSlots
  for (int p = 0; p < kTableProbes; p++) {
    const uint32_t i = (h + (uint32_t)p) & (kTableSlots - 1);
    const uint32_t old = cas(i, slot);
    if (old == kNone || old == slot) return i;
  }
  return kNone;
}
static_assert(kTableSlots == 1u << 11, "table_place takes the top 11 bits of the hash");

// ---- per tree -----------------------------------------------------------------------------------------------------
// vslot: the slot of 10239 (kNone: no such node)
KJF_HD bool is_virus(const uint32_t *parent, uint32_t vslot, uint32_t s) {
  if (vslot == kNone) return false;
  for (uint32_t a = s; a != kNone; a = parent[a]) {
    if (a == vslot) return true;
    if (parent[a] == a) break;
  }
  return false;
}

// ---- sum ----------------------------------------------------------------------------------------------------------
// add(slot, d) for every slot that the d reads of slot s count for
template <class Add>
KJF_HD void sum_walk(const uint32_t *parent, const uint8_t *virus, uint32_t s, uint64_t d, Add add) {
  if (virus[s]) { add(s, d); return; }
  for (uint32_t a = s; a != kNone && parent[a] != a; a = parent[a]) add(a, d);
}

// ---- compact ------------------------------------------------------------------------------------------------------
KJF_HD kaiju_gpu_tally_entry make_entry(uint64_t taxon, uint64_t direct, uint64_t summed, uint32_t virus) {
  kaiju_gpu_tally_entry e;
  e.taxon = taxon; e.direct = direct; e.summed = summed; e.virus = virus; e.reserved = 0;
  return e;
}
KJF_HD kaiju_gpu_tally_info make_info(uint64_t used, uint64_t n_lines, const uint64_t *count) {
  kaiju_gpu_tally_info o;
  o.used = used; o.n_lines = n_lines;
  o.n_total = count[kCntTotal]; o.n_unclassified = count[kCntUnclassified]; o.n_bad_id = count[kCntBadId];
  o.n_unknown_taxon = count[kCntUnknown]; o.n_virus = count[kCntVirus];
  return o;
}

}  // namespace kjt

#endif  // KJ_TALLY_H
