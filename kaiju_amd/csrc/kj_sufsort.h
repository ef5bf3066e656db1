// kj_sufsort.h - the suffix sort of the index builder by prefix doubling over ranks: the per-lane logic, for the device
// (sufsort.hip) and for the host (tests/emu/sufsort_emu.cpp drives the same functions through the whole round loop).
//
// Definition (the header comment of mkfmi.cpp): the text T[0, tlen) holds letter codes 1..20 and a terminator 0 behind every
// sequence.  The output is the nsuf = tlen - nseq positions p with T[p] != 0, ordered letter by letter; a terminator is
// smaller than every letter; two suffixes that reach their terminators together are ordered by position (they belong to
// different sequences, and file order is position order).
//
// Ranks.  rank[p] of a terminator is its sequence number 0 .. nseq-1: terminators are unique, in file order, below all
// letters (BWT rows 0 .. nseq-1).  rank[p] of a letter position is nseq + the number of letter suffixes in groups that sort
// before its group; a group is a run of suffixes that are equal as far as they have been compared.  A suffix alone in its
// group is FINAL: SA[rank[p] - nseq] = p, and its rank never changes again.  With the terminators unique the tie rule needs
// no comparator of its own: behind equal letters two different terminators decide by sequence number = by position.
//
// Round 1 (h = 0 -> KJ_SS_K): a key of KJ_SS_K = 12 symbols, five bits each, per letter suffix; what lies behind a terminator
// reads as 0.  A stable sort of (key, p) with the input in position order.  A suffix whose key contains its terminator is
// final even when its key equals a neighbour's - stability has put equal keys in position order - so group heads are "key
// differs from the predecessor, or key contains a terminator" (the last symbol of such a key is 0: ss_key_has_term).
// Round h -> 2h: only the suffixes that are not final are ACTIVE; they are kept as a list in rank order.  Sort the list by
// (rank[p] << 32 | rank[p + h]), flag the heads, write the new ranks, drop what became final.
//
// Two instantiations.  NARROW: positions, ranks and list indexes in 32 bits, texts below 0xf0000000 symbols (ss_tlen_ok).
// WIDE: all of them in 64 bits, tlen + rank_bias < 2^40 (ss_tlen_ok_wide).  The round key (rank[p], rank[p + h]) then has up to
// 80 bits and is a pair (SsKeyW), sorted in two stable passes: by rank[p + h], then by rank[p]; the scan item is a pair of
// 64-bit list indexes (SsScanItemW).  The wide functions are overloads of the narrow ones on those types, next to them below.
// rank_bias (wide only, 0 in the product): every rank is bias + what it is above, so that a text of a few thousand symbols
// carries ranks, round keys and rank comparisons beyond 2^32 through the real kernels; the scatter subtracts it again.
//
// INVARIANT of the load rank[p + h]: an active suffix never has its terminator within its first h symbols (h symbols have
// been compared, and a suffix whose compared part holds its terminator is final: in round 1 by the head rule, later because
// rank[p + h] is then the rank of a final suffix, which nobody shares).  So p + h lies inside p's own sequence, at most on its
// terminator, and below tlen.  ss_round_key guards the load anyway.
// Consequence: once h >= maxlen + 1 (longest sequence plus its terminator) nothing is active; the driver's loop is bounded by
// that and returns an internal error instead of spinning: rounds <= max(1, ceil(log2((maxlen + 1) / KJ_SS_K)) + 1).
#ifndef KJ_SUFSORT_H
#define KJ_SUFSORT_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KJ_SS_HD __host__ __device__ inline
#else
#define KJ_SS_HD inline
#endif

enum {
  KJ_SS_K = 12,                 // symbols in the key of round 1
  KJ_SS_SYM_BITS = 5,
  KJ_SS_KEY_BITS = KJ_SS_K * KJ_SS_SYM_BITS,
  KJ_SS_LANE_BYTES = 16,        // text bytes per lane of the key kernel (one aligned 16-byte load, and the next one for the look-ahead)
  KJ_SS_BLOCK = 256,
  KJ_SS_TILE = KJ_SS_BLOCK * KJ_SS_LANE_BYTES,   // text bytes per block of the key kernel
  KJ_SS_TEXT_PAD = 2 * KJ_SS_LANE_BYTES,         // zero bytes the key kernel may read behind the text rounded up to 16
  KJ_SS_STATS_ROUNDS = 16
};

// the narrow instantiation: the host builder's own boundary for its 32-bit instantiation
KJ_SS_HD bool ss_tlen_ok(uint64_t tlen) { return tlen < 0xf0000000ull; }
// the wide one: every rank, bias included, below 2^40 (room for 5-byte storage, which is not used today)
KJ_SS_HD bool ss_tlen_ok_wide(uint64_t tlen_plus_bias) { return tlen_plus_bias < (1ull << 40); }

// text bytes on the device: rounded up to a lane's load, plus the look-ahead
KJ_SS_HD uint64_t ss_text_alloc(uint64_t tlen) { return ((tlen + KJ_SS_LANE_BYTES - 1) / KJ_SS_LANE_BYTES) * KJ_SS_LANE_BYTES + KJ_SS_TEXT_PAD; }

// device memory of one sort without the radix sort's and the scans' own temporary storage (which the driver adds): text,
// ranks (4), double-buffered keys (2 x 8) and values (2 x 4), the active list (4), block counts of the key kernel
KJ_SS_HD uint64_t ss_scratch_bytes(uint64_t tlen, uint64_t nsuf) {
  const uint64_t n = nsuf ? nsuf : 1, ntiles = (tlen + KJ_SS_TILE - 1) / KJ_SS_TILE + 1;
  return ss_text_alloc(tlen) + 4 * (tlen + 1) + 16 * n + 8 * n + 4 * n + 4 * ntiles + 6 * 256;
}

// the wide instantiation: text, ranks (8), five arrays of 8 bytes per suffix in one slab - keys x 2, positions x 2, the active
// list; the scan items of 16 bytes lie over a free key buffer and the active list, KJ_SS_WIDE_ALIGN keeps the five apart - and
// 64-bit tile counts and bases.  49 bytes per symbol and the radix sort's and the scans' temporary storage.
enum { KJ_SS_WIDE_ALIGN = 256 };
KJ_SS_HD uint64_t ss_wide_stride(uint64_t nsuf) { return ((8 * (nsuf ? nsuf : 1) + KJ_SS_WIDE_ALIGN - 1) / KJ_SS_WIDE_ALIGN) * KJ_SS_WIDE_ALIGN; }
KJ_SS_HD uint64_t ss_scratch_bytes_wide(uint64_t tlen, uint64_t nsuf) {
  const uint64_t ntiles = (tlen + KJ_SS_TILE - 1) / KJ_SS_TILE + 1;
  return ss_text_alloc(tlen) + 8 * (tlen + 1) + 5 * ss_wide_stride(nsuf) + 16 * ntiles + 6 * 256;
}

// the largest h a round may be asked to run with: beyond it an active suffix is an internal error
KJ_SS_HD bool ss_round_allowed(uint64_t h, uint64_t maxlen) { return h < maxlen + 1; }

// ---- round 1: keys ----------------------------------------------------------------------------------------------------
// the key of position j from the key of position j + 1 and the symbol at j: what lies behind a terminator reads as 0, so the
// key of a terminator position is 0 and a key never carries symbols of the next sequence
KJ_SS_HD uint64_t ss_roll(uint64_t key_next, uint32_t sym) {
  return sym ? ((uint64_t)sym << (KJ_SS_KEY_BITS - KJ_SS_SYM_BITS)) | (key_next >> KJ_SS_SYM_BITS) : 0ull;
}
KJ_SS_HD uint32_t ss_byte(const uint64_t w[4], int j) { return (uint32_t)(w[j >> 3] >> ((j & 7) * 8)) & 0xffu; }

// one lane: w = 32 text bytes (little endian; the lane's 16 and the 16 behind them), keys[j] = key of the lane's byte j.
// Returns the mask of the bytes that are letters (a suffix each).  Bytes 16 .. 26 are the look-ahead of byte 15.
KJ_SS_HD uint32_t ss_lane_keys(const uint64_t w[4], uint64_t keys[KJ_SS_LANE_BYTES]) {
  uint64_t k = 0;
#pragma unroll
  for (int j = KJ_SS_LANE_BYTES + KJ_SS_K - 2; j >= KJ_SS_LANE_BYTES; j--) k = ss_roll(k, ss_byte(w, j));
  uint32_t letters = 0;
#pragma unroll
  for (int j = KJ_SS_LANE_BYTES - 1; j >= 0; j--) {
    const uint32_t s = ss_byte(w, j);
    k = ss_roll(k, s);
    keys[j] = k;
    letters |= (s ? 1u : 0u) << j;
  }
  return letters;
}
KJ_SS_HD uint32_t ss_lane_letters(uint64_t w0, uint64_t w1) {      // number of letters among a lane's 16 bytes
  // a symbol has five bits: all of them or-ed down to bit 0 of its byte say "not a terminator"
  uint64_t a = w0 | (w0 >> 1) | (w0 >> 2), b = w1 | (w1 >> 1) | (w1 >> 2);      // bit 0: bits 0..2, bit 2: bits 2..4
  a = (a | (a >> 2)) & 0x0101010101010101ull;
  b = (b | (b >> 2)) & 0x0101010101010101ull;
  return (uint32_t)((a * 0x0101010101010101ull) >> 56) + (uint32_t)((b * 0x0101010101010101ull) >> 56);
}
KJ_SS_HD bool ss_key_has_term(uint64_t key) { return (key & ((1u << KJ_SS_SYM_BITS) - 1)) == 0; }

// ---- heads, ranks, what stays active -------------------------------------------------------------------------------------
// round 1: entry i of the sorted (key, p) starts a group
KJ_SS_HD bool ss_head_first(uint64_t i, uint64_t key_prev, uint64_t key) { return i == 0 || key != key_prev || ss_key_has_term(key); }
// round h: the key of an active suffix
KJ_SS_HD uint64_t ss_round_key(const uint32_t *rank, uint32_t p, uint64_t h, uint64_t tlen) {
  const uint64_t q = (uint64_t)p + h;
  const uint32_t r2 = q < tlen ? rank[q] : 0u;        // (never out of range: the invariant above)
  return ((uint64_t)rank[p] << 32) | r2;
}
// ... wide: a pair; the sort takes lo first and hi second, both stable
struct SsKeyW { uint64_t hi, lo; };                   // rank[p], rank[p + h]
KJ_SS_HD uint64_t ss_rank_ahead(const uint64_t *rank, uint64_t p, uint64_t h, uint64_t tlen) {
  const uint64_t q = p + h;
  return q < tlen ? rank[q] : 0ull;                   // (never out of range: the invariant above)
}
KJ_SS_HD SsKeyW ss_round_key(const uint64_t *rank, uint64_t p, uint64_t h, uint64_t tlen) {
  const SsKeyW k = {rank[p], ss_rank_ahead(rank, p, h, tlen)};
  return k;
}
// round h: entry i of the sorted list starts a group of the old order / of the new one
KJ_SS_HD bool ss_head_old(uint64_t i, uint64_t key_prev, uint64_t key) { return i == 0 || (key >> 32) != (key_prev >> 32); }
KJ_SS_HD bool ss_head_new(uint64_t i, uint64_t key_prev, uint64_t key) { return i == 0 || key != key_prev; }
KJ_SS_HD bool ss_head_old(uint64_t i, SsKeyW key_prev, SsKeyW key) { return i == 0 || key.hi != key_prev.hi; }
KJ_SS_HD bool ss_head_new(uint64_t i, SsKeyW key_prev, SsKeyW key) { return i == 0 || key.hi != key_prev.hi || key.lo != key_prev.lo; }
// what the inclusive scan runs over: (index of the last old head) << 32 | index of the last new head, both maxima
KJ_SS_HD uint64_t ss_scan_item(uint32_t i, bool head_old, bool head_new) { return ((uint64_t)(head_old ? i : 0u) << 32) | (head_new ? i : 0u); }
struct SsScanMax {
  KJ_SS_HD uint64_t operator()(uint64_t a, uint64_t b) const {
    const uint64_t ah = a >> 32, bh = b >> 32, al = a & 0xffffffffull, bl = b & 0xffffffffull;
    return ((ah > bh ? ah : bh) << 32) | (al > bl ? al : bl);
  }
};
struct SsScanItemW { uint64_t old_head, new_head; };   // ... wide: the two maxima side by side
KJ_SS_HD SsScanItemW ss_scan_item_wide(uint64_t i, bool head_old, bool head_new) {
  const SsScanItemW s = {head_old ? i : 0ull, head_new ? i : 0ull};
  return s;
}
struct SsScanMaxW {
  KJ_SS_HD SsScanItemW operator()(SsScanItemW a, SsScanItemW b) const {
    const SsScanItemW s = {a.old_head > b.old_head ? a.old_head : b.old_head, a.new_head > b.new_head ? a.new_head : b.new_head};
    return s;
  }
};
// the new rank of entry i: round 1 counts from nseq, round h from the rank of the old group (the group's members are all
// active and lie side by side in the list, so the distance of the two heads in the list is the distance of the ranks)
KJ_SS_HD uint32_t ss_rank_first(uint32_t nseq, uint64_t scanned) { return nseq + (uint32_t)scanned; }
KJ_SS_HD uint32_t ss_rank_round(uint64_t key, uint64_t scanned) { return (uint32_t)(key >> 32) + ((uint32_t)scanned - (uint32_t)(scanned >> 32)); }
// entry i is a head and so is its successor (or there is none): alone in its group
KJ_SS_HD bool ss_is_final(uint64_t i, uint64_t n, uint64_t scanned, uint64_t scanned_next) {
  return (uint32_t)scanned == (uint32_t)i && (i + 1 == n || (uint32_t)scanned_next == (uint32_t)(i + 1));
}

// ... wide: first_rank = rank_bias + nseq
KJ_SS_HD uint64_t ss_rank_first(uint64_t first_rank, SsScanItemW scanned) { return first_rank + scanned.new_head; }
KJ_SS_HD uint64_t ss_rank_round(SsKeyW key, SsScanItemW scanned) { return key.hi + (scanned.new_head - scanned.old_head); }
KJ_SS_HD bool ss_is_final(uint64_t i, uint64_t n, SsScanItemW scanned, SsScanItemW scanned_next) {
  return scanned.new_head == i && (i + 1 == n || scanned_next.new_head == i + 1);
}
// round 1: the letters in front of a lane's first byte = the output index of its first letter (tile_base: letters in front of
// the lane's tile, before: in front of its wavefront inside the tile, inc - cnt: in front of the lane inside the wavefront)
KJ_SS_HD uint64_t ss_lane_base(uint64_t tile_base, uint32_t before, uint32_t inc, uint32_t cnt) { return tile_base + before + inc - cnt; }

// ---- the driver (sufsort.hip; host side, linked into libkaiju_mkfmi_gpu.so only) -------------------------------------------
#ifdef __cplusplus
#include <string>
struct kaiju_sufsort_stats;
// text: host pointer, tlen symbols, the last one a terminator; sa_out: host pointer, room for tlen - nseq positions.  Blocking.
// Status codes of mkfmi.h; err gets the message.
int kj_sufsort_device(const uint8_t *text, uint64_t tlen, int device_id, uint32_t *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats,
                      std::string &err);
int kj_sufsort_check_device(int device_id, std::string &err);
// the same sort for the stages that follow it on the device (kj_fmibuild.h): what stays in device memory when it ends
struct SsKeep {
  void *text = nullptr, *rank = nullptr, *sa = nullptr, *k0 = nullptr, *temp = nullptr;   // ss_text_alloc(tlen) bytes, 4 x tlen rounded up to 16, 4 nsuf, 8 nsuf, temp_bytes
  uint64_t temp_bytes = 0, nseq = 0, nsuf = 0, maxlen = 0, bytes = 0;                     // bytes: what the sort had allocated
};
int kj_sufsort_device_keep(const uint8_t *text, uint64_t tlen, int device_id, uint32_t *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats,
                           SsKeep *keep, std::string &err);
uint64_t kj_sufsort_need_bytes(uint64_t tlen, uint64_t nsuf, uint64_t *temp_bytes_out);
// the wide instantiation: 64-bit positions, tlen + rank_bias < 2^40 (ss_tlen_ok_wide); rank_bias = 0 outside the tests
int kj_sufsort_device_wide(const uint8_t *text, uint64_t tlen, int device_id, uint64_t *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats,
                           uint64_t rank_bias, std::string &err);
uint64_t kj_sufsort_need_bytes_wide(uint64_t tlen, uint64_t nsuf, uint64_t rank_bias, uint64_t *temp_bytes_out);
#endif

#endif
