"""Inputs of the SEG region tests (test_seg_lanes.py on the host, test_gpu_seg_regions.py on the device), built from seeds.
Each group is the smallest shape at which the mechanism named with it can fail; kj_core.h: seg_trim, seg_classes, seg_scan,
seg_regions, seg_compute, seg_compute_big."""
from __future__ import annotations

import json
import math
import os

import numpy as np

import util

LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
AMINO = frozenset(b"ACDEFGHIKLMNPQRSTVWY" + b"acdefghiklmnpqrstvwy")


def rand_pep(rng, n):
    return rng.choice(LETTERS, size=n).tobytes()


def stretch(rng, n, kind):
    """a low-complexity stretch of n residues: 0 one letter, 1 two letters 3 : 1 at random, 2 a period of two, 3 a period of three"""
    x = rng.choice(LETTERS, size=3, replace=False)
    if kind == 0:
        return bytes([x[0]]) * n
    if kind == 1:
        return rng.choice([x[0], x[0], x[0], x[1]], size=n).astype(np.uint8).tobytes()
    unit = bytes(x[:kind])
    return (unit * (n // kind + 1))[:n]


def window_cases():
    """lengths round the 12-residue window: nothing below 12 residues is ever flagged"""
    rng = np.random.default_rng(101)
    return [b"A" * n for n in (1, 11, 12, 13, 24)] + [rand_pep(rng, n) for n in (1, 11, 12, 13, 24)]


TIE_UNITS = (b"A", b"AC", b"ACD", b"AAC", b"ACDE")


def tie_cases(step=1):
    """many sub-windows of s_Trim's raw segment share one composition, so the visiting order decides the trimmed ends: the
    tie-break of reduce_min, a lane that keeps a later t.  Repeats of 12 .. 140 residues, bare and with 20 random residues in
    front, behind, on both sides"""
    rng = np.random.default_rng(102)
    out = []
    for unit in TIE_UNITS:
        for n in range(12, 141):
            rep = (unit * (n // len(unit) + 1))[:n]
            f, b = rand_pep(rng, 20), rand_pep(rng, 20)
            if (n - 12) % step == 0:
                out += [rep, f + rep, rep + b, f + rep + b]
    return out


# Palindromes (a flank, a short stretch of few letters, their mirror image) found by a search over 60000 of them: a
# sub-window and its mirror image have one composition and one length, so one probability, and the oracle's region of each
# of these is NOT its own mirror image - s_Trim's minimum was tied between the two and the visiting order, the earlier
# start, decided.  A reduction that loses the tie-break returns the mirrored window or leaves the lanes in disagreement.
TIE_WITNESSES = (
    b"LAGIPCCCLCCCPIGAL", b"HPDSYRRRPRRRYSDPH", b"ATKQFHHHAHHHFQKTA", b"MQDHYNNNQNNNYHDQM", b"NIHRVVVVNVVVVRHIN",
    b"QVWLVPCCCQCCCPVLWVQ", b"GHCQLQQQQGQQQQLQCHG", b"QIWFMAAAAIAAAAMFWIQ", b"GYDADQEEEGEEEQDADYG", b"HRMNFGQQQRQQQGFNMRH",
    b"HGVFESSSSHSSSSEFVGH", b"HVAPYLLLLHLLLLYPAVH", b"SGIPHFYYYGYYYFHPIGS", b"MILYATCEEEYEEECTAYLIM", b"SDGKMFWFFCKCFFWFMKGDS",
    b"YRRKELAAAAYAAAALEKRRY", b"DAEGCWWWWFEFWWWWCGEAD", b"RADMWWWWPWRWPWWWWMDAR", b"STIGQWQSPPIPPSQWQGITS", b"FYMGCEQQQQYQQQQECGMYF",
    b"PEVYYKGSSSESSSGKYYVEP", b"SWPAVCVTVVVWVVVTVCVAPWS", b"PLEDGFFLLFLPLFLLFFGDELP", b"VFAEWNRYYYYFYYYYRNWEAFV",
    b"LKVCAPWDDDDCDDDDWPACVKL", b"YETEHEEKEEEYEEEKEEHETEY", b"FRMPKSSWFWWMWWFWSSKPMRF", b"CDKASTTAATAADAATAATTSAKDC",
    b"RKKPWKKKKAAAKRKAAAKKKKWPKKR", b"CMAGKQGGTTGGGGMGGGGTTGGQKGAMC", b"TLWMFLLLNLNNLLLTLLLNNLNLLLFMWLT", b"CYMHDRPRRRRYRRRRPRDHMYC")


def tie_witnesses(seg_oracle):
    """TIE_WITNESSES, checked: palindromes with one region that is not symmetric"""
    for aa in TIE_WITNESSES:
        regs = seg_oracle(aa)
        assert aa == aa[::-1] and len(regs) == 1 and regs[0][0] != len(aa) - 1 - regs[0][1], aa
    return list(TIE_WITNESSES)


def window_entropies(aa):
    h = []
    for t in range(len(aa) - 11):
        c = {}
        for ch in aa[t: t + 12]:
            c[ch] = c.get(ch, 0) + 1
        h.append(-sum(v / 12 * math.log2(v / 12) for v in c.values()))
    return h


def first_raw_segment(aa):
    """length of the first raw segment SEG hands to s_Trim (window 12, locut 2.2, hicut 2.5; floating point: good for
    choosing inputs, not for expected values), 0 if no window triggers"""
    h = window_entropies(aa)
    for t, v in enumerate(h):
        if v <= 2.2:
            lo = hi = t
            while lo > 0 and h[lo - 1] <= 2.5:
                lo -= 1
            while hi + 1 < len(h) and h[hi + 1] <= 2.5:
                hi += 1
            return hi - lo + 12
    return 0


def limit_cases():
    """raw segments round kSegPacked = 63 (beyond it the generic window function and the global ln(n!) table) and stretches
    round kSegMaxTrim = 50 and far beyond it (D = 50 window lengths, 1275 sub-windows: twenty rounds of 64 lanes)"""
    rng = np.random.default_rng(103)
    out = []
    for n in list(range(46, 72)) + list(range(108, 143)):
        for kind in (0, 1, 2):
            out.append(rand_pep(rng, 25) + stretch(rng, n, kind) + rand_pep(rng, 25))
    return out


STAGE_LENGTHS = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)


def stage_cases():
    """fragments round the LDS stage of the SEG kernels (2048 bytes for k_seg, 1024 / 512 / 256 for teams of 32 / 16 / 8; longer
    fragments are read from device memory and scanned without the window classes): random peptides with three or four
    low-complexity stretches, the last of them straddling the last 20 residues"""
    rng = np.random.default_rng(104)
    out = []
    for k, n in enumerate(STAGE_LENGTHS):
        aa = bytearray(rand_pep(rng, n))
        nst = 3 + k % 2
        for j in range(nst - 1):
            a = (j + 1) * n // (nst + 1) + int(rng.integers(0, 9))
            s = stretch(rng, int(rng.integers(14, 40)), j % 3)
            aa[a: a + len(s)] = s
        a, b = n - 20 - int(rng.integers(5, 15)), n - (k % 3) * 4         # ends at the last residue, or 4 or 8 in front of it
        aa[a: b] = stretch(rng, b - a, k % 2)
        assert len(aa) == n
        out.append(bytes(aa))
    return out


def islands(n_islands, seed, gap=30, island=14):
    """random stretches of `gap` residues alternating with homopolymer islands"""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(n_islands):
        parts.append(rand_pep(rng, gap))
        parts.append(bytes([rng.choice(LETTERS)]) * island)
    parts.append(rand_pep(rng, gap))
    return b"".join(parts)


# region count of the oracle -> (islands, seed): fragments round what a record of the SEG pass holds (15 regions) and what its
# scan lists hold (32 segments).  The tests assert the counts.
RECORD_CASES = {14: (13, 3), 15: (14, 3), 16: (15, 3), 31: (30, 3), 32: (31, 3), 33: (32, 3), 43: (42, 1)}


def record_cases():
    return {want: islands(*RECORD_CASES[want]) for want in sorted(RECORD_CASES)}


def long_case():
    """a protein of more than 65535 residues (16-bit positions of a record) with a few stretches, one across position 65535
    and the last behind it"""
    rng = np.random.default_rng(106)
    aa = bytearray(rand_pep(rng, 66100))
    for a, n, kind in ((1000, 30, 0), (30011, 45, 1), (65520, 30, 0), (65900, 40, 2)):
        aa[a: a + n] = stretch(rng, n, kind)
    return bytes(aa)


def short_flagged_candidates():
    """about 260 peptides of 14 .. 40 residues, most of them low-complexity (the grid-stride batch cycles through those
    for which the oracle reports a region)"""
    rng = np.random.default_rng(107)
    out = []
    for k in range(260):
        n = 14 + k % 27
        s = int(rng.integers(12, n + 1))
        a = int(rng.integers(0, n - s + 1))
        aa = bytearray(rand_pep(rng, n))
        aa[a: a + s] = stretch(rng, s, k % 4)
        out.append(bytes(aa))
    return out


def fuzz_cases(count=1500):
    """the generator of test_kernel_emu.py::test_seg_known_answers (seed 77): peptides of 12 .. 150 residues with a planted
    stretch of one to four letters, and the strings of the known answers of tests/golden/kat_seg.json"""
    rng = np.random.default_rng(77)
    out = []
    for _ in range(count):
        n = int(rng.integers(12, 151))
        few = rng.choice(LETTERS, size=int(rng.integers(1, 5)), replace=False)
        aa = rng.choice(LETTERS, size=n)
        a = int(rng.integers(0, n))
        b = min(n, a + int(rng.integers(8, 90)))
        aa[a:b] = rng.choice(few, size=b - a)
        out.append(aa.tobytes())
    return out


def kat_cases():
    with open(os.path.join(util.GOLD, "kat_seg.json")) as f:
        return [(aa.encode(), [tuple(r) for r in regs]) for aa, regs in json.load(f)]


def separator_cases():
    """reads that stage 1 cuts into several fragments (X, *, letters that are no amino acid) with lower-case residues: the
    region positions are relative to each fragment's start"""
    rng = np.random.default_rng(108)
    out = [b"AAAAAAAAAAAAAAAAXACDEFGHIKLMNPQRSTVWY*GGGGGGGGGGGGGGSSSSSSSSSGGGGKLMNPQRW",
           b"aaaaaaaaaaaaaaaaKLMNPqqqqqqqqqqqqqqqqqXXsssssssssssssT", b"X", b"*AAAAAAAAAAAAAAAAAAAA*", b"AAAAAAAAAAAX"]
    for _ in range(40):
        parts = []
        for _ in range(int(rng.integers(2, 6))):
            n = int(rng.integers(5, 70))
            aa = bytearray(rand_pep(rng, n))
            if rng.random() < 0.7 and n >= 14:
                s = int(rng.integers(12, n + 1))
                a = int(rng.integers(0, n - s + 1))
                aa[a: a + s] = stretch(rng, s, int(rng.integers(0, 4)))
            piece = bytes(aa)
            if rng.random() < 0.4:
                piece = piece.lower()
            parts.append(piece)
            parts.append(bytes(rng.choice(np.frombuffer(b"X*BZJOU", dtype=np.uint8), size=int(rng.integers(1, 3))).tolist()))
        out.append(b"".join(parts[:-1]) if rng.random() < 0.5 else b"".join(parts))
    return out


def fragments_of(read, m=1):
    """(start, fragment in upper case) of every run of amino-acid letters of at least m residues: stage 1 of protein reads
    (kj_core.h: build_fragments_protein) in MEM order of emission"""
    out, start = [], None
    for x, ch in enumerate(read + b"\0"):
        if ch in AMINO:
            if start is None:
                start = x
        elif start is not None:
            if x - start >= m:
                out.append((start, read[start:x].upper()))
            start = None
    return out


class SegOracle:
    """oracle.seg with room for every region a peptide can have, each distinct peptide computed once"""

    def __init__(self, oracle):
        self.oracle, self.cache = oracle, {}

    def __call__(self, aa: bytes):
        got = self.cache.get(aa)
        if got is None:
            got = self.cache[aa] = [tuple(r) for r in self.oracle.seg(aa, max_regions=len(aa) // 8 + 16)]
        return got
