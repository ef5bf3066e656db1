"""The window-probability table of s_Trim (kj_core.h: seg_prob_lookup, seg_trim; host_tables.cpp: seg_prob_table)
on the host.  ln P0 of a sub-window is a function of the multiset of its letter counts; the table holds the double that
seg_prob_of_counts returns for every multiset of windows of up to kSegTabMax residues, and seg_trim's prefix-count path takes
it from there.  Every comparison is of 64-bit patterns or of integers: exact.  tests/emu/seg_table_emu.cpp is built twice, with
the table and with -DKJ_SEG_NO_TABLE; tests/test_gpu_seg_prob_table.py runs the same peptides on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import seg_inputs as si
import util

# partitions of 1 .. kSegTabMax into at most 20 parts
ENTRIES = {24: 7323, 32: 43201, 40: 207041}
SRC = os.path.join(util.EMU_DIR, "seg_table_emu.cpp")


def build(so, defines):
    srcs = [SRC, os.path.join(util.CSRC, "host_tables.cpp")]
    deps = srcs + [os.path.join(util.CSRC, f) for f in ("kj_core.h", "host_tables.h")]
    if not (os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in deps)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-pthread", "-DKJ_SEG_HIST"]
                       + ["-D" + d for d in defines] + ["-o", so] + srcs, check=True)
    L = C.CDLL(so)
    L.ste_open.argtypes = [C.c_char_p, C.c_int]
    L.ste_info.argtypes = [C.c_void_p]
    L.ste_check_entries.argtypes = [C.c_uint64, C.c_void_p]
    L.ste_window.argtypes = [C.c_void_p, C.c_void_p]
    L.ste_seg.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    err = C.create_string_buffer(256)
    assert L.ste_open(err, 256) == 0, err.value
    return L


@pytest.fixture(scope="module")
def tab():
    return build(os.path.join(util.EMU_DIR, "libkaiju_seg_table_emu.so"), ())


@pytest.fixture(scope="module")
def notab():
    return build(os.path.join(util.EMU_DIR, "libkaiju_seg_table_emu_notable.so"), ("KJ_SEG_NO_TABLE",))


def info(L):
    out = np.zeros(6, dtype=np.uint64)
    L.ste_info(out.ctypes.data)
    return dict(zip(("tab_max", "entries", "slots", "probe", "on", "occupied"), (int(v) for v in out)))


def counts20(counts):
    cnt = np.zeros(20, dtype=np.int32)
    cnt[: len(counts)] = counts
    return cnt


def window(L, counts):
    """(seg_prob_lookup finds the multiset, what it found has the bit pattern of seg_prob_of_counts)"""
    out = np.zeros(2, dtype=np.uint64)
    L.ste_window(counts20(counts).ctypes.data, out.ctypes.data)
    return int(out[0]), int(out[1])


def seg(L, aa, prefix=True, drop=None):
    """(regions or None where the scan lists overflowed, the counters of the call [4][64]: raw segment lengths, window lengths
    served by the table, computed on the prefix-count path, computed on the other paths)"""
    left, right = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32)
    hist = np.zeros((4, 64), dtype=np.uint64)
    dropped = counts20(drop) if drop is not None else None
    n = L.ste_seg(aa, len(aa), 1 if prefix else 0, dropped.ctypes.data if drop is not None else None, left.ctypes.data,
                  right.ctypes.data, hist.ctypes.data)
    assert n >= -1, (n, aa)
    return (None if n < 0 else [(int(left[k]), int(right[k])) for k in range(n)]), hist


def test_every_entry(tab):
    """every partition of every l <= kSegTabMax into at most 20 parts, its parts dealt to the letters in a seeded random order:
    the lookup has the bit pattern of seg_prob_of_counts; entry count, distinct keys, load and probe bound of the table"""
    i = info(tab)
    assert i["tab_max"] in ENTRIES and i["on"] == 1
    assert i["entries"] == i["occupied"] == ENTRIES[i["tab_max"]]
    assert i["slots"] & (i["slots"] - 1) == 0 and 2 * i["entries"] <= i["slots"]
    for seed in (1, 2):
        out = np.zeros(5, dtype=np.uint64)
        tab.ste_check_entries(seed, out.ctypes.data)
        parts, mismatches, missing, distinct, max_probe = (int(v) for v in out)
        assert parts == ENTRIES[i["tab_max"]]
        assert (mismatches, missing) == (0, 0)
        assert distinct == parts
        assert max_probe == i["probe"] >= 1                       # the recorded bound is the true maximum


def test_fall_through(tab, oracle):
    """windows the table does not serve take seg_prob_of_counts: one residue more than kSegTabMax, every window of the path
    without prefix counts, and a key that is absent although its length is covered (the lane computes its windows directly)"""
    m = info(tab)["tab_max"]
    for counts in ([m - 5, 3, 1, 1], [m], [2] * (m // 2), [1]):
        assert window(tab, counts) == (1, 1), counts
    for counts in ([m - 4, 3, 1, 1], [m + 1], [3] * 20):
        assert sum(counts) > m and window(tab, counts) == (0, 0), counts
    # a raw segment of m + 1 residues: its one window of m + 1 residues is computed, the others come from the table
    rng = np.random.default_rng(212)
    aa = next(x for x in (si.rand_pep(rng, 25) + si.stretch(rng, n, k) + si.rand_pep(rng, 25) for n in range(m - 16, m + 4) for k in (0, 1, 2))
              if si.first_raw_segment(x) == m + 1)
    want = [tuple(r) for r in oracle.seg(aa, max_regions=32)]
    regs, hist = seg(tab, aa)
    first = int(np.flatnonzero(hist[0])[-1])
    assert regs == want and first >= m + 1 and hist[2][m + 1] >= 1 and hist[2][: m + 1].sum() == 0 and hist[1][m + 1:].sum() == 0
    assert hist[1].sum() > 0 and hist[3].sum() == 0
    # the path without prefix counts never asks the table
    regs0, hist0 = seg(tab, aa, prefix=False)
    assert regs0 == want and hist0[3].sum() == hist[1].sum() + hist[2].sum() and hist0[1].sum() == 0 and hist0[2].sum() == 0
    # an absent key: twelve times one letter, a window of the homopolymer below
    homo = b"ACDEFGHIKLMNPQRSTVWY" + b"A" * 18 + b"ACDEFGHIKLMNPQRSTVWY"
    want = [tuple(r) for r in oracle.seg(homo, max_regions=32)]
    full, hist_full = seg(tab, homo)
    regs, hist = seg(tab, homo, drop=[12])
    assert full == regs == want
    assert hist_full[2].sum() == 0 and hist[2].sum() == hist_full[1].sum() > 0          # every window again, by the direct function


def raw_segment_cases(m):
    """peptides whose first raw segment has m - 1, m, m + 1, 63 and 64 residues, and stretches far beyond kSegMaxTrim = 50"""
    rng = np.random.default_rng(211)
    want = {m - 1, m, m + 1, 63, 64}
    out, seen = [], set()
    for n in list(range(m - 16, m + 4)) + list(range(48, 68)) + [115, 131]:
        for kind in (0, 1, 2):
            aa = si.rand_pep(rng, 25) + si.stretch(rng, n, kind) + si.rand_pep(rng, 25)
            raw = si.first_raw_segment(aa)
            if (raw in want and raw not in seen) or n > 100:
                seen.add(raw)
                out.append(aa)
    assert want <= seen and max(seen) > 64 + 50, sorted(seen)
    return out


def region_cases(m):
    return (list(si.TIE_WITNESSES) + si.tie_cases(step=4) + si.fuzz_cases(400) + [aa for aa, _ in si.kat_cases()] + raw_segment_cases(m))


def test_regions(tab, notab, oracle):
    """palindromes with a tied minimum, periodic repeats, fuzzed peptides, raw segments round kSegTabMax, 63 and kSegMaxTrim:
    the regions with the table == without it == the oracle's; the table serves exactly the windows of up to kSegTabMax
    residues of raw segments of up to 63"""
    m = info(tab)["tab_max"]
    assert info(notab)["on"] == 0
    seg_oracle = si.SegOracle(oracle)
    served = np.zeros(64, dtype=np.uint64)
    cases = region_cases(m)
    for aa in cases:
        got, hist = seg(tab, aa)
        ref, hist0 = seg(notab, aa)
        assert got == ref, aa
        if got is not None:
            assert got == seg_oracle(aa), aa
        assert hist0[1].sum() == 0 and np.array_equal(hist[0], hist0[0]) and np.array_equal(hist[3], hist0[3])
        assert np.array_equal(hist[1] + hist[2], hist0[2])                          # the same windows, served or computed
        assert hist[1][m + 1:].sum() == 0 and hist[2][: m + 1].sum() == 0
        served += hist[1]
    assert sum(1 for aa in cases if seg_oracle(aa)) > len(cases) * 2 // 3
    assert served[2] > 0 and served[m] > 0
