"""The wide (64-bit) instantiation of the suffix sorter's per-lane logic (kaiju_amd/csrc/kj_sufsort.h) on the host:
tests/emu/sufsort_wide_emu.cpp drives the wide functions through the whole round loop as the wide kernels of sufsort.hip run
them - two stable sorts a round, by rank[p + h] and then by rank[p] - with every rank rank_bias higher, so that with a bias
beyond 2^32 every rank, round key and rank comparison of these small texts has high bits.  What a bias cannot lift - positions,
list indexes, tile bases - goes through the single functions with arguments beyond 2^32."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sufsort_inputs as si
import util

BIASES = (0, 2**32 + 12345)
U64 = C.c_uint64


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sufsort_wide_emu") / "libsufsort_wide_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(util.ROOT, "tests", "emu", "sufsort_wide_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.sufsort_wide_emu.argtypes = [C.c_void_p, U64, U64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sufsort_wide_emu.restype = C.c_uint32
    L.sufsort_wide_emu_round_key.argtypes = [U64, U64, U64, C.c_void_p]
    L.sufsort_wide_emu_heads.argtypes = [U64] * 5
    L.sufsort_wide_emu_heads.restype = C.c_uint32
    L.sufsort_wide_emu_scan.argtypes = [U64] * 4 + [C.c_void_p]
    L.sufsort_wide_emu_scan_item.argtypes = [U64, C.c_int, C.c_int, C.c_void_p]
    for name, args in (("rank_first", [U64] * 2), ("rank_round", [U64] * 3), ("lane_base", [U64, C.c_uint32, C.c_uint32, C.c_uint32]),
                       ("scratch_bytes_wide", [U64] * 2), ("scratch_bytes", [U64] * 2)):
        f = getattr(L, "sufsort_wide_emu_" + name)
        f.argtypes, f.restype = args, U64
    L.sufsort_wide_emu_is_final.argtypes = [U64] * 4
    L.sufsort_wide_emu_tlen_ok_wide.argtypes = [U64]
    L.sufsort_wide_emu_tlen_ok.argtypes = [U64]
    return L


def run_emu(L, text, bias):
    sa = np.full(max(1, int(np.count_nonzero(text))), 2**64 - 1, dtype=np.uint64)
    n, rounds, active = C.c_uint64(0), C.c_uint32(0), np.zeros(64, dtype=np.uint64)
    t = np.ascontiguousarray(text)
    bad = L.sufsort_wide_emu(t.ctypes.data, len(t), bias, sa.ctypes.data, C.byref(n), C.byref(rounds), active.ctypes.data)
    return bad, sa[: n.value], rounds.value, active


def pair(f, *args):
    out = np.zeros(4, dtype=np.uint64)
    f(*args, out.ctypes.data)
    return [int(v) for v in out]


# ---- the whole loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", BIASES)
@pytest.mark.parametrize("name", [n for n, _ in si.cases()])
def test_wide_emulation_gives_the_naive_order(emu, name, bias):
    text = si.case(name)
    bad, sa, rounds, active = run_emu(emu, text, bias)
    assert bad == 0, f"violations {bad:#x}"
    want = si.expected(name)
    assert len(sa) == len(want) == int(np.count_nonzero(text))
    assert sa.dtype == np.uint64 and np.array_equal(sa, want.astype(np.uint64))
    assert rounds <= si.round_bound(text), (rounds, si.round_bound(text))
    assert int(active[0]) == len(want)
    act = [int(a) for a in active[:rounds]]
    assert all(a >= b for a, b in zip(act, act[1:])) and all(a > 0 for a in act) and int(active[rounds]) == 0
    if rounds > 1:
        assert act[1] == si.expected_active_after_first_round(name)
    else:
        assert si.expected_active_after_first_round(name) == 0


def test_the_bias_changes_neither_rounds_nor_active_counts(emu):
    for name in ("identical_40x300A", "one_5000xAC", "family_30x900"):
        runs = [run_emu(emu, si.case(name), b) for b in BIASES]
        assert 5 <= runs[0][2] == runs[1][2] and np.array_equal(runs[0][3], runs[1][3]), name


def test_ranks_beyond_2_40_are_refused(emu):
    text = si.case("iid_255")
    assert run_emu(emu, text, 2**40 - 10)[0] == 512          # V_BOUND: 255 + 2^40 - 10 >= 2^40
    assert run_emu(emu, text, 2**40 - 256)[0] == 0


# ---- the single functions beyond 2^32 ----------------------------------------------------------------------------------------
def test_round_key_keeps_both_ranks_whole(emu):
    hi, lo, ahead, outside = pair(emu.sufsort_wide_emu_round_key, 2**33 + 5, 2**32 + 1, 2**32 + 77)
    assert (hi, lo, ahead) == (2**33 + 5, 2**32 + 1, 2**32 + 1)
    assert outside == 0                                      # p + h == tlen: the load is guarded


def test_heads_see_differences_above_bit_32(emu):
    h = emu.sufsort_wide_emu_heads
    assert h(5, 2**33 + 5, 7, 2**33 + 5, 7) == 0             # the same key: no head
    assert h(0, 2**33 + 5, 7, 2**33 + 5, 7) == 3             # the first entry is a head of both
    assert h(5, 5, 7, 2**32 + 5, 7) == 3                     # rank[p] differs in bit 32 only: another old group
    assert h(5, 2**33 + 5, 7, 2**34 + 5, 7) == 3
    assert h(5, 2**33 + 5, 7, 2**33 + 5, 2**32 + 7) == 2     # rank[p + h] differs in bit 32 only: the old group splits
    assert h(5, 2**33 + 5, 2**39 + 7, 2**33 + 5, 2**38 + 7) == 2


def test_scan_operator_takes_each_maximum_whole(emu):
    assert pair(emu.sufsort_wide_emu_scan, 2**32 + 7, 3, 5, 2**32 + 9)[:2] == [2**32 + 7, 2**32 + 9]
    assert pair(emu.sufsort_wide_emu_scan, 5, 2**32 + 9, 2**32 + 7, 3)[:2] == [2**32 + 7, 2**32 + 9]
    assert pair(emu.sufsort_wide_emu_scan, 2**32, 2**32, 1, 1)[:2] == [2**32, 2**32]       # a maximum of the low halves alone would say 1
    assert pair(emu.sufsort_wide_emu_scan_item, 2**32 + 3, 1, 0)[:2] == [2**32 + 3, 0]
    assert pair(emu.sufsort_wide_emu_scan_item, 2**32 + 3, 0, 1)[:2] == [0, 2**32 + 3]


def test_new_ranks_keep_their_high_bits(emu):
    assert emu.sufsort_wide_emu_rank_round(2**33 + 5, 2**32 + 7, 2**32 + 9) == 2**33 + 7
    assert emu.sufsort_wide_emu_rank_round(2**33 + 5, 7, 2**32 + 9) == 2**33 + 2**32 + 7       # heads 2^32 + 2 apart
    assert emu.sufsort_wide_emu_rank_first(2**32 + 12345 + 30, 2**32 + 9) == 2**33 + 12345 + 39


def test_is_final_compares_whole_indexes(emu):
    f = emu.sufsort_wide_emu_is_final
    i = 2**32
    assert f(i, i + 1, i, 0) == 1                            # i + 1 == n = 2^32 + 1: the last entry, a head
    assert f(i, i + 1, 0, 0) == 0                            # ... whose group began at entry 0: equal in the low 32 bits only
    assert f(i, i + 5, i, i + 1) == 1
    assert f(i, i + 5, i, i) == 0                            # the successor belongs to the group
    assert f(i, i + 5, i, 1) == 0                            # (i + 1 in the low 32 bits only)


def test_tile_base_beyond_2_32(emu):
    assert emu.sufsort_wide_emu_lane_base(2**32 + 100, 1000, 48, 16) == 2**32 + 1132
    assert emu.sufsort_wide_emu_lane_base(2**39 + 100, 0, 0, 0) == 2**39 + 100


# ---- constants and sizes -----------------------------------------------------------------------------------------------------
def test_bounds_of_the_two_instantiations(emu):
    assert emu.sufsort_wide_emu_tlen_ok_wide(2**40 - 1) == 1 and emu.sufsort_wide_emu_tlen_ok_wide(2**40) == 0
    assert emu.sufsort_wide_emu_tlen_ok(0xefffffff) == 1 and emu.sufsort_wide_emu_tlen_ok(0xf0000000) == 0


def test_scratch_of_the_wide_sort_fits_the_card(emu):
    """56 bytes per symbol is what passes the size check of an idle 288 GB card at 4.4 G symbols; the formula has 49: text 1,
    ranks 8, keys 2 x 8, positions 2 x 8, active list 8"""
    nsuf, nseq = 4_400_000_000, 15_500_000
    b = emu.sufsort_wide_emu_scratch_bytes_wide(nsuf + nseq, nsuf)
    assert 49 * nsuf <= b <= 56 * nsuf
    assert b <= 49.2 * (nsuf + nseq)
    # the narrow formula is what it was: about 33 bytes a symbol
    assert 33 * 10**6 <= emu.sufsort_wide_emu_scratch_bytes(10**6 + 1000, 10**6) <= 33.2 * 10**6
    # text 1001008 + 32, ranks 4 x 1001001, keys, positions and list 28 x 10^6, 4 x 246 tile counts, 6 x 256
    assert emu.sufsort_wide_emu_scratch_bytes(10**6 + 1000, 10**6) == 1001040 + 4004004 + 28 * 10**6 + 984 + 1536


def test_the_host_library_has_no_wide_device_entry_point():
    from kaiju_amd import build as kbuild
    L = C.CDLL(kbuild.build_mkfmi())
    assert hasattr(L, "kaiju_build_fmi") and not hasattr(L, "kaiju_suffix_sort_device_wide")
