"""The suffix sorter's per-lane logic (kaiju_amd/csrc/kj_sufsort.h) on the host: tests/emu/sufsort_emu.cpp drives the functions
the kernels of sufsort.hip are made of through the whole round loop, with std::stable_sort in the radix sort's place.  On every
text of tests/sufsort_inputs.py the result must be the naive expectation (positions sorted by symbols up to and including the
terminator, then by position); the emulation itself reports a final rank that changed, an active set that grew, a final suffix
in the active list and a load of rank[p + h] outside p's own sequence."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sufsort_inputs as si
import util


@pytest.fixture(scope="module")
def ss_emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sufsort_emu") / "libsufsort_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(util.ROOT, "tests", "emu", "sufsort_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.sufsort_emu.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sufsort_emu.restype = C.c_uint32
    L.sufsort_emu_constants.argtypes = [C.c_void_p]
    L.sufsort_emu_scratch_bytes.argtypes = [C.c_uint64, C.c_uint64]
    L.sufsort_emu_scratch_bytes.restype = C.c_uint64
    return L


def run_emu(L, text):
    sa = np.full(max(1, int(np.count_nonzero(text))), 0xffffffff, dtype=np.uint32)
    n, rounds, active = C.c_uint64(0), C.c_uint32(0), np.zeros(64, dtype=np.uint64)
    t = np.ascontiguousarray(text)
    bad = L.sufsort_emu(t.ctypes.data, len(t), sa.ctypes.data, C.byref(n), C.byref(rounds), active.ctypes.data)
    return bad, sa[: n.value], rounds.value, active


def test_constants_are_the_ones_the_inputs_were_made_for(ss_emu):
    k = np.zeros(8, dtype=np.uint64)
    ss_emu.sufsort_emu_constants(k.ctypes.data)
    assert int(k[0]) == si.K and int(k[1]) == si.TILE and int(k[2]) == 16 and int(k[3]) == 16
    assert int(k[4]) == 1 and int(k[5]) == 0            # the 32-bit boundary of the host builder: 0xf0000000 is refused
    # about 30 bytes a symbol: text 1, ranks 4, keys 2 x 8, values 2 x 4, active list 4
    assert 33 * 10**6 <= ss_emu.sufsort_emu_scratch_bytes(10**6 + 1000, 10**6) <= 33.2 * 10**6


@pytest.mark.parametrize("name", [n for n, _ in si.cases()])
def test_emulation_gives_the_naive_order(ss_emu, name):
    text = si.case(name)
    bad, sa, rounds, active = run_emu(ss_emu, text)
    assert bad == 0, f"violations {bad:#x}"
    want = si.expected(name)
    assert len(sa) == len(want) == int(np.count_nonzero(text))
    assert np.array_equal(sa, want)
    assert rounds <= si.round_bound(text), (rounds, si.round_bound(text))
    assert int(active[0]) == len(want)
    act = [int(a) for a in active[:rounds]]
    assert all(a >= b for a, b in zip(act, act[1:])) and all(a > 0 for a in act) and int(active[rounds]) == 0
    if rounds > 1:
        assert act[1] == si.expected_active_after_first_round(name)
    else:
        assert si.expected_active_after_first_round(name) == 0


def test_deep_inputs_take_the_rounds_they_need(ss_emu):
    """40 x 300 A: every group is tied down to the terminators, five rounds at least; the bound is met with equality there"""
    for name, at_least in (("identical_40x300A", 5), ("one_5000xAC", 5), ("family_30x900", 5)):
        _, _, rounds, _ = run_emu(ss_emu, si.case(name))
        assert at_least <= rounds <= si.round_bound(si.case(name)), name


def test_iid_texts_are_nearly_done_after_the_first_round():
    for name in si.IID_NAMES:
        n = len(si.expected(name))
        assert si.expected_active_after_first_round(name) <= 0.1 * n, name


def test_the_host_library_has_no_device_entry_points():
    from kaiju_amd import build as kbuild
    L = C.CDLL(kbuild.build_mkfmi())
    assert hasattr(L, "kaiju_build_fmi") and not hasattr(L, "kaiju_build_fmi_device") and not hasattr(L, "kaiju_suffix_sort_device")
