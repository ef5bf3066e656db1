"""The suffix sort of the index builder on the device (kaiju_amd/csrc/sufsort.hip, kj_sufsort.h; libkaiju_mkfmi_gpu.so).
suffix_sort on the texts of tests/sufsort_inputs.py against the naive expectation, position by position; the rounds against
the bound that follows from the definition and the active count behind the first round against the count the expectation
gives; whole .fmi files built with device=0 against the host builder's, byte for byte; the refusals."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import sufsort_inputs as si
from kaiju_amd import mkfmi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sorter(gpu_lib):
    return mkfmi._lib_gpu()


@pytest.mark.parametrize("name", [n for n, _ in si.cases()])
def test_suffix_sort_gives_the_naive_order(sorter, name):
    text = si.case(name)
    sa, stats = mkfmi.suffix_sort(text, device=0)
    want = si.expected(name)
    print(name, "suffixes", len(want), "rounds", stats["rounds"], "bound", si.round_bound(text), "active", stats["active"][: stats["rounds"] + 1],
          "ms", round(stats["ms_sort"], 3))
    assert len(sa) == len(want)
    bad = np.flatnonzero(sa != want)
    assert len(bad) == 0, (name, "first difference at row", int(bad[0]), int(sa[bad[0]]), int(want[bad[0]]))
    # rounds: K * 2^(r-1) symbols are compared after round r, nothing is active beyond maxlen + 1 (sufsort_inputs.round_bound)
    assert stats["rounds"] <= si.round_bound(text)
    assert stats["active"][0] == len(want)
    act = stats["active"][: min(stats["rounds"], 16)]
    assert all(a >= b > 0 for a, b in zip(act, act[1:]))
    # the compaction behind the first round keeps exactly the suffixes whose first K symbols are neither unique nor hold the terminator
    assert (stats["active"][1] if stats["rounds"] > 1 else 0) == si.expected_active_after_first_round(name)


def test_iid_texts_are_nearly_done_after_the_first_round(sorter):
    for name in si.IID_NAMES:
        _, stats = mkfmi.suffix_sort(si.case(name), device=0)
        n = stats["active"][0]
        left = stats["active"][1] if stats["rounds"] > 1 else 0
        assert left == si.expected_active_after_first_round(name), name
        assert left <= 0.1 * n, (name, left, n)


def test_deep_groups_take_at_least_five_rounds(sorter):
    _, stats = mkfmi.suffix_sort(si.case("identical_40x300A"), device=0)
    assert 5 <= stats["rounds"] <= si.round_bound(si.case("identical_40x300A"))


# ---- whole files ---------------------------------------------------------------------------------------------------------
def same_file(a, b):
    return os.path.getsize(a) == os.path.getsize(b) and filecmp.cmp(a, b, shallow=False)


def test_golden_database_same_bytes(sorter, golden, tmp_path):
    faa = os.path.join(golden.dir, "db.faa")
    host, dev = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi")
    mkfmi.build_fmi(faa, host, threads=2, exponent=3)
    mkfmi.build_fmi(faa, dev, threads=2, exponent=3, device=0)
    assert same_file(dev, host)
    assert same_file(dev, golden.fmi)


@pytest.mark.parametrize("nseq,seed,exponent,threads", [(257, 1, 3, 1), (1000, 2, 3, 4), (1531, 3, 5, 3), (64, 4, 2, 8)])
def test_synthetic_databases_same_bytes(sorter, tmp_path, nseq, seed, exponent, threads):
    _, leaves = synth.make_taxonomy(3, 3, 3)
    db = synth.make_db(nseq=nseq, seed=seed, leaves=leaves, max_len=900)
    faa = str(tmp_path / "db.faa")
    synth.write_fasta(db, faa)
    host, dev = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi")
    mkfmi.build_fmi(faa, host, threads=threads, exponent=exponent)
    mkfmi.build_fmi(faa, dev, threads=threads, exponent=exponent, device=0)
    assert same_file(dev, host)


def test_replicated_database_same_bytes(sorter, golden, tmp_path):
    faa = os.path.join(golden.dir, "db.faa")
    host, dev = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi")
    mkfmi.build_fmi_replicated(faa, host, copies=3, threads=3, exponent=3, copy_taxids=[11, 222, 3333])
    mkfmi.build_fmi_replicated(faa, dev, copies=3, threads=3, exponent=3, copy_taxids=[11, 222, 3333], device=0)
    assert same_file(dev, host)


def test_forced_64_bit_builder_widens_the_device_result(sorter, golden, tmp_path, monkeypatch):
    faa = os.path.join(golden.dir, "db.faa")
    host, dev = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi")
    mkfmi.build_fmi(faa, host, threads=3, exponent=3)
    monkeypatch.setenv("KAIJU_MKFMI_FORCE64", "1")
    mkfmi.build_fmi(faa, dev, threads=3, exponent=3, device=0)
    assert same_file(dev, host)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_text_at_the_32_bit_boundary_is_refused_by_its_size(sorter):
    """the size check alone: the text behind the pointer has one symbol and is never looked at"""
    text, sa = np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    n = C.c_uint64(7)
    for tlen in (0xf0000000, 0xf0000001, 1 << 32, 1 << 40):
        rc = sorter.kaiju_suffix_sort_device(text.ctypes.data, tlen, 0, sa.ctypes.data, C.byref(n), None)
        assert rc == -1, tlen                                   # KAIJU_GPU_ERR_ARG
        assert b"kaiju_build_fmi" in sorter.kaiju_build_fmi_error()     # the message names the host builder


def test_bad_device_id_is_refused(sorter, golden, tmp_path):
    text, sa = si.case("iid_255"), np.zeros(255, dtype=np.uint32)
    n = C.c_uint64(0)
    for dev in (-1, 4096):
        assert sorter.kaiju_suffix_sort_device(text.ctypes.data, len(text), dev, sa.ctypes.data, C.byref(n), None) == -1
        assert sorter.kaiju_build_fmi_device(os.path.join(golden.dir, "db.faa").encode(), str(tmp_path / "x.fmi").encode(), 1, 3, dev) == -1
        assert not os.path.exists(tmp_path / "x.fmi")
    with pytest.raises(Exception, match="device_id"):
        mkfmi.build_fmi(os.path.join(golden.dir, "db.faa"), str(tmp_path / "y.fmi"), device=4096)


def test_text_must_end_with_a_terminator_and_hold_codes_only(sorter):
    sa, n = np.zeros(8, dtype=np.uint32), C.c_uint64(0)
    for t in (np.array([1, 2, 3], dtype=np.uint8), np.array([1, 21, 0], dtype=np.uint8)):
        assert sorter.kaiju_suffix_sort_device(t.ctypes.data, len(t), 0, sa.ctypes.data, C.byref(n), None) == -1
