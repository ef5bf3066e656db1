"""The wide instantiation of the suffix sort on the device (kaiju_amd/csrc/sufsort.hip, kj_sufsort.h: 64-bit positions, ranks
and list indexes; two stable radix sorts a round).  suffix_sort(wide=True) on the texts of tests/sufsort_inputs.py against the
naive expectation with rank_bias 0, 2^32 + 12345 and 2^39: with a bias every rank, every round key and every rank comparison of
these small texts lies beyond 2^32 in the real kernels.  Narrow against wide; whole .fmi files built through the wide sort
(KAIJU_MKFMI_FORCE64 + KAIJU_MKFMI_DEVICE_WIDE) against the host builder's, byte for byte; the refusals."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import sufsort_inputs as si
from kaiju_amd import mkfmi, synth

pytestmark = pytest.mark.gpu

BIASES = (0, 2**32 + 12345, 2**39)
WIDE_LINE = "wide suffix sort: needs"          # what the wide driver prints under KAIJU_GPU_LOAD_TIMES, and the narrow one does not


@pytest.fixture(scope="module")
def sorter(gpu_lib):
    return mkfmi._lib_gpu()


@pytest.mark.parametrize("bias", BIASES)
@pytest.mark.parametrize("name", [n for n, _ in si.cases()])
def test_wide_suffix_sort_gives_the_naive_order(sorter, name, bias):
    text = si.case(name)
    sa, stats = mkfmi.suffix_sort(text, device=0, wide=True, rank_bias=bias)
    want = si.expected(name)
    print(name, "bias", bias, "suffixes", len(want), "rounds", stats["rounds"], "bound", si.round_bound(text), "active", stats["active"][: stats["rounds"] + 1],
          "ms", round(stats["ms_sort"], 3))
    assert sa.dtype == np.uint64 and len(sa) == len(want)
    bad = np.flatnonzero(sa != want.astype(np.uint64))
    assert len(bad) == 0, (name, "first difference at row", int(bad[0]), int(sa[bad[0]]), int(want[bad[0]]))
    assert stats["rounds"] <= si.round_bound(text)
    assert stats["active"][0] == len(want)
    act = stats["active"][: min(stats["rounds"], 16)]
    assert all(a >= b > 0 for a, b in zip(act, act[1:]))
    assert (stats["active"][1] if stats["rounds"] > 1 else 0) == si.expected_active_after_first_round(name)


@pytest.mark.parametrize("name", ["identical_40x300A", "one_5000xAC"])
def test_deep_groups_take_at_least_five_rounds_above_the_bias(sorter, name):
    _, stats = mkfmi.suffix_sort(si.case(name), device=0, wide=True, rank_bias=2**32 + 12345)
    assert 5 <= stats["rounds"] <= si.round_bound(si.case(name))


@pytest.mark.parametrize("name", ["family_30x900", "golden_db"])
def test_narrow_and_wide_agree(sorter, name):
    text = si.case(name)
    sa32, st32 = mkfmi.suffix_sort(text, device=0)
    sa64, st64 = mkfmi.suffix_sort(text, device=0, wide=True)
    assert sa32.dtype == np.uint32 and sa64.dtype == np.uint64
    assert np.array_equal(sa32.astype(np.uint64), sa64)
    assert st32["rounds"] == st64["rounds"] and st32["active"] == st64["active"]


def test_rank_bias_needs_the_wide_sort():
    with pytest.raises(ValueError):
        mkfmi.suffix_sort(si.case("iid_255"), device=0, rank_bias=5)


# ---- whole files ---------------------------------------------------------------------------------------------------------
def same_file(a, b):
    return os.path.getsize(a) == os.path.getsize(b) and filecmp.cmp(a, b, shallow=False)


def wide_env(monkeypatch):
    monkeypatch.setenv("KAIJU_MKFMI_FORCE64", "1")
    monkeypatch.setenv("KAIJU_MKFMI_DEVICE_WIDE", "1")
    monkeypatch.setenv("KAIJU_GPU_LOAD_TIMES", "1")


def test_golden_database_same_bytes_through_the_wide_sort(sorter, golden, tmp_path, monkeypatch, capfd):
    faa = os.path.join(golden.dir, "db.faa")
    host, dev, dev32 = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi"), str(tmp_path / "dev32.fmi")
    mkfmi.build_fmi(faa, host, threads=2, exponent=3)
    monkeypatch.setenv("KAIJU_MKFMI_FORCE64", "1")
    monkeypatch.setenv("KAIJU_GPU_LOAD_TIMES", "1")
    capfd.readouterr()
    mkfmi.build_fmi(faa, dev32, threads=2, exponent=3, device=0)          # FORCE64 alone: the narrow sort, widened
    err32 = capfd.readouterr().err
    assert "suffix sort" in err32 and WIDE_LINE not in err32
    monkeypatch.setenv("KAIJU_MKFMI_DEVICE_WIDE", "1")
    mkfmi.build_fmi(faa, dev, threads=2, exponent=3, device=0)
    err = capfd.readouterr().err
    assert WIDE_LINE in err and "suffix sort" in err and "rounds, active" in err, err
    assert same_file(dev, host) and same_file(dev32, host)
    assert same_file(dev, golden.fmi)


def test_synthetic_database_same_bytes_through_the_wide_sort(sorter, tmp_path, monkeypatch, capfd):
    _, leaves = synth.make_taxonomy(3, 3, 3)
    db = synth.make_db(nseq=1000, seed=2, leaves=leaves, max_len=900)
    faa = str(tmp_path / "db.faa")
    synth.write_fasta(db, faa)
    host, dev = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi")
    mkfmi.build_fmi(faa, host, threads=4, exponent=3)
    wide_env(monkeypatch)
    capfd.readouterr()
    mkfmi.build_fmi(faa, dev, threads=4, exponent=3, device=0)
    assert WIDE_LINE in capfd.readouterr().err
    assert same_file(dev, host)


def test_replicated_database_same_bytes_through_the_wide_sort(sorter, golden, tmp_path, monkeypatch, capfd):
    faa = os.path.join(golden.dir, "db.faa")
    host, dev = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi")
    mkfmi.build_fmi_replicated(faa, host, copies=3, threads=3, exponent=3, copy_taxids=[11, 222, 3333])
    wide_env(monkeypatch)
    capfd.readouterr()
    mkfmi.build_fmi_replicated(faa, dev, copies=3, threads=3, exponent=3, copy_taxids=[11, 222, 3333], device=0)
    assert WIDE_LINE in capfd.readouterr().err
    assert same_file(dev, host)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_ranks_of_40_bits_and_more_are_refused_by_the_numbers(sorter):
    """the size check alone: the text behind the pointer has one symbol and is never looked at"""
    text, sa = np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64)
    n = C.c_uint64(7)
    for tlen in (1 << 40, 1 << 41):
        assert sorter.kaiju_suffix_sort_device_wide(text.ctypes.data, tlen, 0, sa.ctypes.data, C.byref(n), None, 0) == -1, tlen      # KAIJU_GPU_ERR_ARG
        assert b"kaiju_build_fmi" in sorter.kaiju_build_fmi_error()
    text = si.case("iid_255")
    sa = np.zeros(255, dtype=np.uint64)
    assert sorter.kaiju_suffix_sort_device_wide(text.ctypes.data, len(text), 0, sa.ctypes.data, C.byref(n), None, 2**40 - 10) == -1


def test_the_narrow_refusal_names_the_wide_entry_point(sorter):
    text, sa = np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    n = C.c_uint64(7)
    assert sorter.kaiju_suffix_sort_device(text.ctypes.data, 0xf0000000, 0, sa.ctypes.data, C.byref(n), None) == -1
    msg = sorter.kaiju_build_fmi_error()
    assert b"kaiju_build_fmi" in msg and b"kaiju_suffix_sort_device_wide" in msg


def test_bad_device_id_is_refused(sorter):
    text, sa = si.case("iid_255"), np.zeros(255, dtype=np.uint64)
    n = C.c_uint64(0)
    for dev in (-1, 4096):
        assert sorter.kaiju_suffix_sort_device_wide(text.ctypes.data, len(text), dev, sa.ctypes.data, C.byref(n), None, 0) == -1


def test_text_must_end_with_a_terminator_and_hold_codes_only(sorter):
    sa, n = np.zeros(8, dtype=np.uint64), C.c_uint64(0)
    for t in (np.array([1, 2, 3], dtype=np.uint8), np.array([1, 21, 0], dtype=np.uint8)):
        assert sorter.kaiju_suffix_sort_device_wide(t.ctypes.data, len(t), 0, sa.ctypes.data, C.byref(n), None, 0) == -1


def test_device_stages_are_refused_where_the_wide_sort_is_chosen(sorter, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("KAIJU_MKFMI_DEVICE_WIDE", "1")
    out = tmp_path / "x.fmi"
    with pytest.raises(Exception, match="stages = host"):
        mkfmi.build_fmi(os.path.join(golden.dir, "db.faa"), str(out), device=0, stages="device")
    assert not os.path.exists(out)
