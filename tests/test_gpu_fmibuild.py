"""The stages behind the suffix sort on the device (kaiju_amd/csrc/fmibuild.hip, kj_fmibuild.h; libkaiju_mkfmi_gpu.so):
fmi_arrays(text, device=0) against the numpy expectation of tests/fmibuild_expect.py, array by array, on every case of the host
emulation's test; whole .fmi files built with stages="device" against the host builder's, byte for byte; a second build of the
same input in one process; the refusals, which leave no file behind."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import fmibuild_expect as fe
from kaiju_amd import mkfmi, synth

pytestmark = pytest.mark.gpu

ALL_STAGES = 31                   # KAIJU_FMI_STAGE_BWT | RANKS | SAMPLES | CHECKPOINTS | RECODE


@pytest.fixture(scope="module")
def builder(gpu_lib):
    return mkfmi._lib_gpu()


# ---- arrays ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,copies,exponent", fe.CASES, ids=fe.CASE_IDS)
def test_device_arrays_are_the_expectation(builder, name, copies, exponent):
    want = fe.expected(name, copies, exponent)
    got, stats = mkfmi.fmi_arrays(fe.text(name), copies=copies, exponent=exponent, device=0)
    print(name, copies, exponent, "rows", want["bwtlen"], {k: round(v, 3) for k, v in stats.items() if k.startswith("ms_")}, "bytes", stats["device_bytes"])
    d = fe.first_difference(got, want)
    assert d is None, (name, copies, exponent, "first difference (array, index, got, want):", d)
    assert stats["device_stages"] == ALL_STAGES and stats["stages"] == ["bwt", "ranks", "samples", "checkpoints", "recode"]
    assert stats["device_bytes"] > 0
    assert (stats["sort"]["rounds"] == 0) == (want["nseq"] * copies == want["bwtlen"])       # no round without a suffix


@pytest.mark.parametrize("name,copies,exponent", [("golden_db", 1, 3), ("iid_4097", 17, 3), ("identical_40x300A", 1, 3), ("terminators_only", 1, 3)])
def test_device_arrays_without_the_coding(builder, name, copies, exponent):
    """a wrong BWT told from a wrong coding: the raw letters"""
    want = fe.expected(name, copies, exponent)
    got, stats = mkfmi.fmi_arrays(fe.text(name), copies=copies, exponent=exponent, device=0, recode=False)
    d = fe.first_difference(got, want, recode=False)
    assert d is None, (name, "first difference (array, index, got, want):", d)
    assert stats["device_stages"] == ALL_STAGES - 16


def test_history_does_not_matter(builder):
    """A, B, A on one process: the second A is the first"""
    a = ("iid_4097", 17, 3)
    b = ("identical_40x300A", 3, 2)
    first, _ = mkfmi.fmi_arrays(fe.text(a[0]), copies=a[1], exponent=a[2], device=0)
    other, _ = mkfmi.fmi_arrays(fe.text(b[0]), copies=b[1], exponent=b[2], device=0)
    again, _ = mkfmi.fmi_arrays(fe.text(a[0]), copies=a[1], exponent=a[2], device=0)
    assert fe.first_difference(other, fe.expected(*b)) is None
    for k in fe.ARRAYS:
        assert np.array_equal(first[k], again[k]), k
    assert fe.first_difference(again, fe.expected(*a)) is None


# ---- whole files ---------------------------------------------------------------------------------------------------------
def same_file(a, b):
    return os.path.getsize(a) == os.path.getsize(b) and filecmp.cmp(a, b, shallow=False)


def test_golden_database_same_bytes(builder, golden, tmp_path):
    faa = os.path.join(golden.dir, "db.faa")
    host, dev = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi")
    mkfmi.build_fmi(faa, host, threads=2, exponent=3)
    mkfmi.build_fmi(faa, dev, threads=2, exponent=3, device=0, stages="device")
    assert same_file(dev, host)
    assert same_file(dev, golden.fmi)


@pytest.mark.parametrize("nseq,seed,exponent,threads", [(257, 1, 3, 1), (1000, 2, 3, 4), (1531, 3, 5, 3), (64, 4, 2, 8)])
def test_synthetic_databases_same_bytes(builder, tmp_path, nseq, seed, exponent, threads):
    _, leaves = synth.make_taxonomy(3, 3, 3)
    db = synth.make_db(nseq=nseq, seed=seed, leaves=leaves, max_len=900)
    faa = str(tmp_path / "db.faa")
    synth.write_fasta(db, faa)
    host, dev = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi")
    mkfmi.build_fmi(faa, host, threads=threads, exponent=exponent)
    mkfmi.build_fmi(faa, dev, threads=threads, exponent=exponent, device=0, stages="device")
    assert same_file(dev, host)


def test_replicated_database_same_bytes(builder, golden, tmp_path):
    faa = os.path.join(golden.dir, "db.faa")
    host, dev = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi")
    mkfmi.build_fmi_replicated(faa, host, copies=3, threads=3, exponent=3, copy_taxids=[11, 222, 3333])
    mkfmi.build_fmi_replicated(faa, dev, copies=3, threads=3, exponent=3, copy_taxids=[11, 222, 3333], device=0, stages="device")
    assert same_file(dev, host)


def test_forced_64_bit_builder_takes_the_device_arrays(builder, golden, tmp_path, monkeypatch):
    faa = os.path.join(golden.dir, "db.faa")
    host, dev = str(tmp_path / "host.fmi"), str(tmp_path / "dev.fmi")
    mkfmi.build_fmi(faa, host, threads=3, exponent=3)
    monkeypatch.setenv("KAIJU_MKFMI_FORCE64", "1")
    mkfmi.build_fmi(faa, dev, threads=3, exponent=3, device=0, stages="device")
    assert same_file(dev, host)


def test_stats_of_a_whole_build(builder, golden, tmp_path):
    faa = os.path.join(golden.dir, "db.faa").encode()
    for stages, mask in ((1, ALL_STAGES), (0, 0)):
        st = mkfmi.FmiBuildStats()
        out = str(tmp_path / f"s{stages}.fmi")
        assert builder.kaiju_build_fmi_device_ex(faa, out.encode(), 2, 3, 1, None, 0, 0, stages, C.byref(st)) == 0
        assert st.device_stages == mask and st.sort.rounds >= 1 and same_file(out, golden.fmi)
        assert (st.device_bytes > 0) == (stages == 1)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_unknown_stages_value_is_refused(builder, golden, tmp_path):
    faa, out = os.path.join(golden.dir, "db.faa").encode(), tmp_path / "x.fmi"
    for stages in (2, -1, 31):
        assert builder.kaiju_build_fmi_device_ex(faa, str(out).encode(), 1, 3, 1, None, 0, 0, stages, None) == -1      # KAIJU_GPU_ERR_ARG
        assert b"stages" in builder.kaiju_build_fmi_error()
        assert not out.exists()


def test_bad_device_id_is_refused(builder, golden, tmp_path):
    faa, out = os.path.join(golden.dir, "db.faa").encode(), tmp_path / "x.fmi"
    text = np.ascontiguousarray(fe.text("iid_255"))
    a = mkfmi.FmiArrays()
    for dev in (-1, 4096):
        assert builder.kaiju_build_fmi_device_ex(faa, str(out).encode(), 1, 3, 1, None, 0, dev, 1, None) == -1
        assert not out.exists()
        assert builder.kaiju_fmi_arrays_device(text.ctypes.data, len(text), 1, 3, dev, 1, C.byref(a), None) == -1
    with pytest.raises(Exception, match="device_id"):
        mkfmi.build_fmi(faa.decode(), str(tmp_path / "y.fmi"), device=4096, stages="device")
    assert not (tmp_path / "y.fmi").exists()


def test_rows_beyond_the_device_memory_are_refused_by_the_size_check(builder, tmp_path):
    """one sequence of 4 096 letters, 2^31 - 2 copies: about 8.8 T rows.  The size check answers before anything is allocated."""
    faa, out = tmp_path / "one.faa", tmp_path / "one.fmi"
    rng = np.random.default_rng(5)
    faa.write_text(">s_1\n" + "".join("ACDEFGHIKLMNPQRSTVWY"[i] for i in rng.integers(0, 20, size=4096)) + "\n")
    st = mkfmi.FmiBuildStats()
    rc = builder.kaiju_build_fmi_device_ex(str(faa).encode(), str(out).encode(), 1, 3, 2**31 - 2, None, 0, 0, 1, C.byref(st))
    msg = builder.kaiju_build_fmi_error()
    print(rc, msg)
    assert rc == -6                                               # KAIJU_GPU_ERR_NOMEM
    assert b"stages = host" in msg and b"MiB" in msg
    assert st.device_bytes > 8 << 40 and st.device_stages == 0
    assert not out.exists()
