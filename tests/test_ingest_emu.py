"""Record extraction (kaiju_amd/csrc/kj_ingest.h) on the host: tests/emu/ingest_emu.cpp drives the per-lane functions the
kernels of ingest.hip are made of, pass by pass and tile by tile, with the tiles of every pass in forward, reversed and
shuffled order.  For every input of tests/ingest_inputs.py seqs, off, the name spans and the info fields must be what the
reading loop of the command line programs gives (ingest_expect.ref_spans, itself compared with test_cli_ingest.ref_records
here), pairs interleaved as parse_blocks does.  Without a device the three entry points must exist and say so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ingest_expect
import ingest_inputs
import util
from test_cli_ingest import ref_records

INFO_FIELDS = ("n_records", "n_records2", "max_mate_len", "name_mismatch", "seq_bytes", "overflow")


def build_ingest_emu(directory):
    so = str(directory / "libingest_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(util.ROOT, "tests", "emu", "ingest_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.ingest_emu.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_int, C.c_uint32]
    L.ingest_emu_constants.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope="module")
def ingest_emu(tmp_path_factory):
    return build_ingest_emu(tmp_path_factory.mktemp("ingest_emu"))


def constants(L):
    k = np.zeros(4, dtype=np.uint32)
    L.ingest_emu_constants(k.ctypes.data)
    return int(k[0]), int(k[1])


def run_emu(L, text1, text2, fastq, keep, rec_cap, order, seed=1):
    t1 = np.frombuffer(text1 + b"\0", dtype=np.uint8)
    t2 = np.frombuffer((text2 or b"") + b"\0", dtype=np.uint8)
    seqs = np.zeros(len(t1) + len(t2), dtype=np.uint8)
    off = np.full(2 * rec_cap + 1, 0xdead, dtype=np.uint64)
    names = np.full((rec_cap + 1, 2), 0xdead, dtype=np.uint32)
    info = np.zeros(1, dtype=ingest_expect_info_dtype())
    rc = L.ingest_emu(t1.ctypes.data, len(text1), t2.ctypes.data, len(text2 or b""), 1 if text2 is not None else 0, 1 if fastq else 0,
                      1 if keep else 0, rec_cap, seqs.ctypes.data, off.ctypes.data, names.ctypes.data, info.ctypes.data, order, seed)
    assert rc == 0
    return seqs, off, names, info[0]


def ingest_expect_info_dtype():
    return np.dtype([("n_records", "<u4"), ("n_records2", "<u4"), ("max_mate_len", "<u4"), ("name_mismatch", "<u4"),
                     ("seq_bytes", "<u8"), ("overflow", "<u4"), ("reserved", "<u4")])


def compare(got, want, what):
    seqs, off, names, info = got
    n = len(want["off"]) // 2
    for f in INFO_FIELDS:
        assert int(info[f]) == int(want[f]), (what, f, int(info[f]), want[f])
    assert np.array_equal(off[: 2 * n + 1], want["off"]), (what, "off")
    assert bytes(seqs[: want["seq_bytes"]]) == bytes(want["seqs"]), (what, "seqs")
    assert np.array_equal(names[:n], want["names"]), (what, "names")


def test_expectation_is_the_reading_loop():
    """ingest_expect.ref_spans (format and keep_names as arguments, positions) gives the names and sequences of
    test_cli_ingest.ref_records wherever that one detects the same format"""
    for name, fastq, keep, t1, t2 in ingest_inputs.cases(4096, 256):
        for t in (t1, t2):
            first = [l for l in (t or b"").split(b"\n") if l]
            if t is None or keep or (first and (first[0][:1] == b"@") != fastq):
                continue
            assert [(t[p:p + l], s) for p, l, s in ingest_expect.ref_spans(t, fastq)] == ref_records(t), name


def test_every_input_in_every_tile_order(ingest_emu):
    T, S = constants(ingest_emu)
    assert T % 16 == 0 and S >= 2
    for name, fastq, keep, t1, t2 in ingest_inputs.cases(T, S):
        want = ingest_expect.expected(t1, t2, fastq, keep)
        cap = max(want["n_records"], want["n_records2"]) + 2
        for order in (0, 1, 2):
            compare(run_emu(ingest_emu, t1, t2, fastq, keep, cap, order, seed=7 + order), want, (name, order))


def test_capacity_one_below_the_record_count(ingest_emu):
    T, S = constants(ingest_emu)
    for name, fastq, keep, t1, t2 in ingest_inputs.cases(T, S):
        if name not in ("fuzz_fastq_crlf_blanks", "fuzz_fasta", "pair_equal", "fa_header_only", "fq_cut_after_header"):
            continue
        full = ingest_expect.expected(t1, t2, fastq, keep)
        cap = len(full["off"]) // 2 - 1
        want = ingest_expect.expected(t1, t2, fastq, keep, rec_cap=cap)
        assert want["overflow"] == 1
        got = run_emu(ingest_emu, t1, t2, fastq, keep, cap, 2)
        compare(got, want, name)
        assert np.all(got[2][cap:] == 0xdead) and np.all(got[1][2 * cap + 1:] == 0xdead), name


def test_entry_points_exist_and_need_a_device():
    from kaiju_amd import api
    L = api.lib()
    for sym in ("kaiju_gpu_parse_block", "kaiju_gpu_parse_block_device", "kaiju_gpu_classify_text_compact"):
        assert hasattr(L, sym), sym
    if api.device_count() > 0:
        pytest.skip("a HIP device is visible: the answer without one cannot be seen here")
    info = np.zeros(1, dtype=api.PARSE_INFO_DTYPE)
    buf = np.zeros(64, dtype=np.uint64)
    assert L.kaiju_gpu_parse_block(None, b"@r\nA\n", 5, None, 0, 1, 0, 4, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, info.ctypes.data) == -4
    assert L.kaiju_gpu_parse_block_device(None, None, 0, None, 0, 1, 0, 4, None, None, None, None, None) == -4
    assert L.kaiju_gpu_classify_text_compact(None, None, b"@r\nA\n", 5, None, 0, 1, 0, 4, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                             info.ctypes.data) == -4
