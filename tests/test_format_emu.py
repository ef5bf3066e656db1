"""The output lines (kaiju_amd/csrc/kj_format.h) on the host: tests/emu/format_emu.cpp drives the per-lane functions the kernels
of format.hip are made of, pass by pass, with the work units of every pass in forward, reversed and shuffled order.  For every
input of tests/format_inputs.py the bytes and kaiju_gpu_format_info must be what format_expect builds from the decisions of
kaiju_finalize_compact.  The table of the E-value gate, kaiju_gpu_format_bound, and - without a device - the answer of the three
compute entry points."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import format_expect
import format_inputs
import util
from kaiju_amd import api

LN_2, LAMBDA, LN_K = 0.6931471805, 0.3176, -2.009915479       # ConsumerThread.hpp:41-44, as in taxonomy.cpp


def build_format_emu(directory):
    so = str(directory / "libformat_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(util.ROOT, "tests", "emu", "format_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.format_emu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_double, C.c_double, C.c_int,
                             C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint32]
    L.format_emu_constants.argtypes = [C.c_void_p]
    L.format_emu_table.argtypes = [C.c_void_p, C.c_uint32]
    L.format_emu_pow_factor.restype = C.c_double
    L.format_emu_pow_factor.argtypes = [C.c_uint32]
    return L


def constants(L):
    k = np.zeros(4, dtype=np.uint32)
    L.format_emu_constants(k.ctypes.data)
    return int(k[0]), int(k[1]), int(k[3])


def golden_db_length(golden):
    with open(golden.fmi, "rb") as f:
        hdr = np.frombuffer(f.read(12), dtype=np.uint8)
    return float(int(hdr[:8].view("<i8")[0]) - int(hdr[8:12].view("<i4")[0]))      # db_length = bwtlen - nseq (Config.cpp:20)


@pytest.fixture(scope="module")
def format_emu(tmp_path_factory):
    return build_format_emu(tmp_path_factory.mktemp("format_emu"))


@pytest.fixture(scope="module")
def inputs(format_emu, golden):
    B, S, K = constants(format_emu)
    return format_inputs.cases(B, S, K, golden_db_length(golden))


def db_of(case, golden):
    return golden_db_length(golden) if case["db"] == "golden" else case["db"]


def library_table(K):
    """the table the library gives its contexts (the compiler of kaiju_finalize_compact made it)"""
    pw = np.full(K, -1.0)
    assert api.lib().kaiju_gpu_format_evalue_table(pw.ctypes.data, K) == 0
    return pw


def run_emu(L, case, db_length, out_cap, order, seed=1, slack=37):
    """the emulation, with the library's table, on a buffer of out_cap + slack bytes of 0xA5; returns (buffer, info)"""
    pw = library_table(constants(L)[2])
    out = np.full(out_cap + slack, 0xA5, dtype=np.uint8)
    info = np.zeros(1, dtype=format_expect.FORMAT_INFO_DTYPE)
    text = np.frombuffer(case["text1"] + b"\0", dtype=np.uint8)
    rc = L.format_emu(pw.ctypes.data, case["recs"].ctypes.data, case["off"].ctypes.data, len(case["recs"]), 1 if case["paired"] else 0, text.ctypes.data,
                      len(case["text1"]), case["names"].ctypes.data, db_length, case["min_evalue"], 1 if case["mode"] == "greedy" else 0,
                      1 if case["protein"] else 0, out.ctypes.data, out_cap, info.ctypes.data, order, seed)
    assert rc == 0
    return out, info[0]


def compare(out, info, want, what):
    for f in format_expect.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def test_both_outcomes_in_every_gate_group(inputs, golden):
    """from the reference alone: every group of the gate cases holds lines the gate lets pass and lines it stops, and the
    same records in MEM mode ignore it"""
    seen = 0
    for case in inputs:
        if not case["id"].startswith(("gate_", "nogate_")):
            continue
        res = format_expect.expected(case, db_of(case, golden))["res"]["classified"]
        if case["id"].startswith("gate_"):
            assert res.any() and not res.all(), case["id"]
            # (per pair of lengths: the score below the flip is stopped, the flip and its upper neighbour pass, 1 is stopped, the rest pass)
            assert res.reshape(-1, 8).tolist() == [[0, 1, 1, 0, 1, 1, 1, 1]] * (len(res) // 8), case["id"]
            seen += 1
        else:
            assert res.all(), case["id"]
    assert seen == 12


def test_every_input_in_every_order(format_emu, inputs, golden):
    for case in inputs:
        want = format_expect.expected(case, db_of(case, golden))
        for order in (0, 1, 2):
            out, info = run_emu(format_emu, case, db_of(case, golden), len(want["text"]) + 5, order, seed=3 + order)
            compare(out, info, want, (case["id"], order))


def test_capacity(format_emu, inputs, golden):
    jobs = format_inputs.capacity_cases(inputs, lambda k: format_expect.expected(k, db_of(k, golden)))
    assert len(jobs) == 20
    for case, cap in jobs:
        want = format_expect.expected(case, db_of(case, golden), cap)
        assert want["info"]["overflow"] == (1 if cap < len(want["text"]) else 0) and want["info"]["text_bytes"] == len(want["text"])
        assert want["written"] == want["text"][: len(want["written"])] and (not want["written"] or want["written"].endswith(b"\n"))
        for order in (0, 2):
            out, info = run_emu(format_emu, case, db_of(case, golden), cap, order)
            compare(out, info, want, (case["id"], cap, order))


def test_table_of_the_evalue_gate(format_emu):
    """K is large enough by the rule of kj_format.h, every entry is the host expression - in the emulation's build and in the
    library's own"""
    _, _, K = constants(format_emu)
    want = np.asarray([math.pow(2, -1 * ((LAMBDA * b - LN_K) / LN_2)) for b in range(K)])
    pw = np.full(K, -1.0)
    assert format_emu.format_emu_table(pw.ctypes.data, K) == 1
    assert pw.tobytes() == want.tobytes()
    first_zero = int(np.argmax(pw == 0.0))
    assert 2000 < first_zero < K and np.all(pw[first_zero:] == 0.0) and not np.signbit(pw[first_zero:]).any() and np.all(pw[:first_zero] > 0)
    for b in (K, K + 1, 2 ** 31, 2 ** 32 - 1):
        f = format_emu.format_emu_pow_factor(b)
        assert f == 0.0 and not np.signbit(f)
    # a table that ends where the factor is still positive must be refused
    assert format_emu.format_emu_table(pw.ctypes.data, first_zero - 1) == 0
    # the library's table, entry by entry, against the library's own kaiju_finalize_compact: with db_length 1 and a protein
    # read of one letter the E-value IS the factor, so a record passes with min_evalue = entry and is stopped just below it
    lib_pw = library_table(K)
    assert np.all(lib_pw[first_zero + 1:] == 0.0) and not np.signbit(lib_pw).any() and np.all(np.diff(lib_pw) <= 0)
    recs = np.zeros(1, dtype=api.COMPACT_DTYPE)
    off = np.asarray([0, 1, 1], dtype=np.uint64)
    for b in range(1, K):
        recs[0] = (5, b, 1)
        for me, want_c in ((lib_pw[b], 1), (np.nextafter(lib_pw[b], -1.0), 0)):
            p = api.default_params("greedy", min_evalue=float(me), input_is_protein=1)
            assert int(format_expect.finalize(p, 1.0, recs, off, False)[0]["classified"]) == want_c, (b, me)


def test_format_bound():
    L = api.lib()
    for b, n in ((0, 0), (5, 1), (1000, 17), (2 ** 32 - 33, 2 ** 31 - 17)):
        assert L.kaiju_gpu_format_bound(b, n) == b + 24 * n
    # the longest line there is: a name, "C\t", "\t", twenty digits, "\n"
    assert len(b"C\t" + b"\t" + str(2 ** 64 - 1).encode() + b"\n") == 24


def test_entry_points_exist_and_need_a_device():
    L = api.lib()
    for sym in ("kaiju_gpu_format_compact", "kaiju_gpu_format_compact_device", "kaiju_gpu_classify_text_to_text", "kaiju_gpu_format_bound"):
        assert hasattr(L, sym), sym
    if api.device_count() > 0:
        return            # (a HIP device is visible: the answer without one cannot be seen here)
    info = np.zeros(1, dtype=format_expect.FORMAT_INFO_DTYPE)
    pinfo = np.zeros(1, dtype=api.PARSE_INFO_DTYPE)
    buf = np.zeros(64, dtype=np.uint64)
    assert L.kaiju_gpu_format_compact(None, buf.ctypes.data, buf.ctypes.data, 1, 0, b"@r\n", 3, buf.ctypes.data, buf.ctypes.data, 64, info.ctypes.data) == -4
    assert L.kaiju_gpu_format_compact_device(None, None, None, 0, 0, None, 0, None, None, 0, None, None) == -4
    assert L.kaiju_gpu_classify_text_to_text(None, None, b"@r\nA\n", 5, None, 0, 1, 0, 4, buf.ctypes.data, 64, pinfo.ctypes.data, info.ctypes.data) == -4
