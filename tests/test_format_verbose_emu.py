"""The lines of kaiju -v (kaiju_amd/csrc/kj_format_verbose.h) on the host: tests/emu/format_verbose_emu.cpp drives the per-lane and
per-team functions the kernels of format_verbose.hip are made of, pass by pass, with the work units of every pass - the lanes
of a team among them - in forward, reversed and shuffled order.  For every input of tests/format_verbose_inputs.py the bytes and
kaiju_gpu_format_verbose_info must be what format_verbose_expect builds from the rules.  kaiju_accession_ranks against Python,
and - without a device - the answer of the new entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import format_verbose_expect as fve
import format_verbose_inputs as fvi
import index_truth
import util
from kaiju_amd import api

INDEX_DB = 54321.0           # db_length of the index the emulated contexts have (any number serves)


def build_format_verbose_emu(directory):
    so = str(directory / "libformat_verbose_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, os.path.join(util.ROOT, "tests", "emu", "format_verbose_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.format_verbose_emu.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32]
    L.format_verbose_emu_constants.argtypes = [C.c_void_p]
    return L


def constants(L):
    k = np.zeros(5, dtype=np.uint32)
    L.format_verbose_emu_constants(k.ctypes.data)
    return int(k[0]), int(k[1]), int(k[3])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_format_verbose_emu(tmp_path_factory.mktemp("format_verbose_emu"))


@pytest.fixture(scope="module")
def inputs(emu):
    B, S, K = constants(emu)
    return fvi.cases(B, S, K, INDEX_DB)


@pytest.fixture(scope="module")
def table():
    return fvi.accession_table()


@pytest.fixture(scope="module")
def want_of(inputs):
    """format_verbose_expect.expected of a case without a capacity, computed once"""
    memo = {}

    def get(case):
        if case["id"] not in memo:
            memo[case["id"]] = fve.expected(case, INDEX_DB)
        return memo[case["id"]]
    return get


def device_arrays(case):
    """the arrays of the device form from the kaiju_gpu_verbose records"""
    v = case["v"]
    return (np.ascontiguousarray(v["n_acc"]), np.ascontiguousarray(v["acc_iseq"]).reshape(-1), np.ascontiguousarray(v["text_len"]),
            np.ascontiguousarray(v["truncated"]))


def run_emu(L, case, table, out_cap, order, seed=1, slack=37):
    """the emulation, with the library's table of the E-value gate, on a buffer of out_cap + slack bytes of 0xA5"""
    K = constants(L)[2]
    pw = np.full(K, -1.0)
    assert api.lib().kaiju_gpu_format_evalue_table(pw.ctypes.data, K) == 0
    rank, plen, aoff, blob = table
    out = np.full(out_cap + slack, 0xA5, dtype=np.uint8)
    info = np.zeros(1, dtype=api.FORMAT_VERBOSE_INFO_DTYPE)
    text = np.frombuffer(case["text1"] + b"\0", dtype=np.uint8)
    pep = np.frombuffer(case["pep"] + b"\0", dtype=np.uint8)
    blob_a = np.frombuffer(blob + b"\0", dtype=np.uint8)
    nacc, acc, tlen, trunc = device_arrays(case)
    ptr = lambda x: x.ctypes.data
    a = np.asarray([ptr(pw), ptr(case["hits"]), ptr(case["recs"]), ptr(case["off"]), len(case["recs"]), 1 if case["paired"] else 0, ptr(nacc), ptr(acc),
                    ptr(case["text_pos"]), ptr(tlen), ptr(trunc), ptr(pep), case["text_cap"], ptr(text), len(case["text1"]), ptr(case["names"]),
                    ptr(blob_a), ptr(aoff), ptr(plen), ptr(rank), len(rank), ptr(out), out_cap, ptr(info), 1 if case["mode"] == "greedy" else 0,
                    1 if case["protein"] else 0], dtype=np.uint64)
    d = np.asarray([INDEX_DB, case["min_evalue"]])
    assert L.format_verbose_emu(a.ctypes.data, d.ctypes.data, order, seed) == 0
    return out, info[0]


def compare(out, info, want, what):
    for f in fve.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def test_the_inputs_hold_what_they_claim(inputs, want_of):
    """from the reference alone: both outcomes of the gate, truncated and inexact records, every alignment of the copied
    segments"""
    by_id = {k["id"]: k for k in inputs}
    assert [len(by_id["n_%d" % n]["recs"]) for n in fvi.RECORD_COUNTS] == list(fvi.RECORD_COUNTS)
    gates = [k for k in inputs if k["id"].startswith("gate_")]
    assert len(gates) == 6 and {(k["paired"], k["protein"]) for k in gates} == {(False, False), (True, False), (False, True)}
    for k in gates:
        res = want_of(k)["res"]["classified"]
        assert res.any() and not res.all(), k["id"]
        assert want_of(by_id["no" + k["id"]])["res"]["classified"].all()
    assert want_of(by_id["texts"])["info"]["n_truncated"] == 2 and want_of(by_id["taxon_ids"])["info"]["n_inexact"] == 2
    big = want_of(by_id["n_65537"])["info"]
    assert 0 < big["n_classified"] < 0.05 * big["n_records"]
    # the grid: source and destination alignment of names and peptides; the middle at every alignment of its place
    g, w = by_id["alignment_grid"], want_of(by_id["alignment_grid"])
    assert w["res"]["classified"].all()
    seen_n, seen_p, seen_m = set(), set(), set()
    for r in range(len(g["recs"])):
        lo, nl, tl = int(w["line_off"][r]), int(g["names"][r]["len"]), int(g["v"][r]["text_len"])
        seen_n.add((int(g["names"][r]["pos"]) % 16, (lo + 2) % 16))
        seen_p.add((int(g["text_pos"][r]) % 16, (int(w["line_off"][r + 1]) - 1 - tl) % 16))
        seen_m.add((lo + 3 + nl) % 16)
    assert len(seen_n) == 256 and len(seen_p) == 256 and len(seen_m) == 16


def test_every_input_in_every_order(emu, inputs, table, want_of):
    for case in inputs:
        want = want_of(case)
        for order in (0, 1, 2):
            out, info = run_emu(emu, case, table, len(want["text"]) + 5, order, seed=3 + order)
            compare(out, info, want, (case["id"], order))


def test_capacity(emu, inputs, table, want_of):
    jobs = fvi.capacity_cases(inputs, want_of)
    assert len(jobs) == 36
    for case, cap in jobs:
        want = fve.expected(case, INDEX_DB, cap)
        assert want["info"]["overflow"] == (1 if cap < len(want["text"]) else 0) and want["info"]["text_bytes"] == len(want["text"])
        assert want["written"] == want["text"][: len(want["written"])] and (not want["written"] or want["written"].endswith(b"\n"))
        for order in (0, 2):
            out, info = run_emu(emu, case, table, cap, order)
            compare(out, info, want, (case["id"], cap, order))


def python_ranks(names):
    pre = [fve.prefix(nm) for nm in names]
    order = {p: k for k, p in enumerate(sorted({p for p in pre if p is not None}))}
    return ([order[p] if p is not None else 0xffffffff for p in pre], [len(p) if p is not None else 0 for p in pre])


def library_ranks(names):
    n = len(names)
    arr = (C.c_char_p * n)(*names)
    rank, plen = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    assert api.lib().kaiju_accession_ranks(arr, n, rank.ctypes.data, plen.ctypes.data) == 0
    return rank.tolist(), plen.tolist()


def test_accession_ranks(golden):
    assert library_ranks(fvi.DB_NAMES) == python_ranks(fvi.DB_NAMES)
    r, l = library_ranks(fvi.DB_NAMES)
    assert r[fvi.I_NONE] == 0xffffffff and r[fvi.I_LEAD] == 0 and l[fvi.I_LEAD] == 0 and r[fvi.I_SAME_A] == r[fvi.I_SAME_B]
    assert r[fvi.I_AB] < r[fvi.I_ABDOT] < r[fvi.I_ABC] and l[fvi.I_LONG] == 300 and l[fvi.I_MANY] == len(b"WP_000123.1")
    assert max(x for x in r if x != 0xffffffff) == r[fvi.I_HIGH] > r[fvi.I_ZZ]       # bytes compare as unsigned: 0xc3 behind 'Z'
    names = [nm.encode() for nm in index_truth.read_fasta_records(os.path.join(golden.dir, "db.faa"))[0]]
    assert len(names) > 20 and library_ranks(names) == python_ranks(names)
    assert library_ranks([]) == ([], [])


def test_entry_points_exist_and_need_a_device():
    L = api.lib()
    for sym in ("kaiju_gpu_index_upload_accessions", "kaiju_gpu_format_verbose", "kaiju_gpu_format_verbose_device", "kaiju_gpu_classify_batch_verbose_text",
                "kaiju_accession_ranks"):
        assert hasattr(L, sym), sym
    if api.device_count() > 0:
        return            # (a HIP device is visible: the answer without one cannot be seen here)
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    text, nbytes = C.c_void_p(), C.c_uint64()
    assert L.kaiju_gpu_index_upload_accessions(None) == -4
    assert L.kaiju_gpu_format_verbose(None, p, p, p, p, 0, 10, p, p, 1, 0, b"r", 1, p, p, 64, p) == -4
    assert L.kaiju_gpu_format_verbose_device(None, None, None, None, 0, 0, None, None, None, None, None, 0, None, 0, None, None, 0, None, None) == -4
    assert L.kaiju_gpu_classify_batch_verbose_text(None, None, b"ACGT", p, 1, 0, b"r", 1, p, C.byref(text), C.byref(nbytes), p) == -4
