"""The lines of kaijux / kaijup (kaiju_amd/csrc/kj_format_seq.h) on the host: tests/emu/format_seq_emu.cpp drives the per-lane and
per-team functions the kernels of format_seq.hip are made of, pass by pass, with the work units of every pass - the lanes of a
team and of every step of the fragment scan among them - in forward, reversed and shuffled order.  For every input of
tests/format_seq_inputs.py the bytes and kaiju_gpu_format_verbose_info must be what format_seq_expect builds from the rules.
The same source as a program of its own, built with the address and undefined-behaviour sanitizers (their runtimes linked
statically), runs a dump of all of them and must stay clean.  And - without a device - the answer of the new entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import format_seq_expect as fse
import format_seq_inputs as fsi
import util
from kaiju_amd import api

INDEX_DB = 54321.0           # db_length of the index the emulated contexts have (any number serves)
EMU_SRC = os.path.join(util.ROOT, "tests", "emu", "format_seq_emu.cpp")


def build_format_seq_emu(directory):
    so = str(directory / "libformat_seq_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, EMU_SRC], check=True)
    L = C.CDLL(so)
    L.format_seq_emu.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32]
    L.format_seq_emu_constants.argtypes = [C.c_void_p]
    return L


def constants(L):
    k = np.zeros(6, dtype=np.uint32)
    L.format_seq_emu_constants(k.ctypes.data)
    return int(k[0]), int(k[1]), int(k[3])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_format_seq_emu(tmp_path_factory.mktemp("format_seq_emu"))


@pytest.fixture(scope="module")
def inputs(emu):
    B, S, K = constants(emu)
    return fsi.cases(B, S, K, INDEX_DB)


def db_of(case):
    return INDEX_DB if case["db"] == "golden" else case["db"]


@pytest.fixture(scope="module")
def want_of(inputs):
    """format_seq_expect.expected of a case without a capacity, computed once"""
    memo = {}

    def get(case):
        if case["id"] not in memo:
            memo[case["id"]] = fse.expected(case, db_of(case))
        return memo[case["id"]]
    return get


def device_arrays(case):
    """the arrays of the device form from the kaiju_gpu_verbose records"""
    v = case["v"]
    return np.ascontiguousarray(v["text_len"]), np.ascontiguousarray(v["truncated"])


def run_emu(L, case, out_cap, order, seed=1, slack=37):
    """the emulation, with the library's table of the E-value gate, on a buffer of out_cap + slack bytes of 0xA5"""
    K = constants(L)[2]
    pw = np.full(K, -1.0)
    assert api.lib().kaiju_gpu_format_evalue_table(pw.ctypes.data, K) == 0
    slen, soff, blob = fsi.name_table()
    out = np.full(out_cap + slack, 0xA5, dtype=np.uint8)
    info = np.zeros(1, dtype=api.FORMAT_VERBOSE_INFO_DTYPE)
    text = np.frombuffer(case["text1"] + b"\0", dtype=np.uint8)
    pep = np.frombuffer((case["pep"] or b"") + b"\0", dtype=np.uint8)
    seqs = np.frombuffer(case["seqs"] + b"\0", dtype=np.uint8)
    blob_a = np.frombuffer(blob + b"\0", dtype=np.uint8)
    tlen, trunc = device_arrays(case)
    ptr = lambda x: x.ctypes.data
    greedy = 1 if case["mode"] == "greedy" else 0
    a = np.asarray([ptr(pw), ptr(case["hits"]), ptr(case["off"]), len(case["hits"]), 1 if case["paired"] else 0, ptr(seqs), ptr(case["text_pos"]), ptr(tlen),
                    ptr(trunc), 0 if case["pep"] is None else ptr(pep), case["text_cap"], ptr(text), len(case["text1"]), ptr(case["names"]), ptr(blob_a),
                    ptr(soff), ptr(slen), len(slen), ptr(out), out_cap, ptr(info), greedy, 1 if case["protein"] else 0, case["u_rule"], case["min_frag"],
                    case["min_score"], greedy], dtype=np.uint64)
    d = np.asarray([db_of(case), case["min_evalue"]])
    assert L.format_seq_emu(a.ctypes.data, d.ctypes.data, order, seed) == 0
    return out, info[0]


def compare(out, info, want, what):
    for f in fse.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def test_the_inputs_hold_what_they_claim(emu, inputs, want_of):
    """from the rules alone: every kind of line, both outcomes of the gate, the fragments of the kaijup rule, truncated and inexact
    records, every alignment of the copied segments"""
    by_id = {k["id"]: k for k in inputs}
    counts = fsi.RECORD_COUNTS + (fsi.BIG_COUNT,)
    assert [len(by_id["n_%d" % n]["hits"]) for n in counts] == list(counts) and fsi.BIG_COUNT > constants(emu)[1] ** 2
    big = want_of(by_id["n_%d" % fsi.BIG_COUNT])["info"]
    assert 0 < big["n_records"] - big["n_classified"] < big["n_classified"]
    assert sorted(len(nm) for nm in fsi.DB_NAMES[:6]) == list(fsi.TABLE_NAME_LENGTHS) and all(c in fsi.DB_NAMES[fsi.I_ODD] for c in b"_,\t")
    for n in (65, 257):
        t = want_of(by_id["n_%d" % n])["text"]
        assert b"\nC\t" in t and b"\t0\n" in t and any(l.startswith(b"U") and l.count(b"\t") == 1 for l in t.split(b"\n"))
    gates = [k for k in inputs if k["id"].startswith("gate_")]
    assert len(gates) == 12 and {(k["paired"], k["protein"]) for k in gates} == {(False, False), (True, False), (False, True)}
    assert {k["db"] for k in gates} == {"golden", 1e12}
    for k in gates:
        w = want_of(k)
        res = w["res"]["classified"]
        assert res.any() and not res.all(), k["id"]
        assert want_of(by_id["no" + k["id"]])["res"]["classified"].all()
        if not k["protein"]:
            # a record with ids that the gate rejects is long enough: "U\tname\n", never "\t0"
            assert all(l == b"U\tg%d\n" % r for r, l in enumerate(w["lines"]) if not res[r])
    # without a peptide column every 'C' line ends ",\t\n" (or "\t\t\n": no id is impossible on a 'C' line)
    plain = want_of(by_id["ids_plain"])
    assert all(l.endswith(b",\t\n") for l in plain["lines"] if l.startswith(b"C")) and plain["info"]["n_classified"] == len(plain["lines"]) - 1
    assert b"C\tequal\t20\tL,L,L17_abcdefghijklm,L17_abcdefghijklm,L17_abcdefghijklm,\t\n" in plain["lines"]
    assert b"C\tno_seq\t20\tL15_abcdefghijk,,,,\t\n" in plain["lines"] and b"C\tempty_only\t20\t,\t\n" in plain["lines"]
    over = [l for l in plain["lines"] if l.startswith(b"C\tover\t")][0]
    assert over.count(b",") == 21 + 1                        # (21 names, and the comma inside the odd name)
    assert want_of(by_id["texts"])["info"]["n_truncated"] == 2 and want_of(by_id["names_best"])["info"]["n_inexact"] == 2
    assert b"U\tbest0\n" in want_of(by_id["names_best"])["lines"] and b"C\tbest4294967295\t4294967295\tQ00.1_100,\t\n" in want_of(by_id["names_best"])["lines"]
    past = want_of(by_id["names_past_end"])["lines"]
    assert past[1] == b"U\t\n" and past[2].startswith(b"C\tlast_name\t")
    for l in (13, 14, 15):
        assert len(b"C\t" + b"n" * l + b"\t") == l + 3 and want_of(by_id["first_name_%d" % l])["lines"][0].startswith(b"C\t" + b"n" * l + b"\t7\t")
    # the nucleotide rule
    m3 = 3 * fsi.M
    for pe in (False, True):
        w = want_of(by_id["u_nt_%s_mem" % ("pairs" if pe else "single")])["lines"]
        short = {(l1, l2) for l1 in (m3 - 1, m3) for l2 in (0, m3 - 1, m3) if (l1 < m3 and l2 < m3 if pe else l1 < m3)}
        assert {b"U\tu_%d_%d\t0\n" % x for x in short} == {l for l in w if l.endswith(b"\t0\n")} and len(short) == (2 if pe else 3)
    # the kaijup rule, outcome by outcome
    gated = lambda cid: {l.split(b"\t")[1] for l in want_of(by_id[cid])["lines"] if l.endswith(b"\t0\n")}
    breaks = {b"break_" + bytes([c]) for c in b"BJOUXZbjouxz*"}
    mem_gated = {b"empty", b"short", b"two_short", b"at_end_short", b"straddle31_short", b"long_broken", b"not_letters"} | breaks
    assert gated("u_protein_mem") == mem_gated
    assert gated("u_protein_greedy") == mem_gated | {b"lowA", b"s64", b"s64_twice"}
    assert gated("u_protein_m5_s30") == {b"empty", b"not_letters"}
    assert {bytes([c + 32 * k]) for c in b"BJOUXZ" for k in (0, 1)} == {bytes([c]) for c in range(256) if bytes([c]).isalpha() and c < 128
                                                                        and chr(c).upper() not in fse.BLOSUM62_DIAGONAL}
    # the grid: source and destination alignment of names and peptides; the middle at every alignment of its place
    g, w = by_id["alignment_grid"], want_of(by_id["alignment_grid"])
    assert w["res"]["classified"].all()
    seen_n, seen_p, seen_m = set(), set(), set()
    for r in range(len(g["hits"])):
        lo, nl, tl = int(w["line_off"][r]), int(g["names"][r]["len"]), int(g["v"][r]["text_len"])
        seen_n.add((int(g["names"][r]["pos"]) % 16, (lo + 2) % 16))
        seen_p.add((int(g["text_pos"][r]) % 16, (int(w["line_off"][r + 1]) - 1 - tl) % 16))
        seen_m.add((lo + 3 + nl) % 16)
    assert len(seen_n) == 256 and len(seen_p) == 256 and len(seen_m) == 16


def test_every_input_in_every_order(emu, inputs, want_of):
    for case in inputs:
        want = want_of(case)
        for order in (0, 1, 2):
            out, info = run_emu(emu, case, len(want["text"]) + 5, order, seed=3 + order)
            compare(out, info, want, (case["id"], order))


def test_second_step_of_the_scan_at_the_exact_capacity(emu, inputs, want_of):
    """more records than the one block on top of the prefix sum takes in a step, into a buffer of exactly the text's length"""
    case = [k for k in inputs if k["id"] == "n_%d" % fsi.BIG_COUNT][0]
    want = want_of(case)
    out, info = run_emu(emu, case, len(want["text"]), 2, seed=8)
    compare(out, info, want, case["id"])


def test_capacity(emu, inputs, want_of):
    jobs = fsi.capacity_cases(inputs, want_of)
    assert len(jobs) == 8 * len(fsi.CAPACITY_IDS)
    for case, cap in jobs:
        want = fse.expected(case, db_of(case), cap)
        assert want["info"]["overflow"] == (1 if cap < len(want["text"]) else 0) and want["info"]["text_bytes"] == len(want["text"])
        assert want["written"] == want["text"][: len(want["written"])] and (not want["written"] or want["written"].endswith(b"\n"))
        for order in (0, 2):
            out, info = run_emu(emu, case, cap, order)
            compare(out, info, want, (case["id"], cap, order))


def test_sanitizer_build_runs_every_input_clean(tmp_path):
    """the emulation as a program of its own, with the address and undefined-behaviour sanitizers, on all inputs and capacity
    cases in the three orders: every array in a heap block of exactly its size"""
    exe, cases_file = str(tmp_path / "format_seq_emu_san"), str(tmp_path / "cases.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-DFORMAT_SEQ_EMU_MAIN",
                    "-o", exe, EMU_SRC], check=True)
    fsi.main(cases_file)
    r = subprocess.run([exe, cases_file], capture_output=True, timeout=600)
    assert r.returncode == 0 and b" 0 differ" in r.stdout and not r.stderr, (r.stdout[-400:], r.stderr[-2000:])


def test_entry_points_exist_and_need_a_device():
    L = api.lib()
    for sym in ("kaiju_gpu_index_upload_seq_names", "kaiju_gpu_index_seq_name_bytes", "kaiju_gpu_format_seq", "kaiju_gpu_format_seq_device",
                "kaiju_gpu_classify_batch_seq_text"):
        assert hasattr(L, sym), sym
    assert L.kaiju_gpu_index_seq_name_bytes(None) == 0
    for name in ("upload_seq_names",):
        assert hasattr(api.Index, name)
    for name in ("format_seq", "format_seq_device", "classify_seq_text"):
        assert hasattr(api.Classifier, name)
    if api.device_count() > 0:
        return            # (a HIP device is visible: the answer without one cannot be seen here)
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    text, nbytes = C.c_void_p(), C.c_uint64()
    assert L.kaiju_gpu_index_upload_seq_names(None) == -4
    assert L.kaiju_gpu_format_seq(None, p, p, 1, 0, 0, None, None, None, None, 0, 0, b"r", 1, p, p, 64, p) == -4
    assert L.kaiju_gpu_format_seq(None, None, None, 0, 0, 7, None, None, None, None, 0, 0, None, 0, None, None, 0, None) == -4
    assert L.kaiju_gpu_format_seq_device(None, None, None, 0, 0, 0, None, None, None, None, 0, None, 0, None, None, 0, None, None) == -4
    assert L.kaiju_gpu_format_seq_device(None, p, p, 1, 0, 1, p, p, p, p, 0, p, 0, p, p + 4, 64, p, None) == -4      # (a misaligned output too)
    assert L.kaiju_gpu_classify_batch_seq_text(None, b"ACGT", p, 1, 0, 0, 0, b"r", 1, p, C.byref(text), C.byref(nbytes), p) == -4
    assert L.kaiju_gpu_classify_batch_seq_text(None, b"ACGT", p, 1, 0, 1, 1, b"r", 1, p, C.byref(text), C.byref(nbytes), p) == -4
