"""The lines with the column of kaiju-addTaxonNames (kaiju_amd/csrc/kj_format_names.h) on the host:
tests/emu/format_names_emu.cpp drives the per-lane functions the kernels of format_names.hip are made of, pass by pass, with
the work units of every pass in forward, reversed and shuffled order.  Every input of tests/format_inputs.py, and records
drawn over every taxon of tests/golden/names/deep/, in the three modes with and without the unclassified lines, must give the
bytes and kaiju_gpu_format_names_info that tests/names_expect.py builds (the reference tool pins that file:
tests/test_names_expect_golden.py).  The tables the upload builds, read byte by byte as the write pass reads them, against the
loader's own walk of the tree."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import format_expect
import names_expect
import names_inputs
import util
from kaiju_amd import api
from test_format_emu import db_of, golden_db_length, library_table

NAMES_MODE = {"name": (0, None), "path": (1, None)}
GUARD = 37


def mode_args(mode):
    return (2, mode[len("ranks:"):].encode()) if mode.startswith("ranks:") else NAMES_MODE[mode]


def build_format_names_emu(directory):
    so = str(directory / "libformat_names_emu.so")
    src = [os.path.join(util.ROOT, "tests", "emu", "format_names_emu.cpp"), os.path.join(util.ROOT, "kaiju_amd", "csrc", "taxon_names.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", so] + src, check=True)
    L = C.CDLL(so)
    L.kaiju_taxon_names_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_void_p]
    L.kaiju_taxon_names_free.argtypes = [C.c_void_p]
    L.kaiju_taxon_names_annotation.restype = C.c_int64
    L.kaiju_taxon_names_annotation.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    L.kaiju_taxon_names_last_error.restype = C.c_char_p
    L.format_names_emu_constants.argtypes = [C.c_void_p]
    L.format_names_emu_table.restype = C.c_int64
    L.format_names_emu_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint32]
    L.format_names_emu_annotation.restype = C.c_int64
    L.format_names_emu_annotation.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    L.format_names_emu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_double, C.c_double,
                                   C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint32]
    return L


def constants(L):
    k = np.zeros(4, dtype=np.uint32)
    L.format_names_emu_constants(k.ctypes.data)
    return int(k[0]), int(k[1]), int(k[3])


def load(L, nodes, names, mode):
    m, ranks = mode_args(mode)
    h = C.c_void_p()
    assert L.kaiju_taxon_names_load(nodes.encode(), names.encode(), m, ranks, C.byref(h)) == 0, L.kaiju_taxon_names_last_error()
    return h


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_format_names_emu(tmp_path_factory.mktemp("format_names_emu"))


@pytest.fixture(scope="module")
def trees(emu):
    """per mode: the loaded tables of deep/ and the expectation"""
    t = {m: (load(emu, names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, m), names_inputs.deep_expect(m)) for m in names_inputs.MODES}
    yield t
    for h, _ in t.values():
        emu.kaiju_taxon_names_free(h)


@pytest.fixture(scope="module")
def inputs(emu, golden):
    import format_inputs
    B, S, K = constants(emu)
    assert (B, S, K) == (4096, 256, 4096)
    return format_inputs.cases(B, S, K, golden_db_length(golden)) + [names_inputs.drawn(n) for n in (300, 4096)]


@pytest.fixture(scope="module")
def base(inputs, golden):
    """the three-column lines of every case (format_expect), made once"""
    return {k["id"]: format_expect.expected(k, db_of(k, golden)) for k in inputs}


def run_emu(L, case, handle, drop, db_length, out_cap, order, seed=1):
    pw = library_table(constants(L)[2])
    out = np.full(out_cap + GUARD, 0xA5, dtype=np.uint8)
    info = np.zeros(1, dtype=api.FORMAT_NAMES_INFO_DTYPE)
    text = np.frombuffer(case["text1"] + b"\0", dtype=np.uint8)
    rc = L.format_names_emu(pw.ctypes.data, case["recs"].ctypes.data, case["off"].ctypes.data, len(case["recs"]), 1 if case["paired"] else 0,
                            text.ctypes.data, len(case["text1"]), case["names"].ctypes.data, db_length, case["min_evalue"],
                            1 if case["mode"] == "greedy" else 0, 1 if case["protein"] else 0, handle, 1 if drop else 0, out.ctypes.data, out_cap,
                            info.ctypes.data, order, seed)
    assert rc == 0
    return out, info[0]


def compare(out, info, want, what):
    for f in names_expect.NAMES_INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def test_every_input_in_every_variant_and_order(emu, trees, inputs, base, golden):
    seen = {f: 0 for f in ("n_unknown_taxon", "n_unnamed_taxon", "n_dropped")}
    for case in inputs:
        for mode, drop in names_inputs.VARIANTS:
            handle, expect = trees[mode]
            want = names_expect.expected(expect, base[case["id"]], drop)
            for f in seen:
                seen[f] += want["info"][f]
            for order in (0, 1, 2):
                out, info = run_emu(emu, case, handle, drop, db_of(case, golden), len(want["text"]) + 5, order, seed=3 + order)
                compare(out, info, want, (case["id"], mode, drop, order))
    assert all(v > 0 for v in seen.values()), seen


def test_second_step_of_the_scan_at_the_exact_capacity(emu, trees, golden):
    """more records than the one block on top of the prefix sum takes in a step, into a buffer of exactly the text's length"""
    case = names_inputs.big()
    assert len(case["recs"]) > constants(emu)[1] ** 2
    handle, expect = trees["path"]
    want = names_expect.expected(expect, format_expect.expected(case, db_of(case, golden)), False)
    assert want["info"]["n_unknown_taxon"] > 0 and b"\tLineage 9; \n" in want["text"]
    out, info = run_emu(emu, case, handle, False, db_of(case, golden), len(want["text"]), 2, seed=8)
    compare(out, info, want, case["id"])


def test_capacity(emu, trees, inputs, base, golden):
    jobs = names_inputs.capacity_jobs(inputs, lambda k, m, d: names_expect.expected(trees[m][1], base[k["id"]], d))
    assert len(jobs) == 4 * (2 * 6 + 2 * 5)
    cut_inside = 0
    for case, mode, drop, cap in jobs:
        want = names_expect.expected(trees[mode][1], base[case["id"]], drop, cap)
        assert want["info"]["overflow"] == (1 if cap < len(want["text"]) else 0) and want["info"]["text_bytes"] == len(want["text"])
        assert want["written"] == want["text"][: len(want["written"])] and (not want["written"] or want["written"].endswith(b"\n"))
        cut_inside += 0 < cap - len(want["written"]) and cap < len(want["text"])
        for order in (0, 2):
            out, info = run_emu(emu, case, trees[mode][0], drop, db_of(case, golden), cap, order)
            compare(out, info, want, (case["id"], mode, drop, cap, order))
    assert cut_inside >= 8


def test_tables_against_the_walk(emu, trees):
    """path_len / rank_src / rank_len from the build functions, read as the write pass reads them, give for every node of deep/
    (and for taxa that are none) the annotation the loader's own walk gives, and the one of names_expect; in every order of
    the slots the tables are the same"""
    taxa = names_inputs.deep_taxa()
    for mode in names_inputs.MODES:
        handle, expect = trees[mode]
        longest = 0
        for t in taxa:
            want = expect.annotation(t)
            n = emu.kaiju_taxon_names_annotation(handle, t, None, 0)
            assert n == (-1 if want is None else len(want)), (mode, t)
            buf, buf2 = np.zeros(max(n, 0) + 1, dtype=np.uint8), np.zeros(max(n, 0) + 1, dtype=np.uint8)
            assert emu.kaiju_taxon_names_annotation(handle, t, buf.ctypes.data, max(n, 0)) == n
            assert emu.format_names_emu_annotation(handle, t, buf2.ctypes.data, max(n, 0)) == n, (mode, t)
            if want is not None:
                assert buf[:n].tobytes() == want and buf2[:n].tobytes() == want, (mode, t)
                longest = max(longest, n)
        most = C.c_uint64()
        cap = emu.format_names_emu_table(handle, 0, None, 0, C.byref(most), 0, 1)
        assert cap > 0 and cap & (cap - 1) == 0
        # (the largest annotation of any slot: but in name mode nodes without a name of their own have one too)
        assert most.value >= longest and (mode != "name" or most.value == longest)
        for which in {"name": (), "path": (4,), names_inputs.RANKS_DEEP: (5, 6)}[mode]:
            tabs = []
            for order in (0, 1, 2):
                a = np.zeros(cap * (3 if which == 6 else 1), dtype=np.uint32)
                assert emu.format_names_emu_table(handle, which, a.ctypes.data, a.nbytes, None, order, 5) == cap
                tabs.append(a)
            assert np.array_equal(tabs[0], tabs[1]) and np.array_equal(tabs[0], tabs[2]) and not np.any(tabs[0] == 0xdeadbeef)
