"""The stand-alone annotator (kaiju_amd/csrc/kj_annotate.h) on the host: tests/emu/annotate_emu.cpp drives the per-lane
functions the kernels of annotate.hip are made of, pass by pass, with the work units of every pass in forward, reversed and
shuffled order.  The fixtures the reference tool wrote and the smallest texts at which a pass can go wrong, in {name, path,
ranks} x {keep, drop}, must give the bytes and kaiju_gpu_annotate_info of tests/annotate_expect.py (the reference tool pins
that file: tests/test_annotate_expect_golden.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import annotate_expect
import annotate_inputs as ai
import names_inputs
import util
from kaiju_amd import api
from test_format_names_emu import mode_args

GUARD = 37


def build_annotate_emu(directory):
    so = str(directory / "libannotate_emu.so")
    src = [os.path.join(util.ROOT, "tests", "emu", "annotate_emu.cpp"), os.path.join(util.ROOT, "kaiju_amd", "csrc", "taxon_names.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", so] + src, check=True)
    L = C.CDLL(so)
    L.kaiju_taxon_names_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_void_p]
    L.kaiju_taxon_names_free.argtypes = [C.c_void_p]
    L.kaiju_taxon_names_last_error.restype = C.c_char_p
    L.annotate_emu_constants.argtypes = [C.c_void_p]
    L.annotate_emu_bound.restype = C.c_uint64
    L.annotate_emu_bound.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    L.annotate_emu.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint32]
    return L


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    L = build_annotate_emu(tmp_path_factory.mktemp("annotate_emu"))
    k = np.zeros(4, dtype=np.uint32)
    L.annotate_emu_constants(k.ctypes.data)
    assert [int(x) for x in k] == [ai.TILE, 256, ai.CHUNK, ai.TILE]
    return L


def load(L, nodes, names, mode):
    m, ranks = mode_args(mode)
    h = C.c_void_p()
    assert L.kaiju_taxon_names_load(nodes.encode(), names.encode(), m, ranks, C.byref(h)) == 0, L.kaiju_taxon_names_last_error()
    return h


@pytest.fixture(scope="module")
def trees(emu):
    """per mode: the loaded tables of deep/ and the expectation; "golden:<mode>": those of tests/golden/nodes.dmp"""
    t = {m: (load(emu, names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, m), ai.deep_names(m)) for m in names_inputs.MODES}
    for m in ("name", "path"):
        t["golden:" + m] = (load(emu, os.path.join(ai.GOLDEN, "nodes.dmp"), names_inputs.GOLDEN_NAMES, m), ai.golden_names(m))
    yield t
    for h, _ in t.values():
        emu.kaiju_taxon_names_free(h)


def run_emu(L, text, handle, drop, out_cap, order, seed=1):
    out = np.full(out_cap + GUARD, 0xA5, dtype=np.uint8)
    info = np.zeros(1, dtype=api.ANNOTATE_INFO_DTYPE)
    rc = L.annotate_emu(text, len(text), handle, 1 if drop else 0, out.ctypes.data, out_cap, info.ctypes.data, order, seed)
    assert rc == 0, rc
    return out, info[0]


def compare(out, info, want, what):
    for f in annotate_expect.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def check(L, trees, text, what, orders=(0, 1, 2), variants=ai.VARIANTS):
    """text in every variant and order, into a buffer five bytes longer than needed"""
    for mode, drop in variants:
        handle, names = trees[mode]
        want = annotate_expect.expected(names, text, drop)
        assert len(want["text"]) <= L.annotate_emu_bound(len(text), text.count(b"\n") + 1, handle)
        for order in orders:
            out, info = run_emu(L, text, handle, drop, len(want["text"]) + 5, order, seed=3 + order)
            compare(out, info, want, (what, mode, drop, order))


@pytest.mark.parametrize("fixture", ["deep", "odd"])
def test_fixtures(emu, trees, fixture):
    text = ai.fixture_input(fixture)
    check(emu, trees, text, fixture)
    for out, mode, drop in ai.FOUR_MODES:                    # and straight against the files the tool wrote
        got, info = run_emu(emu, text, trees[mode][0], drop, len(ai.fixture_output(fixture, out)), 0)
        assert bytes(got[: int(info["text_bytes"])]) == ai.fixture_output(fixture, out) and info["overflow"] == 0


@pytest.mark.parametrize("run", ["mem", "greedy"])
def test_verbose_lines(emu, trees, run):
    text = ai.verbose_input(run)
    for kind in ("name", "path"):
        handle, names = trees["golden:" + kind]
        want = ai.verbose_output(run, kind)
        assert annotate_expect.expected(names, text)["text"] == want
        out, info = run_emu(emu, text, handle, False, len(want), 2, seed=5)
        assert bytes(out[: len(want)]) == want and np.all(out[len(want):] == 0xA5) and int(info["text_bytes"]) == len(want)


def test_small_cases(emu, trees):
    seen = {f: 0 for f in ("n_bad_id", "n_unknown_taxon", "n_unnamed_taxon", "n_dropped", "n_empty", "n_annotated")}
    ids = set()
    for what, text in ai.small_cases():
        ids.add(what)
        check(emu, trees, text, what)
        for mode, drop in ai.VARIANTS:
            for f in seen:
                seen[f] += annotate_expect.expected(trees[mode][1], text, drop)["info"][f]
    assert {"bytes_0", "bytes_1", "bytes_15", "bytes_16", "bytes_17", "bytes_4095", "bytes_4096", "bytes_4097", "only_newlines", "no_newline",
            "line_end_every_offset", "body_16_off0", "body_32_off1", "long_line", "all_dropped"} <= ids
    assert all(v > 0 for k, v in seen.items() if k != "n_bad_id"), seen
    e = annotate_expect.expected(trees["path"][1], dict(ai.small_cases())["all_dropped"], True)
    assert e["text"] == b"" and e["info"]["n_dropped"] == 21 and e["info"]["n_empty"] == 1


def test_second_step_of_the_scan_at_the_exact_capacity(emu, trees):
    text = ai.big()
    assert text.count(b"\n") == names_inputs.BIG_COUNT > 256 * 256
    handle, names = trees["path"]
    want = annotate_expect.expected(names, text)
    assert want["info"]["n_unknown_taxon"] > 0 and want["info"]["n_empty"] > 6000 and b"\tLineage 9; \n" in want["text"]
    out, info = run_emu(emu, text, handle, False, len(want["text"]), 2, seed=8)
    compare(out, info, want, "big")


def test_capacity(emu, trees):
    text = ai.capacity_text()
    jobs, cut_inside = 0, 0
    for mode, drop in (("path", False), ("path", True), ("name", True), (ai.RANKS_DEEP, False)):
        handle, names = trees[mode]
        full = annotate_expect.expected(names, text, drop)
        caps = ai.capacity_caps(full, mode)
        assert len(caps) == (7 if mode == "path" else 6)
        for cap in caps:
            want = annotate_expect.expected(names, text, drop, cap)
            assert want["info"]["overflow"] == (1 if cap < len(full["text"]) else 0) and want["info"]["text_bytes"] == len(full["text"])
            assert want["written"] == full["text"][: len(want["written"])] and (not want["written"] or want["written"].endswith(b"\n"))
            cut_inside += 0 < cap - len(want["written"]) and cap < len(full["text"])
            for order in (0, 2):
                out, info = run_emu(emu, text, handle, drop, cap, order)
                compare(out, info, want, (mode, drop, cap, order))
            jobs += 1
    assert jobs == 2 * 7 + 2 * 6 and cut_inside >= 8
