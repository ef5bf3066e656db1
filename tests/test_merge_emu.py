"""The merger (kaiju_amd/csrc/kj_merge.h) on the host: tests/emu/merge_emu.cpp drives the per-lane functions the kernels of
merge.hip are made of, pass by pass, with the work units of every pass in forward, reversed and shuffled order.  The fixtures
the reference tool wrote and the smallest texts at which a pass can go wrong must give the bytes and kaiju_gpu_merge_info of
tests/merge_expect.py (the reference tool pins that file: tests/test_merge_expect_golden.py)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import merge_expect as me
import merge_inputs as mi
import util
from kaiju_amd import api
from test_merge_expect_golden import as_double, in_domain

GUARD = 37


def build_merge_emu(directory):
    so = str(directory / "libmerge_emu.so")
    src = [os.path.join(util.ROOT, "tests", "emu", "merge_emu.cpp"), os.path.join(util.ROOT, "kaiju_amd", "csrc", "taxonomy.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", so] + src, check=True)
    L = C.CDLL(so)
    L.kaiju_taxonomy_load.argtypes = [C.c_char_p, C.c_void_p]
    L.kaiju_taxonomy_free.argtypes = [C.c_void_p]
    L.merge_emu_constants.argtypes = [C.c_void_p]
    L.merge_emu_bound.restype = C.c_uint64
    L.merge_emu_bound.argtypes = [C.c_uint64, C.c_uint64]
    L.merge_emu_score.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.merge_emu_score_cmp.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32]
    L.merge_emu.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int,
                            C.c_uint32]
    return L


class Trees:
    """nodes.dmp bytes -> (the emulation's tree, the model's)"""

    def __init__(self, L, directory):
        self.L, self.dir, self.known = L, directory, {}

    def get(self, nodes):
        if nodes is None:
            return None, {}
        if nodes not in self.known:
            path = self.dir / ("nodes%d.dmp" % len(self.known))
            path.write_bytes(nodes)
            h = C.c_void_p()
            assert self.L.kaiju_taxonomy_load(str(path).encode(), C.byref(h)) == 0
            self.known[nodes] = (h, me.parse_nodes(nodes))
        return self.known[nodes]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("merge_emu")
    L = build_merge_emu(d)
    k = np.zeros(5, dtype=np.uint32)
    L.merge_emu_constants(k.ctypes.data)
    assert [int(x) for x in k] == [mi.TILE, 256, mi.CHUNK, mi.TILE, 32]
    trees = Trees(L, d)
    yield L, trees
    for h, _ in trees.known.values():
        L.kaiju_taxonomy_free(h)


def run_emu(L, tree, t1, t2, mode, use_score, final, out_cap, order, seed=1):
    out = np.full(out_cap + GUARD, 0xA5, dtype=np.uint8)
    info = np.zeros(1, dtype=api.MERGE_INFO_DTYPE)
    rc = L.merge_emu(t1, len(t1), t2, len(t2), tree, me.MODE_CODE[mode], 1 if use_score else 0, 1 if final else 0, out.ctypes.data, out_cap, info.ctypes.data,
                     order, seed)
    assert rc == 0, rc
    return out, info[0]


def compare(out, info, want, what):
    for f in me.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def check(emu, nodes, t1, t2, mode, use_score, final, what, orders=(0, 1, 2)):
    L, trees = emu
    tree, parent = trees.get(nodes)
    want = me.expected(parent, t1, t2, mode, use_score, final)
    assert len(want["text"]) <= L.merge_emu_bound(len(t1), len(t2))
    for order in orders:
        out, info = run_emu(L, tree, t1, t2, mode, use_score, final, len(want["text"]) + 5, order, seed=3 + order)
        compare(out, info, want, (what, order))
    return want


@pytest.mark.parametrize("mode,use_score", mi.VARIANTS)
def test_odd_and_real(emu, mode, use_score):
    for what, (nodes, t1, t2), (text, _) in (("odd", mi.odd(), mi.odd_output(mode, use_score)), ("real", mi.real(), mi.real_output(mode, use_score))):
        want = check(emu, nodes, t1, t2, mode, use_score, True, what)
        assert want["text"] == text                              # and straight against the file the tool wrote
    if mode == "lowest":
        _, t1, t2 = mi.odd()
        assert check(emu, None, t1, t2, mode, use_score, True, "odd without a tree")["text"] == mi.odd_output(mode, use_score, tree=False)[0]


def test_stops(emu):
    for name in mi.stop_names():
        t1, t2, use_score, text, summary = mi.stop_case(name)
        want = check(emu, None, t1, t2, "1", use_score, True, name)
        assert want["text"] == text and me.summary(want["info"]) == summary


def test_small_cases(emu):
    seen = set()
    for what, nodes, t1, t2, mode, use_score, final in mi.small_cases():
        want = check(emu, nodes, t1, t2, mode, use_score, final, what)
        seen.add(want["info"]["stop_why"])
        seen.add(what)
    assert {me.STOP["score_wide"], me.STOP["2_short"], me.STOP["2_column"], me.STOP["1_class"], "pairs_700", "stop_two", "offset_16", "long_name"} <= seen
    cases = {c[0]: c for c in mi.small_cases()}
    e = lambda what: me.expected(me.parse_nodes(cases[what][1] or b""), *cases[what][2:])
    assert e("stop_two")["info"]["stop_pair"] == 300 and e("stop_two_near")["info"]["stop_pair"] == 255 and e("stop_two")["info"]["count_c2"] == 300
    digits = e("lca_digits_lca_s")["text"].split(b"\n")
    assert [len(l.split(b"\t")[2]) for l in digits[:4]] == [1, 10, 19, 20] and digits[3].split(b"\t")[2] == b"%d" % mi.BIG
    assert e("score_wide_s")["info"]["stop_pair"] == 1 and e("score_wide")["info"]["stop_pair"] == me.NO_PAIR and e("score_wide_cu_s")["info"]["stop_pair"] == me.NO_PAIR
    assert e("score_1e300_s")["info"]["stop_why"] == me.STOP["score_wide"] and e("score_1e309_s")["text"] == b"C\ta\t5\t1\n"
    assert e("ragged_final0")["info"]["used1"] == 12 and e("ragged_final0")["info"]["used2"] == 12 and e("ragged_final1")["info"]["stop_why"] == me.STOP["2_tabs"]
    assert e("ids_lca_s")["text"].startswith(b"C\tr0\t4\t1.5\nC\tr1\t4\t1.5\nC\tr2\t5\t1.5\nC\tr3\tx\t1.5\n")


def test_name_compare(emu):
    cases = mi.name_compare_cases()
    assert len(cases) == 16 * (1 + 1 + 2 + 4 * 3)
    stops = 0
    for what, t1, t2 in cases:
        want = check(emu, None, t1, t2, "1", False, True, what, orders=(2,))
        if "equal" in what:
            assert want["info"]["stop_pair"] == me.NO_PAIR and want["info"]["count"] == 7
        else:
            assert want["info"]["stop_pair"] == 7 and want["info"]["stop_why"] == me.STOP["names"]
            stops += 1
    assert stops == 16 * 15


def test_capacity(emu):
    L, trees = emu
    nodes, t1, t2 = mi.odd()
    tree, parent = trees.get(nodes)
    full = me.expected(parent, t1, t2, "lca", True)
    total = len(full["text"])
    last = len(full["text"].rstrip(b"\n").rsplit(b"\n", 1)[0]) + 1
    for cap in (total, total - 1, last, last - 1, 0, 1, 7, 8, 4096, 4097, total + 100):
        want = me.expected(parent, t1, t2, "lca", True, True, cap)
        assert want["info"]["overflow"] == (1 if cap < total else 0) and want["info"]["text_bytes"] == total
        assert want["written"] == full["text"][: len(want["written"])] and (not want["written"] or want["written"].endswith(b"\n"))
        for order in (0, 2):
            out, info = run_emu(L, tree, t1, t2, "lca", True, True, cap, order)
            compare(out, info, want, (cap, order))
    assert len(me.expected(parent, t1, t2, "lca", True, True, total - 1)["written"]) == last


def test_carry_over_in_two_calls_equals_one(emu):
    L, trees = emu
    nodes, t1, t2 = mi.real()
    tree, parent = trees.get(nodes)
    whole = me.expected(parent, t1, t2, "lowest", True)
    for cut1, cut2 in ((5000, 3000), (3000, 5000), (1, 20000), (len(t1), 100)):
        a = check(emu, nodes, t1[:cut1], t2[:cut2], "lowest", True, False, ("first call", cut1, cut2), orders=(2,))
        u1, u2 = a["info"]["used1"], a["info"]["used2"]
        assert u1 <= cut1 and u2 <= cut2 and (u1 == 0 or t1[u1 - 1:u1] == b"\n") and (u2 == 0 or t2[u2 - 1:u2] == b"\n")
        b = check(emu, nodes, t1[u1:], t2[u2:], "lowest", True, True, ("second call", cut1, cut2), orders=(2,))
        assert a["text"] + b["text"] == whole["text"]
        for f in ("count", "count_c1", "count_c2", "count_c12", "count_c3", "count_c1_not_c2", "count_c2_not_c1"):
            assert a["info"][f] + b["info"][f] == whole["info"][f]


def test_scores_as_decimals(emu):
    """kjm::score_value / score_cmp against the doubles on texts inside the domain; outside it they say so"""
    L, _ = emu
    rng = random.Random(7)
    n = 0
    for _ in range(20000):
        a, b = in_domain(rng), in_domain(rng)
        if rng.random() < 0.3:
            b = a + b"0" if b"." in a else a
        try:
            me.score_value(a), me.score_value(b)
        except me.ScoreWide:
            exp, mant = C.c_int32(), C.c_uint64()
            assert 2 in (L.merge_emu_score(a, len(a), C.byref(exp), C.byref(mant)), L.merge_emu_score(b, len(b), C.byref(exp), C.byref(mant)))
            continue
        x, y = as_double(a), as_double(b)
        assert L.merge_emu_score_cmp(a, len(a), b, len(b)) == (x > y) - (x < y), (a, b)
        n += 1
    assert n > 10000
    exp, mant = C.c_int32(), C.c_uint64()
    for s, kind in ((b"9007199254740993", 2), (b"1" + b"0" * 300, 2), (b"1" + b"0" * 308, 2), (b"1" + b"0" * 309, 0), (b"9" * 400, 0), (b"", 0), (b".", 0),
                    (b"0." + b"0" * 300 + b"1", 2), (b"0." + b"0" * 299 + b"1", 1), (b"123456789012345", 1), (b"1234567890123456", 2), (b"12345678901234500000", 1)):
        assert L.merge_emu_score(s, len(s), C.byref(exp), C.byref(mant)) == kind, s


def test_walks_end_on_trees_outside_the_domain(emu):
    """a parent that is no node (the reference aborts) and cycles other than the self-parent (the reference never returns): no
    golden, but every walk ends - it counts a stored depth down - and every pair gives a line"""
    L, trees = emu
    nodes = mi.nodes([(1, 1), (2, 1), (3, 2), (10, 77), (11, 10), (12, 11), (50, 51), (51, 52), (52, 50), (53, 50), (60, 60), (61, 61)])
    tree, _ = trees.get(nodes)
    ids = [1, 2, 3, 10, 11, 12, 50, 51, 52, 53, 60, 61, 77]
    pairs = [(a, b) for a in ids for b in ids if a != b]
    t1 = b"".join(b"C\tr%d\t%d\t5\n" % (k, a) for k, (a, b) in enumerate(pairs))
    t2 = b"".join(b"C\tr%d\t%d\t5\n" % (k, b) for k, (a, b) in enumerate(pairs))
    for mode in ("lca", "lowest"):
        out, info = run_emu(L, tree, t1, t2, mode, True, True, L.merge_emu_bound(len(t1), len(t2)), 2)
        assert int(info["stop_pair"]) == me.NO_PAIR and int(info["count_c12"]) == len(pairs) == 156
        lines = bytes(out[: int(info["text_bytes"])]).split(b"\n")[:-1]
        assert len(lines) == len(pairs) and all(l.startswith(b"C\tr%d\t" % k) and l.endswith(b"\t5") for k, l in enumerate(lines))
        # inside the domain the answers are the tool's: 3 and 2 under the root 1
        assert lines[pairs.index((3, 2))] == b"C\tr%d\t%d\t5" % (pairs.index((3, 2)), 1 if mode == "lca" else 3)
