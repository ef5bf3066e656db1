"""The Krona text (kaiju_amd/csrc/kj_krona.h) on the host: tests/emu/krona_emu.cpp drives the per-lane functions the kernels of
krona.hip are made of, pass by pass, with the work units of every pass in forward, reversed and shuffled order.  Every
direct[] pattern of the fixtures, injected counts of 1, 9, 10, 10^19 and 2^64 - 1, capacities at 0, at a line end +- 1 and
inside a lineage must give the bytes and the info of tests/krona_expect.py (the reference tool pins that file:
tests/test_krona_expect_golden.py), with the guard bytes behind the text untouched; and the tables, read as the write pass
reads them, must spell what a walk with strings spells."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import krona_expect as ke
import krona_inputs as ki
import table_expect as te
import table_inputs as ti
import util
from kaiju_amd import api


def build_krona_emu(directory):
    so = str(directory / "libkrona_emu.so")
    src = [os.path.join(util.ROOT, "tests", "emu", "krona_emu.cpp"), os.path.join(util.ROOT, "kaiju_amd", "csrc", "taxon_names.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", so] + src, check=True)
    L = C.CDLL(so)
    L.kaiju_taxon_names_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_void_p]
    L.kaiju_taxon_names_free.argtypes = [C.c_void_p]
    L.krona_emu_constants.argtypes = [C.c_void_p]
    L.krona_emu_create.restype = C.c_void_p
    L.krona_emu_create.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_uint32]
    L.krona_emu_free.argtypes = [C.c_void_p]
    L.krona_emu_longest.restype = C.c_uint64
    L.krona_emu_longest.argtypes = [C.c_void_p]
    L.krona_emu_check_tables.restype = C.c_int64
    L.krona_emu_check_tables.argtypes = [C.c_void_p]
    L.krona_emu_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint32]
    return L


class Emu:
    def __init__(self, L, nodes, names, ranks, order, mode=api.NAMES_NAME):
        self.L, self.order = L, order
        self.names = C.c_void_p()
        assert L.kaiju_taxon_names_load(nodes.encode(), names.encode(), mode, None, C.byref(self.names)) == 0
        self.h = L.krona_emu_create(self.names, None if ranks is None else ranks.encode(), order, 7)
        assert self.h

    def text(self, direct, n_unclassified=0, unclassified=False, out_cap=0):
        ids = np.array(list(direct.keys()), dtype=np.uint64)
        counts = np.array(list(direct.values()), dtype=np.uint64)
        out = np.full(max(out_cap, 1), 0x77, dtype=np.uint8)
        info = np.zeros(1, dtype=api.KRONA_INFO_DTYPE)
        rc = self.L.krona_emu_text(self.h, ids.ctypes.data, counts.ctypes.data, len(ids), n_unclassified, 1 if unclassified else 0, out.ctypes.data, out_cap,
                                   info.ctypes.data, self.order, 11)
        assert rc == 0, rc
        return bytes(out[:int(info[0]["written_bytes"])]), info[0]

    def close(self):
        self.L.krona_emu_free(self.h)
        self.L.kaiju_taxon_names_free(self.names)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = build_krona_emu(tmp_path_factory.mktemp("krona_emu"))
    k = np.zeros(5, dtype=np.uint32)
    L.krona_emu_constants(k.ctypes.data)
    assert [int(x) for x in k] == [4096, 16, 64, api.KRONA_MAX_TALLIES, 64]
    return L


def same(emu, tree, direct, n_u, unclassified, ranks, out_cap, what):
    want = ke.expected(tree, direct, n_u, unclassified, ranks, out_cap)
    got, info = emu.text(direct, n_u, unclassified, out_cap)
    assert got == want["written"], what
    for f in ke.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f)
    assert int(info["reserved"]) == 0


def capacities(tree, direct, n_u, unclassified, ranks):
    """0, every line end and one byte to either side of it, a byte inside the longest lineage, the exact size and beyond"""
    lines, _, _ = ke.lines_of(tree, direct, n_u, unclassified, ranks)
    caps, at = {0}, 0
    for line in lines:
        at += len(line)
        caps |= {at - 1, at, at + 1}
    if lines:
        k = max(range(len(lines)), key=lambda i: len(lines[i]))
        caps.add(sum(len(x) for x in lines[:k]) + len(lines[k]) // 2)
    return sorted(caps | {at + 40})


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(ki.SETS))
def test_the_fixtures_at_every_capacity(lib, order, name):
    u, ranks = ki.SETS[name]
    emu = Emu(lib, ki.NODES, ki.NAMES, ranks, order)
    tree = ki.fixture_tree()
    for label in ki.FILES:
        direct, n_u = ke.direct_of(tree, [ti.read(ki.FILES[label])])
        for cap in capacities(tree, direct, n_u, u, ranks):
            same(emu, tree, direct, n_u, u, ranks, cap, (label, name, cap))
    emu.close()


@pytest.mark.parametrize("order", [0, 2])
def test_the_golden_reads_over_the_real_tree(lib, order):
    tree = ti.real_tree()
    direct, n_u = ke.direct_of(tree, [ti.read(ki.REAL_FILE)])
    for name, (u, ranks) in sorted(ki.SETS.items()):
        emu = Emu(lib, ti.REAL_NODES, ti.REAL_NAMES, ranks, order, api.NAMES_PATH)       # (names of any mode serve)
        want = ke.expected(tree, direct, n_u, u, ranks)
        got, info = emu.text(direct, n_u, u, len(want["text"]))
        assert got == want["text"] and ke.sorted_lines(got) == ke.sorted_lines(ki.golden("real", name)), name
        same(emu, tree, direct, n_u, u, ranks, len(want["text"]) // 2, (name, "half"))
        emu.close()


@pytest.mark.parametrize("order", [0, 1, 2])
def test_injected_counts_of_every_width(lib, order):
    tree = ki.fixture_tree()
    emu = Emu(lib, ki.NODES, ki.NAMES, None, order)
    counts = [1, 9, 10, 99, 100, 10 ** 19, 2 ** 64 - 1, 999999, 1000000]
    ids = sorted(tree.nodes)
    direct = {tid: counts[k % len(counts)] for k, tid in enumerate(ids)}
    direct[999] = 5                                           # no node: nowhere
    for cap in capacities(tree, direct, 2 ** 64 - 1, True, None):
        same(emu, tree, direct, 2 ** 64 - 1, True, None, cap, cap)
    # one taxon alone, every node in turn: every direct[] pattern of one line
    for tid in ids:
        same(emu, tree, {tid: 10}, 0, False, None, 4096, tid)
    emu.close()


@pytest.mark.parametrize("ranks", [None, "superkingdom,phylum,genus,species", "superkingdom,genus,,no rank", "tribe", ""])
def test_the_tables_spell_what_a_walk_with_strings_spells(lib, ranks, tmp_path):
    for nodes, names in ((ki.NODES, ki.NAMES), (ti.REAL_NODES, ti.REAL_NAMES)):
        for order in (0, 2):
            emu = Emu(lib, nodes, names, ranks, order)
            seen = lib.krona_emu_check_tables(emu.h)
            assert seen >= 0, seen
            assert (seen > 0) == (ranks not in ("tribe", "")), (ranks, seen)
            emu.close()


def test_a_deep_chain_with_short_and_long_names(lib, tmp_path):
    """lines longer than a block of the write pass, names of 1 and of about 200 bytes: lines cross every 16-byte phase"""
    nodes, names = ki.chain_tree(64)
    (tmp_path / "nodes.dmp").write_bytes(nodes)
    (tmp_path / "names.dmp").write_bytes(names)
    tree = te.Tree(nodes, names)
    direct = {tid: 1 + tid % 13 for tid in tree.nodes}
    for ranks in (None, "genus,no rank"):
        for order in (0, 2):
            emu = Emu(lib, str(tmp_path / "nodes.dmp"), str(tmp_path / "names.dmp"), ranks, order)
            assert lib.krona_emu_check_tables(emu.h) > 0
            want = ke.expected(tree, direct, 0, False, ranks)
            assert max(len(x) for x in want["text"].split(b"\n")) > 4096 and want["info"]["n_unnamed_taxa"] == 1
            for cap in (len(want["text"]), len(want["text"]) - 1, 5000, 4096, 4095, 0):
                same(emu, tree, direct, 0, False, ranks, cap, (ranks, order, cap))
            emu.close()


def test_the_loader_keeps_the_name_of_a_parent_that_is_no_node(lib):
    """... and only that: the line of 499 in names.dmp changes nothing for a tree that has the node"""
    tree = ki.fixture_tree()
    emu = Emu(lib, ki.NODES, ki.NAMES, None, 0)
    got, _ = emu.text({500: 1, 501: 2}, 0, False, 200)
    assert got in (b"1\tDangling parent\tOrphan genus\n2\tDangling parent\tOrphan genus\tOrphan species\n",
                   b"2\tDangling parent\tOrphan genus\tOrphan species\n1\tDangling parent\tOrphan genus\n")
    emu.close()
    emu = Emu(lib, ki.NODES, ti.NAMES, None, 0)              # the table fixture's names.dmp: 499 has no name
    got, _ = emu.text({500: 1, 501: 2}, 0, False, 200)
    assert ke.sorted_lines(got) == [b"1", b"2\tOrphan genus\tOrphan species"]     # (the genus below the unnamed id prints no name of its own)
    assert got == ke.expected(ti.fixture_tree(), {500: 1, 501: 2})["text"]
    emu.close()


def test_a_list_beyond_the_maximum_is_refused(lib):
    names = C.c_void_p()
    assert lib.kaiju_taxon_names_load(ki.NODES.encode(), ki.NAMES.encode(), api.NAMES_NAME, None, C.byref(names)) == 0
    ok = ",".join("r%d" % k for k in range(64)).encode()
    h = lib.krona_emu_create(names, ok, 0, 1)
    assert h
    lib.krona_emu_free(h)
    assert not lib.krona_emu_create(names, ok + b",one_more", 0, 1)
    lib.kaiju_taxon_names_free(names)
