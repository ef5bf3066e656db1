"""The tally (kaiju_amd/csrc/kj_tally.h) on the host: tests/emu/tally_emu.cpp drives the per-lane functions the kernels of
tally.hip are made of, pass by pass, with the work units of every pass in forward, reversed and shuffled order.  The fixture
the reference tool read, random texts over the fixture tree and a text cut at every byte offset must give the counts and
entries of tests/table_expect.py (the reference tool pins that file: tests/test_table_expect_golden.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import table_expect as te
import table_inputs as ti
import util
from kaiju_amd import api


def build_tally_emu(directory):
    so = str(directory / "libtally_emu.so")
    src = [os.path.join(util.ROOT, "tests", "emu", "tally_emu.cpp"), os.path.join(util.ROOT, "kaiju_amd", "csrc", "taxon_names.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", so] + src, check=True)
    L = C.CDLL(so)
    L.kaiju_taxon_names_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_void_p]
    L.kaiju_taxon_names_free.argtypes = [C.c_void_p]
    L.tally_emu_constants.argtypes = [C.c_void_p]
    L.tally_emu_create.restype = C.c_void_p
    L.tally_emu_create.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.tally_emu_free.argtypes = [C.c_void_p]
    L.tally_emu_spilled.restype = C.c_uint64
    L.tally_emu_spilled.argtypes = [C.c_void_p]
    L.tally_emu_reset.argtypes = [C.c_void_p]
    L.tally_emu_add.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_uint32]
    L.tally_emu_result.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32]
    return L


class Emu:
    def __init__(self, L, nodes, names, order):
        self.L, self.order = L, order
        self.names = C.c_void_p()
        assert L.kaiju_taxon_names_load(nodes.encode(), names.encode(), api.NAMES_NAME, None, C.byref(self.names)) == 0
        self.h = L.tally_emu_create(self.names, order, 7)

    def add(self, text, final=True):
        info = np.zeros(1, dtype=api.TALLY_INFO_DTYPE)
        assert self.L.tally_emu_add(self.h, text, len(text), 1 if final else 0, info.ctypes.data, self.order, 11) == 0
        return info[0]

    def reset(self):
        self.L.tally_emu_reset(self.h)

    def result(self, cap=4096):
        ent = np.zeros(cap, dtype=api.TALLY_ENTRY_DTYPE)
        n = C.c_uint64()
        totals = np.zeros(1, dtype=api.TALLY_INFO_DTYPE)
        rc = self.L.tally_emu_result(self.h, ent.ctypes.data, cap, C.byref(n), totals.ctypes.data, self.order, 13)
        return rc, ent[:min(n.value, cap)], totals[0], n.value

    def close(self):
        self.L.tally_emu_free(self.h)
        self.L.kaiju_taxon_names_free(self.names)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = build_tally_emu(tmp_path_factory.mktemp("tally_emu"))
    k = np.zeros(6, dtype=np.uint32)
    L.tally_emu_constants(k.ctypes.data)
    assert [int(x) for x in k] == [4096, 16, 32, 56, ti.TABLE_SLOTS, ti.COUNT_SHARE]
    return L


@pytest.fixture(scope="module", params=[0, 1, 2])
def emu(lib, request):
    e = Emu(lib, ti.NODES, ti.NAMES, request.param)
    yield e
    e.close()


def same_info(info, want, what):
    for f in te.INFO_FIELDS:
        assert int(info[f]) == want[f], (what, f, int(info[f]), want[f])


def same_entries(ent, want, what):
    got = sorted((int(e["taxon"]), int(e["direct"]), int(e["summed"]), int(e["virus"])) for e in ent)
    assert got == want, what
    assert not np.any(ent["reserved"])


def check(emu, texts, what):
    """texts: added one behind the other, all but the last one with final=0 and the rest carried as a caller would"""
    tree = ti.fixture_tree()
    emu.reset()
    carry, whole = b"", b"".join(texts)
    for k, t in enumerate(texts):
        final = k + 1 == len(texts)
        info = emu.add(carry + t, final)
        same_info(info, te.count_text(tree, carry + t, final)[0], (what, "call", k))
        carry = (carry + t)[int(info["used"]):]
    totals, entries = te.tally(tree, [whole])
    rc, ent, tot, n = emu.result()
    assert rc == 0 and n == len(entries)
    for f in te.INFO_FIELDS[2:]:
        assert int(tot[f]) == totals[f], (what, f)
    assert int(tot["used"]) == len(whole)
    same_entries(ent, entries, what)


def test_the_odd_fixture_and_the_two_small_files(emu):
    for label, text in ti.fixture_texts():
        check(emu, [text], label)


def test_random_texts_over_the_fixture_tree(emu):
    rng = np.random.default_rng(5)
    for k in range(6):
        check(emu, [ti.random_text(rng, ti.fixture_tree(), 50 + 97 * k, final_newline=bool(k & 1))], "random %d" % k)


def test_a_text_cut_at_every_byte_offset_counts_the_same(emu):
    text = ti.read(os.path.join(ti.TABLE, "odd", "in.tsv"))
    text = text[:600] + text[-300:]                     # lines of every kind, no final newline
    tree = ti.fixture_tree()
    totals, entries = te.tally(tree, [text])
    for cut in range(len(text) + 1):
        emu.reset()
        first = emu.add(text[:cut], final=False)
        used = int(first["used"])
        assert used == text[:cut].rfind(b"\n") + 1
        emu.add(text[used:], final=True)
        rc, ent, tot, _ = emu.result()
        assert rc == 0
        for f in te.INFO_FIELDS[2:]:
            assert int(tot[f]) == totals[f], (cut, f)
        assert int(tot["used"]) == len(text)
        same_entries(ent, entries, cut)


def test_more_taxa_in_a_block_than_its_table_holds(lib, tmp_path):
    """one block, more different taxa than the table has slots: the lines that find no room are counted by their lanes"""
    nodes, names = ti.many_taxa_tree(ti.WIDE_TAXA)
    (tmp_path / "nodes.dmp").write_bytes(nodes)
    (tmp_path / "names.dmp").write_bytes(names)
    tree = te.Tree(nodes, names)
    for order in (0, 2):
        e = Emu(lib, str(tmp_path / "nodes.dmp"), str(tmp_path / "names.dmp"), order)
        for what, text in ti.table_shapes().items():
            before = lib.tally_emu_spilled(e.h)
            e.reset()
            info = e.add(text)
            totals, entries = te.tally(tree, [text])
            rc, ent, tot, n = e.result(cap=8192)
            assert rc == 0 and n == len(entries), what
            same_entries(ent, entries, what)
            for f in te.INFO_FIELDS:
                assert int(info[f]) == int(tot[f]) == totals[f], (what, f)
            spilled = lib.tally_emu_spilled(e.h) - before
            assert (spilled > 0) == (what != "fits_the_table"), (what, spilled)
        e.close()


def test_more_entries_than_room_is_said_and_nothing_is_written(emu):
    emu.reset()
    emu.add(ti.fixture_texts()[0][1])
    rc, ent, _, n = emu.result(cap=3)
    assert rc == -2 and n > 3 and not np.any(ent["taxon"])
    emu.reset()
    rc, ent, tot, n = emu.result()
    assert rc == 0 and n == 0 and int(tot["n_total"]) == 0
