"""kaiju-convertNR (kaiju_amd/csrc/kj_convert.h) on the host: tests/emu/convert_emu.cpp drives the per-lane functions the
kernels of accmap.hip and convert.hip are made of, pass by pass, with the units of every pass in forward, reversed and shuffled
order.  The map and the records must be those of tests/convert_expect.py (the reference tool pins that file:
tests/test_convert_expect_golden.py) on the fixtures and on random small inputs; the local entry rule must give the entries of
the sequential loop, and the fold of the pairwise LCA the LCA of the set in every order."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import convert_expect as ce
import util
from kaiju_amd import api

NODES = os.path.join(ce.GOLD, "nodes.dmp")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("convert_emu") / "libconvert_emu.so")
    src = [os.path.join(util.ROOT, "tests", "emu", "convert_emu.cpp"), os.path.join(util.ROOT, "kaiju_amd", "csrc", "taxonomy.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", so] + src, check=True)
    L = C.CDLL(so)
    V, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name, res, args in (("cvemu_tree", V, [C.c_char_p]), ("cvemu_tree_free", None, [V]), ("cvemu_map_create", V, [V, V, U64, U64]),
                            ("cvemu_map_free", None, [V]), ("cvemu_map_add", C.c_int, [V, C.c_char_p, U64, C.c_int, C.c_int, U64, C.c_int, U32]),
                            ("cvemu_map_lookup", U64, [V, C.c_char_p, U32, V]), ("cvemu_map_stats", None, [V, V]), ("cvemu_strtoul", U64, [C.c_char_p, U64]),
                            ("cvemu_hash", U64, [C.c_char_p, U32]), ("cvemu_entries", U32, [C.c_char_p, U64, V, V, U32, C.c_int, U32]),
                            ("cvemu_lca_fold", U64, [V, V, U32]), ("cvemu_conv_create", V, [V, V, U32, V, V, C.c_int]), ("cvemu_conv_free", None, [V]),
                            ("cvemu_convert", C.c_int, [V, C.c_char_p, U64, V, U64, V, C.c_int, U32])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def fx():
    return ce.Fixture()


class Map:
    def __init__(self, L, tree, merged=(), slots=8):
        pairs = np.array([x for p in merged for x in p], dtype=np.uint64)
        self.L, self.h = L, L.cvemu_map_create(tree, pairs.ctypes.data, len(pairs) // 2, slots)

    def add(self, text, first=True, keys=False, value=1, order=0, seed=1):
        assert self.L.cvemu_map_add(self.h, text, len(text), 1 if first else 0, 1 if keys else 0, value, order, seed) == 0
        return self

    def lookup(self, key):
        probes = C.c_uint32()
        return self.L.cvemu_map_lookup(self.h, key, len(key), C.byref(probes))

    def stats(self):
        out = np.zeros(7, dtype=np.uint64)
        self.L.cvemu_map_stats(self.h, out.ctypes.data)
        return dict(zip(("entries", "slots", "arena", "lines", "no_insert", "duplicates", "rehashes"), (int(x) for x in out)))


def blocks_of(text, sizes):
    """the text cut behind line ends, into blocks of about the sizes given in turn"""
    out, at, k = [], 0, 0
    while at < len(text):
        end = text.find(b"\n", min(len(text) - 1, at + sizes[k % len(sizes)])) + 1
        end = end if end > 0 else len(text)
        out.append(text[at:end])
        at, k = end, k + 1
    return out


def keys_of(text):
    return {ce.map_line(l)[0] for l in ce.getlines(text)} | {l for l in ce.getlines(text)} | {b"nope", b""}


def convert(L, conv, text, out_cap, order, seed=3):
    buf = np.full(out_cap + 64, 0x77, dtype=np.uint8)
    shift = (-buf.ctypes.data) % 16
    info = np.zeros(1, dtype=api.CONVERT_INFO_DTYPE)
    assert L.cvemu_convert(conv, text, len(text), buf.ctypes.data + shift, out_cap, info.ctypes.data, order, seed) == 0
    assert (buf[shift + out_cap:] == 0x77).all() and (buf[:shift] == 0x77).all()
    return bytes(buf[shift:shift + int(info[0]["written_bytes"])]), info[0]


def same(L, conv, want, text, out_cap, order, what):
    got, info = convert(L, conv, text, out_cap, order)
    assert got == want["written"], what
    for f in ce.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f)
    assert int(info["reserved0"]) == 0 and not info["reserved"].any()


@pytest.mark.parametrize("order", [0, 1, 2])
def test_the_map_of_the_fixture_in_one_block_and_in_many(lib, fx, order):
    tree = lib.cvemu_tree(NODES.encode())
    text = ce.golden("map.tsv")
    pairs = ce.merged_pairs(ce.golden("merged.dmp"))
    for sizes in ([len(text)], [40, 1, 90], [1]):
        m = Map(lib, tree, pairs)
        for k, b in enumerate(blocks_of(text, sizes)):
            m.add(b, first=k == 0, order=order, seed=k)
        for key in keys_of(text):
            assert m.lookup(key) == fx.model.lookup(key), (sizes, key)
        st = m.stats()
        assert (st["entries"], st["lines"], st["no_insert"], st["duplicates"]) == (len(fx.model.map), fx.model.lines, fx.model.no_insert, fx.model.duplicates)
        assert st["entries"] * 4 <= st["slots"] * 3 and st["rehashes"] >= 1
        lib.cvemu_map_free(m.h)
    lib.cvemu_tree_free(tree)


def test_random_maps_first_inserting_line_wins_in_every_order(lib, fx):
    tree = lib.cvemu_tree(NODES.encode())
    rng = random.Random(11)
    taxa = [b"562", b"564", b"1", b"666", b"777", b"4", b"-1", b"", b"99999999999999999999", b" 2", b"+2157"]
    for trial in range(60):
        keys = [bytes(rng.choice(b"AB.") for _ in range(rng.choice((0, 1, 2, 15, 16, 17, 33)))) for _ in range(6)]
        lines = [b"x\t" + rng.choice(keys) + b"\t" + rng.choice(taxa) + rng.choice((b"", b"\t9", b"\r")) for _ in range(rng.randrange(1, 40))]
        text = b"header\n" + b"\n".join(lines) + rng.choice((b"", b"\n"))
        want = ce.Model(fx.nodes, fx.merged).add_text(text)
        for order in (0, 1, 2):
            m = Map(lib, tree, ce.merged_pairs(ce.golden("merged.dmp")))
            for k, b in enumerate(blocks_of(text, [rng.randrange(1, 60)])):
                m.add(b, first=k == 0, order=order, seed=trial)
            for key in keys + [b"zz"]:
                assert m.lookup(key) == want.lookup(key), (trial, order, key, text)
            assert m.stats()["duplicates"] == want.duplicates
            lib.cvemu_map_free(m.h)
    lib.cvemu_tree_free(tree)


def test_keys_of_every_length_class_and_a_wrapping_probe(lib):
    tree = lib.cvemu_tree(NODES.encode())
    keys = [b"", b"A", b"A" * 15, b"A" * 16, b"A" * 17, b"A" * 33, b"A" * 32 + b"B", b"A\x00", b"B" * 16 + b"C"]
    m = Map(lib, tree, slots=8).add(b"".join(b"k\t%s\t%d\n" % (k, 561 + (i & 1)) for i, k in enumerate(keys)), first=False)
    for i, k in enumerate(keys):
        assert m.lookup(k) == 561 + (i & 1), k
    for k in (b"AA", b"A" * 14, b"A" * 18, b"A" * 32 + b"C", b"B" * 16):
        assert m.lookup(k) == ce.MISS, k
    lib.cvemu_map_free(m.h)
    # six keys whose home is one of the last two of eight slots: the probes wrap around the end
    for key in keys + [b"W%d" % k for k in range(300)]:
        assert lib.cvemu_hash(key, len(key)) == ce.key_hash(key), key
    found = ce.keys_with_late_homes(6)
    m = Map(lib, tree, slots=8).add(b"".join(b"k\t%s\t562\n" % key for key in found), first=False)
    st = m.stats()
    assert st["slots"] == 8 and st["entries"] == 6 and st["rehashes"] == 0
    assert all(m.lookup(key) == 562 for key in found) and m.lookup(b"W") == ce.MISS
    lib.cvemu_map_free(m.h)
    lib.cvemu_tree_free(tree)


def test_strtoul_of_a_field(lib):
    for text in (b"562", b"  +7x", b"-1", b"", b"abc", b"18446744073709551615", b"18446744073709551616", b"-18446744073709551054", b"\t\r 12\t3", b"- 5",
                 b"5\x006", b"00000000000000000000000012", b"+-3", b"18446744073709551614"):
        assert lib.cvemu_strtoul(text, len(text)) == ce.strtoul(text), text


@pytest.mark.parametrize("order", [0, 2])
def test_the_local_entry_rule_is_the_sequential_one(lib, fx, order):
    rng = random.Random(7)
    lines = [l for l in ce.getlines(fx.nr) if l[:1] == b">"]
    lines += [b">" + bytes(rng.choice(b"\x01\x01  ab>") for _ in range(rng.randrange(0, 40))) for _ in range(1500)]
    start, end = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint32)
    for line in lines:
        n = lib.cvemu_entries(line, len(line), start.ctypes.data, end.ctypes.data, 64, order, 5)
        assert [(int(start[k]), int(end[k])) for k in range(n)] == ce.entries_sequential(line), line


def test_the_fold_of_the_pairwise_lca_is_the_lca_of_the_set(lib, fx):
    tree = lib.cvemu_tree(NODES.encode())
    rng = random.Random(3)
    ids = sorted(fx.nodes)
    for _ in range(400):
        pick = [rng.choice(ids) for _ in range(rng.randrange(1, 7))]
        want = ce.lca(fx.nodes, set(pick))
        for _ in range(4):
            rng.shuffle(pick)
            a = np.array(pick, dtype=np.uint64)
            assert lib.cvemu_lca_fold(tree, a.ctypes.data, len(a)) == want, pick
    lib.cvemu_tree_free(tree)


def test_two_roots_drop_the_record_and_count_it(lib, tmp_path):
    nodes = b"1\t|\t1\t|\n2\t|\t1\t|\n5\t|\t5\t|\n6\t|\t5\t|\n7\t|\t40\t|\n"
    (tmp_path / "nodes.dmp").write_bytes(nodes)
    tree = lib.cvemu_tree(str(tmp_path / "nodes.dmp").encode())
    tn = ce.parse_pairs(nodes)
    m = Map(lib, tree).add(b"k\tA\t2\nk\tB\t6\nk\tC\t7\n", first=False)
    ids = np.array([2, 5, 7], dtype=np.uint64)
    conv = lib.cvemu_conv_create(tree, ids.ctypes.data, 3, m.h, None, 0)
    text = b">A x\x01B y\nAAA\n>B x\nCCC\n>A x\nDDD\n>C x\x01A y\nEEE\n>C x\nFFF\n"
    want = ce.convert(tn, (2, 5, 7), {b"A": 2, b"B": 6, b"C": 7}, set(), text)
    assert want["text"] == b">6\nCCC\n>2\nDDD\n>7\nFFF\n" and want["info"]["dropped_no_lca"] == 2
    for order in (0, 1, 2):
        same(lib, conv, want, text, 64, order, order)
    lib.cvemu_conv_free(conv)
    lib.cvemu_map_free(m.h)
    lib.cvemu_tree_free(tree)


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(ce.SETS))
def test_the_fixtures_at_every_capacity(lib, fx, name, order):
    a, l, e = ce.SETS[name]
    tree = lib.cvemu_tree(NODES.encode())
    m = Map(lib, tree, ce.merged_pairs(ce.golden("merged.dmp"))).add(ce.golden("map.tsv"), order=order)
    x = Map(lib, None).add(ce.golden("excl.txt"), first=False, keys=True, order=order)
    ids = np.array(fx.listed if l else ce.DEFAULT_INCLUDE, dtype=np.uint64)
    conv = lib.cvemu_conv_create(tree, ids.ctypes.data, len(ids), m.h, x.h if e else None, 1 if a else 0)
    full = fx.expected(name)
    assert ce.file_of(full["text"]) == ce.golden("out_%s.txt" % name)
    caps, at = {0, len(full["text"]) + 40}, 0
    for r in full["records"]:
        at += len(r)
        caps |= {at - 1, at, at + 1}
    for cap in sorted(caps):
        same(lib, conv, fx.expected(name, out_cap=cap), fx.nr, cap, order, (name, cap))
    same(lib, conv, fx.expected(name, text=fx.nr_none, out_cap=16), fx.nr_none, 16, order, "none")
    same(lib, conv, fx.expected(name, text=b"", out_cap=16), b"", 16, order, "empty")
    lib.cvemu_conv_free(conv)
    for h in (m.h, x.h):
        lib.cvemu_map_free(h)
    lib.cvemu_tree_free(tree)


def test_random_texts_and_long_sequences(lib, fx):
    tree = lib.cvemu_tree(NODES.encode())
    m = Map(lib, tree, ce.merged_pairs(ce.golden("merged.dmp"))).add(ce.golden("map.tsv"))
    x = Map(lib, None).add(ce.golden("excl.txt"), first=False, keys=True)
    conv = lib.cvemu_conv_create(tree, np.array(ce.DEFAULT_INCLUDE, dtype=np.uint64).ctypes.data, 3, m.h, x.h, 1)
    rng = random.Random(23)
    accs = [b"A1.1", b"A2.1", b"A3.1", b"A4.1", b"E1.1", b"ZZ", b"", b"B1.1", b"B3.1", b"V\x011.1"]
    for trial in range(150):
        lines = []
        for _ in range(rng.randrange(0, 8)):
            kind = rng.randrange(5)
            if kind == 0:
                lines.append(b">" + b"\x01".join(rng.choice(accs) + rng.choice((b" d", b"", b" ", b" a b")) for _ in range(rng.randrange(0, 5))))
            elif kind == 1:
                lines.append(b"")
            else:
                lines.append(bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYXBJOUZacd*-\r") for _ in range(rng.randrange(0, 70))))
        text = b"\n".join(lines) + rng.choice((b"", b"\n"))
        full = ce.convert(fx.nodes, ce.DEFAULT_INCLUDE, fx.model.map, fx.excluded, text, add_acc=True)
        for cap in {0, len(full["text"]), max(0, len(full["text"]) - 1), len(full["text"]) // 2}:
            same(lib, conv, ce.convert(fx.nodes, ce.DEFAULT_INCLUDE, fx.model.map, fx.excluded, text, add_acc=True, out_cap=cap), text, cap, trial % 3, (trial, cap, text))
    # 40 000 letters on one line and on 700 lines, a header of 3000 entries beside headers of one
    seq = bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYXx") for _ in range(40000))
    big = b">A1.1 x\x01A2.1 y\x01" + b"\x01".join(rng.choice((b"A1.1 x", b"A2.1 y", b"ZZ.9 z")) for _ in range(2998))
    text = b">A1.1 one line\n" + seq + b"\n>A2.1 many\n" + b"\n".join(seq[k:k + 58] for k in range(0, len(seq), 58)) + b"\n" + big + b"\nACD\n>A3.1 z\nEFG\n"
    full = ce.convert(fx.nodes, ce.DEFAULT_INCLUDE, fx.model.map, fx.excluded, text, add_acc=True)
    assert full["info"]["n_kept"] == 4 and full["info"]["n_entries"] == 3003 and b">A1.1_561\nACD\n" in full["text"]
    for cap, order in ((len(full["text"]), 0), (len(full["text"]), 2), (len(full["text"]) - 1, 1), (50000, 2)):
        same(lib, conv, ce.convert(fx.nodes, ce.DEFAULT_INCLUDE, fx.model.map, fx.excluded, text, add_acc=True, out_cap=cap), text, cap, order, cap)
    lib.cvemu_conv_free(conv)
    for h in (m.h, x.h):
        lib.cvemu_map_free(h)
    lib.cvemu_tree_free(tree)
