"""The rule set of kaiju-convertRefSeq (kaiju_amd/csrc/kj_convert.h) on the host: tests/emu/refseq_emu.cpp drives refseq_map_line
and first_entry - what k_am_parse and k_cv_first call per lane - and the passes around them, with the units of every pass in
forward, reversed and shuffled order.  The map and the records must be those of tests/refseq_expect.py (the reference tool pins
that file: tests/test_refseq_expect_golden.py) on the fixtures, on random small inputs, with the first space of a header at
every offset around the 16-byte chunks, and the same text must come out differently under the two rule sets, as the two
models say."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import convert_expect as ce
import refseq_expect as rs
import util
from kaiju_amd import api

NODES = os.path.join(rs.GOLD, "nodes.dmp")
ORDERS = (0, 1, 2)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("refseq_emu") / "librefseq_emu.so")
    src = [os.path.join(util.ROOT, "tests", "emu", "refseq_emu.cpp"), os.path.join(util.ROOT, "kaiju_amd", "csrc", "taxonomy.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", so] + src, check=True)
    L = C.CDLL(so)
    V, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name, res, args in (("cvemu_tree", V, [C.c_char_p]), ("cvemu_tree_free", None, [V]), ("cvemu_map_create", V, [V, V, U64, U64]),
                            ("cvemu_map_free", None, [V]), ("cvemu_map_add", C.c_int, [V, C.c_char_p, U64, C.c_int, C.c_int, U64, C.c_int, U32]),
                            ("rsemu_map_add", C.c_int, [V, C.c_char_p, U64, C.c_int, C.c_int, U32]),
                            ("cvemu_map_lookup", U64, [V, C.c_char_p, U32, V]), ("cvemu_map_stats", None, [V, V]),
                            ("cvemu_conv_create", V, [V, V, U32, V, V, C.c_int]), ("cvemu_conv_free", None, [V]),
                            ("cvemu_convert", C.c_int, [V, C.c_char_p, U64, V, U64, V, C.c_int, U32]),
                            ("rsemu_convert", C.c_int, [V, C.c_char_p, U64, V, U64, V, C.c_int, U32]),
                            ("rsemu_first_space", U64, [C.c_char_p, U64, U64, U64])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def fx():
    return rs.Fixture()


@pytest.fixture(scope="module")
def tree(lib):
    t = lib.cvemu_tree(NODES.encode())
    yield t
    lib.cvemu_tree_free(t)


class Map:
    def __init__(self, L, tree, merged=(), slots=8):
        pairs = np.array([x for p in merged for x in p], dtype=np.uint64)
        self.L, self.h = L, L.cvemu_map_create(tree, pairs.ctypes.data, len(pairs) // 2, slots)

    def add(self, text, first=True, order=0, seed=1):
        assert self.L.rsemu_map_add(self.h, text, len(text), 1 if first else 0, order, seed) == 0
        return self

    def add_nr(self, text, first=True, order=0, seed=1):
        assert self.L.cvemu_map_add(self.h, text, len(text), 1 if first else 0, 0, 0, order, seed) == 0
        return self

    def lookup(self, key):
        probes = C.c_uint32()
        return self.L.cvemu_map_lookup(self.h, key, len(key), C.byref(probes))

    def stats(self):
        out = np.zeros(7, dtype=np.uint64)
        self.L.cvemu_map_stats(self.h, out.ctypes.data)
        return dict(zip(("entries", "slots", "arena", "lines", "no_insert", "duplicates", "rehashes"), (int(x) for x in out)))

    def free(self):
        self.L.cvemu_map_free(self.h)


def blocks_of(text, lines_per_block):
    """the text cut behind line ends, `lines_per_block` lines a block"""
    lines = text.split(b"\n")
    lines = [l + b"\n" for l in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    return [b"".join(lines[k:k + lines_per_block]) for k in range(0, len(lines), lines_per_block)]


def keys_of(text):
    lines = ce.getlines(text)
    return {l.split(b"\t")[0] for l in lines} | {l.split(b"\t")[0][:-1] for l in lines} | {l for l in lines} | {b"nope", b"", b"WP", b"WP_"}


def convert(L, conv, text, out_cap, order, seed=3, fn="rsemu_convert"):
    buf = np.full(out_cap + 64, 0x77, dtype=np.uint8)
    shift = (-buf.ctypes.data) % 16
    info = np.zeros(1, dtype=api.CONVERT_INFO_DTYPE)
    assert getattr(L, fn)(conv, text, len(text), buf.ctypes.data + shift, out_cap, info.ctypes.data, order, seed) == 0
    assert (buf[shift + out_cap:] == 0x77).all() and (buf[:shift] == 0x77).all()
    return bytes(buf[shift:shift + int(info[0]["written_bytes"])]), info[0]


def same(L, conv, want, text, out_cap, order, what, fn="rsemu_convert"):
    got, info = convert(L, conv, text, out_cap, order, fn=fn)
    assert got == want["written"], what
    for f in rs.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f)
    assert int(info["reserved0"]) == 0 and not info["reserved"].any()


def conv_of(L, tree, m, include=rs.DEFAULT_INCLUDE, add_acc=False):
    ids = np.array(include, dtype=np.uint64)
    return L.cvemu_conv_create(tree, ids.ctypes.data, len(ids), m.h, None, 1 if add_acc else 0)


@pytest.mark.parametrize("order", ORDERS)
def test_the_map_of_the_fixture_in_one_block_and_in_blocks_of_a_few_lines(lib, fx, tree, order):
    text = rs.golden("map.tsv")
    for per in (1000, 3, 2, 1):
        m = Map(lib, tree, fx.pairs)
        for k, b in enumerate(blocks_of(text, per)):
            m.add(b, first=k == 0, order=order, seed=k)
        for key in keys_of(text):
            assert m.lookup(key) == fx.model.lookup(key), (per, key)
        st = m.stats()
        assert (st["entries"], st["lines"], st["no_insert"], st["duplicates"]) == (len(fx.model.map), fx.model.lines, fx.model.no_insert, fx.model.duplicates)
        assert st["entries"] * 4 <= st["slots"] * 3 and st["rehashes"] >= 1
        m.free()


@pytest.mark.parametrize("order", ORDERS)
def test_the_first_line_wins_where_a_truncated_key_meets_a_full_one(lib, fx, tree, order):
    """WP_12 (562) and WP_123 (666, merged: the key WP_12, 562 too - so 9606 and 564 stand in to tell the lines apart)"""
    pairs = [(666, 9606)]
    for lines, want in (([b"WP_12\t564", b"WP_123\t666"], 564), ([b"WP_123\t666", b"WP_12\t564"], 9606),
                        ([b"WP_12\t777", b"WP_123\t666", b"WP_12\t564"], 9606), ([b"WP_123\t55555", b"WP_12\t564", b"WP_123\t666"], 564)):
        text = b"\n".join(lines) + b"\n"
        model = rs.Model(fx.nodes, {666: 9606}).add_text(text, first_block=False)
        assert model.lookup(b"WP_12") == want and model.lookup(b"WP_123") == rs.MISS
        for per in (len(lines), 1):                           # in one block, and a line a block
            m = Map(lib, tree, pairs)
            for k, b in enumerate(blocks_of(text, per)):
                m.add(b, first=False, order=order, seed=k)
            assert m.lookup(b"WP_12") == want and m.lookup(b"WP_123") == rs.MISS and m.lookup(b"WP_1") == rs.MISS, (lines, per)
            st = m.stats()
            assert st["entries"] == 1 and st["duplicates"] == model.duplicates and st["no_insert"] == model.no_insert
            m.free()


def test_random_maps_against_the_model(lib, fx, tree):
    rng = random.Random(11)
    taxa = [b"562", b"564", b"1", b"666", b"777", b"4", b"-1", b"", b"0", b"99999999999999999999", b" 2", b"+2157", b"562\r", b"9606x", b"5\x0062"]
    heads = [b"WP_", b"WP_", b"WP_", b"NP_", b"wp_", b"WP", b"W", b""]
    for trial in range(80):
        keys = [rng.choice(heads) + bytes(rng.choice(b"AB. ") for _ in range(rng.choice((0, 1, 2, 12, 13, 14, 30)))) for _ in range(6)]
        keys += [k + b"A" for k in keys[:3]]                 # a key and the key that is longer by a byte: the collision
        lines = [rng.choice(keys) + rng.choice((b"\t", b"\t", b"\t", b"")) + rng.choice(taxa) + rng.choice((b"", b"\t9")) for _ in range(rng.randrange(1, 40))]
        text = b"header\n" + b"\n".join(lines) + rng.choice((b"", b"\n"))
        want = rs.Model(fx.nodes, fx.merged).add_text(text)
        for order in ORDERS:
            m = Map(lib, tree, fx.pairs)
            for k, b in enumerate(blocks_of(text, rng.randrange(1, 6))):
                m.add(b, first=k == 0, order=order, seed=trial)
            for key in keys + [k[:-1] for k in keys if k] + [b"zz"]:
                assert m.lookup(key) == want.lookup(key), (trial, order, key, text)
            st = m.stats()
            assert (st["entries"], st["lines"], st["no_insert"], st["duplicates"]) == (len(want.map), want.lines, want.no_insert, want.duplicates)
            m.free()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(rs.SETS))
def test_the_fixtures_at_every_capacity(lib, fx, tree, name, order):
    a, l = rs.SETS[name]
    m = Map(lib, tree, fx.pairs).add(rs.golden("map.tsv"), order=order)
    conv = conv_of(lib, tree, m, fx.listed if l else rs.DEFAULT_INCLUDE, a)
    full = fx.expected(name)
    assert rs.file_of(full["text"]) == rs.golden("out_%s.txt" % name)
    caps, at = {0, len(full["text"]) + 40}, 0
    for r in full["records"]:
        at += len(r)
        caps |= {at - 1, at, at + 1}
    for cap in sorted(caps):
        same(lib, conv, fx.expected(name, out_cap=cap), fx.faa, cap, order, (name, cap))
    same(lib, conv, fx.expected(name, text=fx.faa_none, out_cap=16), fx.faa_none, 16, order, "none")
    same(lib, conv, fx.expected(name, text=b"", out_cap=16), b"", 16, order, "empty")
    lib.cvemu_conv_free(conv)
    m.free()


def test_random_texts_against_the_model(lib, fx, tree):
    m = Map(lib, tree, fx.pairs).add(rs.golden("map.tsv"))
    conv = conv_of(lib, tree, m, add_acc=True)
    rng = random.Random(23)
    accs = [b"WP_1.1", b"WP_5.", b"WP_5.1", b"WP", b"WP_", b"", b"ZZ", b"WP_H.1", b"WP_B1.1", b"WP_\x011.1", b"WP_R1", b"WP_K"]
    model = lambda t, cap=None: rs.convert(fx.nodes, rs.DEFAULT_INCLUDE, fx.model.map, t, add_acc=True, out_cap=cap)
    for trial in range(150):
        lines = []
        for _ in range(rng.randrange(0, 8)):
            kind = rng.randrange(5)
            if kind == 0:
                lines.append(b">" + rng.choice(accs) + rng.choice((b" d", b"", b" ", b" a b", b"\x01WP_1.1 x", b" x\x01WP_1.1 y", b"\r")))
            elif kind == 1:
                lines.append(b"")
            else:
                lines.append(bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYXBJOUZacd*-\r") for _ in range(rng.randrange(0, 70))))
        text = b"\n".join(lines) + rng.choice((b"", b"\n"))
        n = len(model(text)["text"])
        for cap in {0, n, max(0, n - 1), n // 2}:
            same(lib, conv, model(text, cap), text, cap, trial % 3, (trial, cap, text))
    lib.cvemu_conv_free(conv)
    m.free()


SPACE_AT = (15, 16, 17, 31, 32, 33)


def test_the_first_space_around_the_chunk_boundaries(lib, fx, tree):
    """the first space of a header at line offsets 15 .. 33, the line starting at every residue mod 16: found where it is, and
    the accession in front of it is the one looked up; a second space, a space in the line in front and one behind the line end
    change nothing"""
    keys = {at: b"WP_" + b"K" * (at - 4) for at in SPACE_AT}                 # '>' + the key: the space is byte `at` of the line
    m = Map(lib, tree, fx.pairs).add(b"".join(b"%s\t%d\n" % (k, 562 if at & 1 else 564) for at, k in keys.items()), first=False)
    conv = conv_of(lib, tree, m, add_acc=True)
    amap = {k: (562 if at & 1 else 564) for at, k in keys.items()}
    for start in range(16):
        lead = (b"A" * (start - 1) + b"\n") if start else b""                # sequence lines in front of the first header: dropped
        for at in SPACE_AT:
            line = b">" + keys[at] + b" d e"
            for text in (lead + line + b"\nACD\n", lead + line[:at + 1] + b"\nACD\n", lead + line[:at] + b"\n x y\n", lead + line[:at]):
                e = text.find(b"\n", start) if text.find(b"\n", start) >= 0 else len(text)
                want_sp = start + at if start + at < e else e
                assert lib.rsemu_first_space(text, len(text), start, e) == want_sp, (start, at, text)
                want = rs.convert(fx.nodes, rs.DEFAULT_INCLUDE, amap, text, add_acc=True)
                assert want["info"]["n_hits"] == (1 if want_sp < e else 0)
                same(lib, conv, want, text, len(want["text"]), (start + at) % 3, (start, at, text))
    lib.cvemu_conv_free(conv)
    m.free()


def test_one_text_under_both_rule_sets(lib, fx, tree):
    """the fixture's map file and text through the rules of kaiju-convertNR and through those of kaiju-convertRefSeq: each gives
    what its model says, and the two differ"""
    text, faa = rs.golden("map.tsv"), fx.faa + b"\n>ZZ.1 unknown\x01WP_1.1 known\nFFFF\n>WP_4C.1 column two\nAAAD\n"
    nr_model = ce.Model(fx.nodes, fx.merged).add_text(text)
    m_rs, m_nr = Map(lib, tree, fx.pairs).add(text), Map(lib, tree, fx.pairs).add_nr(text)
    for key in keys_of(text):
        assert m_rs.lookup(key) == fx.model.lookup(key) and m_nr.lookup(key) == nr_model.lookup(key), key
    assert m_rs.lookup(b"WP_5.") == 562 and m_nr.lookup(b"WP_5.") == rs.MISS and m_nr.lookup(b"WP_4C.1") == 562 and m_rs.lookup(b"WP_4C.1") == rs.MISS
    c_rs, c_nr = conv_of(lib, tree, m_rs, add_acc=True), conv_of(lib, tree, m_nr, add_acc=True)
    want_rs = rs.convert(fx.nodes, rs.DEFAULT_INCLUDE, fx.model.map, faa, add_acc=True)
    want_nr = ce.convert(fx.nodes, rs.DEFAULT_INCLUDE, nr_model.map, set(), faa, add_acc=True)
    # (under the NR rules the accession of a two-column line is its second column: only the four-column line gives a key of the text)
    assert want_nr["text"] == b">WP_4C.1_562\nAAAD\n" * 2 and b"WP_4C" not in want_rs["text"] and want_rs["info"]["n_kept"] == 19
    for order in ORDERS:
        same(lib, c_rs, want_rs, faa, len(want_rs["text"]), order, "refseq")
        same(lib, c_nr, want_nr, faa, len(want_nr["text"]), order, "nr", fn="cvemu_convert")
    # the header rules alone, over the one map: the loop over '\x01' of the NR rules finds "WP_1.1" behind "ZZ.1 unknown", the
    # RefSeq rules look up "ZZ.1" and drop the record
    want_loop = ce.convert(fx.nodes, rs.DEFAULT_INCLUDE, fx.model.map, set(), faa, add_acc=True)
    assert b">WP_1.1_562\nFFFF\n" in want_loop["text"] and b"FFFF" not in want_rs["text"]
    same(lib, c_rs, want_loop, faa, len(want_loop["text"]), 2, "the NR header rules over the RefSeq map", fn="cvemu_convert")
    same(lib, c_nr, rs.convert(fx.nodes, rs.DEFAULT_INCLUDE, nr_model.map, faa, add_acc=True), faa, 4096, 2, "the RefSeq header rules over the NR map")
    for c in (c_rs, c_nr):
        lib.cvemu_conv_free(c)
    for m in (m_rs, m_nr):
        m.free()
