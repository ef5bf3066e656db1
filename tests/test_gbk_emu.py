"""kaiju-gbk2faa (kaiju_amd/csrc/kj_gbk.h) on the host: tests/emu/gbk_emu.cpp drives the per-lane functions the kernels of
gbk.hip are made of, pass by pass, with the units of every pass in forward, reversed and shuffled order.  Kinds, captures,
output, counts and the carried state must be those of tests/gbk_expect.py (the script pins that file:
tests/test_gbk_expect_golden.py): on the fixtures whole and with a cut behind every line, on generated lines, at every
capacity around every end of an output line with guard bytes behind it, and the state must stay where it was after an
overflow."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import gbk_expect as ge
import util
from kaiju_amd import api

ORDERS = [0, 1, 2]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gbk_emu") / "libgbk_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", so, os.path.join(util.ROOT, "tests", "emu", "gbk_emu.cpp")], check=True)
    L = C.CDLL(so)
    V, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name, res, args in (("gbemu_create", V, []), ("gbemu_free", None, [V]), ("gbemu_reset", None, [V]), ("gbemu_state", None, [V, V, V, V, U64]),
                            ("gbemu_classify", U32, [C.c_char_p, U64, V]), ("gbemu_convert", C.c_int, [V, C.c_char_p, U64, V, U64, V, C.c_int, U32])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


class Emu:
    def __init__(self, L):
        self.L, self.h = L, L.gbemu_create()

    def state(self):
        st = np.zeros(3, dtype=np.uint32)
        tax, pid = np.zeros(1 << 16, dtype=np.uint8), np.zeros(1 << 16, dtype=np.uint8)
        self.L.gbemu_state(self.h, st.ctypes.data, tax.ctypes.data, pid.ctypes.data, len(tax))
        return ge.State(bytes(tax[:st[0]]) or None, bytes(pid[:st[1]]) or None, bool(st[2]))

    def convert(self, text, out_cap, order, seed=3):
        buf = np.full(out_cap + 64, 0x77, dtype=np.uint8)
        shift = (-buf.ctypes.data) % 16
        info = np.zeros(1, dtype=api.GBK_INFO_DTYPE)
        assert self.L.gbemu_convert(self.h, text, len(text), buf.ctypes.data + shift, out_cap, info.ctypes.data, order, seed) == 0
        assert (buf[shift + out_cap:] == 0x77).all() and (buf[:shift] == 0x77).all()          # the guard bytes
        n = int(info[0]["written_bytes"])
        assert (buf[shift + n:] == 0x77).all()
        return bytes(buf[shift:shift + n]), info[0]

    def close(self):
        self.L.gbemu_free(self.h)


def same(emu, want, text, out_cap, order, what):
    got, info = emu.convert(text, out_cap, order)
    assert got == want["written"], what
    for f in ge.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f)
    assert [int(x) for x in info["lines_kind"]] == want["kinds"], what
    assert int(info["reserved0"]) == 0 and not info["reserved"].any()
    assert emu.state() == want["state"], what


@pytest.fixture()
def emu(lib):
    e = Emu(lib)
    yield e
    e.close()


def test_kinds_and_captures_line_by_line(lib):
    rng = random.Random(11)
    lines = [l for name in ge.FIXTURES for l in ge.getlines(ge.golden(name + ".gbk"))]
    lines += ge.getlines(ge.random_text(rng, 3000, taxon_first=False))
    lines += [b' /translation="' + b"ACDX" * 40 + b'" tail', b"x" * 37 + b' /protein_id="' + b"p" * 50 + b'"', b'"', b"", b'/db_xref="taxon:1"', b'/db_xref="taxon:1',
              b'/protein_id="a"', b'\t/translation="a', b'\t/translation="a"', b' /translation="a""', b' /translation="a" "']
    cap = np.zeros(2, dtype=np.uint32)
    seen = set()
    for line in lines:
        kind, want = ge.kind_of(line)
        got = lib.gbemu_classify(line, len(line), cap.ctypes.data)
        assert got & 7 == kind and bool(got & 8) == (b'"' in line), line
        if kind < 5:
            assert line[cap[0]:cap[1]] == want, line
        seen.add(kind)
    assert seen == {1, 2, 3, 4, 5}


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ge.FIXTURES)
def test_the_fixtures_whole_and_cut_behind_every_line(emu, name, order):
    text = ge.golden(name + ".gbk")
    full = ge.convert(text)
    same(emu, full, text, len(full["text"]) + 5, order, name)
    assert ge.convert_file(text)[0] == ge.golden(name + ".faa")
    cuts = ge.cuts_behind_lines(text)
    for cut in cuts:                                           # two blocks, the cut behind every line in turn
        emu.L.gbemu_reset(emu.h)
        st = ge.State()
        for block in (text[:cut], text[cut:]):
            want = ge.convert(block, st)
            same(emu, want, block, len(want["text"]), order, (name, cut))
            st = want["state"]
    emu.L.gbemu_reset(emu.h)                                   # every line a block of its own
    st, out = ge.State(), []
    for a, e in zip([0] + cuts, cuts + [len(text)]):
        want = ge.convert(text[a:e], st)
        same(emu, want, text[a:e], len(want["text"]), order, (name, a))
        if want["info"]["no_taxon_line"]:                      # (where the script dies; its file is empty)
            out = []
            break
        st = want["state"]
        out.append(want["text"])
    assert b"".join(out) == ge.golden(name + ".faa")


@pytest.mark.parametrize("order", ORDERS)
def test_capacities_around_every_line_end_and_the_state_after_an_overflow(emu, order):
    text = ge.golden("rules.gbk")
    cut = text.index(b"HIK xyz")                               # inside a translation, a taxon and a protein id carried in
    first = ge.convert(text[:cut])
    second = ge.convert(text[cut:], first["state"])
    ends = []
    for o in second["lines"]:
        ends.append((ends[-1] if ends else 0) + len(o))
    caps = sorted({0, len(second["text"])} | {max(0, e + d) for e in ends for d in (-1, 0, 1)})
    assert len(caps) > 3 * len(second["lines"]) - 4
    for cap in caps:
        emu.L.gbemu_reset(emu.h)
        same(emu, first, text[:cut], len(first["text"]), order, "first")
        want = ge.convert(text[cut:], first["state"], out_cap=cap)
        same(emu, want, text[cut:], cap, order, cap)           # (the state is compared in there: untouched when it overflows)
        if want["info"]["overflow"]:
            assert want["state"] == first["state"]
            again = ge.convert(text[cut:], first["state"])
            same(emu, again, text[cut:], want["info"]["text_bytes"], order, ("again", cap))


@pytest.mark.parametrize("order", ORDERS)
def test_generated_text_across_scan_blocks_and_write_blocks(emu, order):
    rng = random.Random(17)
    big = ge.genbank_text(rng, 6, origin_lines=120, taxon_digits=25, pid_len=300) + ge.genbank_text(rng, 2, pid_len=1)
    long_line = b' /translation="' + bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYXBZ") for _ in range(5000)) + b'"\n'
    many = b' /translation="' + b"\n".join(bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYx ") for _ in range(rng.randrange(0, 70))) for _ in range(700)) + b'"\n'
    text = b'/db_xref="taxon:7"\n' + big + long_line + many + ge.random_text(rng, 600) + b'\n /translation="MKV'
    assert text.count(b"\n") > 1500
    full = ge.convert(text)
    assert full["state"].in_t and len(full["text"]) > 5 * 4096
    n = len(full["text"])
    for cap in (n, n - 1, 4096, 4097, 0):
        emu.L.gbemu_reset(emu.h)
        same(emu, ge.convert(text, out_cap=cap), text, cap, order, cap)
    emu.L.gbemu_reset(emu.h)                                   # in blocks of about 3000 bytes
    st, at = ge.State(), 0
    while at < len(text):
        end = text.find(b"\n", min(len(text) - 1, at + 3000)) + 1 or len(text)
        want = ge.convert(text[at:end], st)
        same(emu, want, text[at:end], len(want["text"]), order, at)
        st, at = want["state"], end
    for trial in range(30):                                    # small texts, from the start of a file: missing taxa among them
        emu.L.gbemu_reset(emu.h)
        t = ge.random_text(rng, rng.randrange(0, 12), taxon_first=rng.random() < 0.5)
        want = ge.convert(t)
        same(emu, want, t, len(want["text"]), order, t)
