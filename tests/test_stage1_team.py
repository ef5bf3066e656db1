"""The team stage 1 (kj_core.h: build_fragments_team, sixteen lanes per read, run on the host phase by phase) against the
one-lane fast stage 1 it replaces (build_fragments_fast<false, kS1Units>): the same peptide areas (stop padding included),
fragment lists, ReadMeta and error flags, byte for byte.  No GPU needed; test_gpu_stage1_team.py compares the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import util

SRC = os.path.join(util.EMU_DIR, "stage1_team_emu.cpp")


@pytest.fixture(scope="module")
def s1t(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("s1t") / "libstage1_team_emu.so")
    srcs = [SRC] + [os.path.join(util.CSRC, f) for f in ("host_index.cpp", "host_tables.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-pthread", "-o", so] + srcs,
                   check=True)
    L = C.CDLL(so)
    L.s1t_load.restype = C.c_void_p
    L.s1t_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.s1t_free.argtypes = [C.c_void_p]
    L.s1t_nuc3.argtypes = [C.c_void_p, C.c_void_p]
    L.s1t_compare.restype = C.c_int
    L.s1t_compare.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                              C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    err = C.create_string_buffer(512)
    h = L.s1t_load(util.Golden().fmi.encode(), err, 512)
    assert h, err.value
    yield L, h
    L.s1t_free(h)


def compare(s1t, mates1, mates2=None, m=11, mode=0, min_score=65):
    L, h = s1t
    seqs, off = util.pack(mates1, mates2)
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    first = C.c_int64(-1)
    err = (C.c_uint32 * 2)()
    nf = (C.c_uint64 * 2)()
    bad = L.s1t_compare(h, mode, m, min_score, seqs.ctypes.data, off.ctypes.data, len(mates1), 1 if mates2 is not None else 0,
                        C.byref(first), err, nf)
    where = None if first.value < 0 else (mates1[first.value], mates2[first.value] if mates2 is not None else None)
    assert bad == 0, (m, mode, bad, where)
    assert err[0] == err[1], (err[0], err[1])
    return err[0], nf[0], nf[1]


LETTERS = np.frombuffer(b"ACGTACGTACGTACGTACGTNacgtuURYKMSWBDHVn.*-", dtype=np.uint8)


def fuzz(rng, n, lo=1, hi=191, frac_clean=0.4, frac_orf=0.2):
    """reads of lo..hi nt: clean ACGT, reads without a stop in any frame (GCN codons: runs up to the whole string, m = 64
    included) with the odd substitution, and reads with N, IUPAC letters, lowercase, U and junk"""
    out = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        x = rng.random()
        if x < frac_orf:
            cod = rng.choice(np.array([b"GCA", b"GCC", b"GCG", b"GCT"]), size=ln // 3 + 1)
            r = bytearray(b"".join(cod)[:ln])
            for _ in range(int(rng.integers(0, 3))):
                if ln:
                    r[int(rng.integers(0, ln))] = int(rng.choice(LETTERS))
            out.append(bytes(r))
        elif x < frac_orf + frac_clean:
            out.append(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ln).tobytes())
        else:
            out.append(rng.choice(LETTERS, size=ln).tobytes())
    return out


def test_nuc3_letters(s1t):
    """the code table the translation relies on: 0..3 for bases, 4 for everything else - the zero bytes behind a mate's end included"""
    L, h = s1t
    t = (C.c_uint8 * 256)()
    L.s1t_nuc3(h, t)
    assert all(v <= 4 for v in t)
    assert t[0] == 4                                    # bytes behind a mate's end read as invalid bases: stops


@pytest.mark.parametrize("mode", [0, 1])
def test_golden_reads(s1t, mode):
    g = util.Golden()
    for m in (1, 11, 12, 20, 64):
        reads = [r for r in g.reads if len(r) <= 191]
        compare(s1t, reads, m=m, mode=mode)
        p1 = [a for a, b in zip(g.p1, g.p2) if len(a) <= 191 and len(b) <= 191]
        p2 = [b for a, b in zip(g.p1, g.p2) if len(a) <= 191 and len(b) <= 191]
        compare(s1t, p1, p2, m=m, mode=mode)


@pytest.mark.parametrize("m", [1, 11, 12, 20, 64])
def test_fuzzed_single(s1t, m):
    rng = np.random.default_rng(1000 + m)
    _, nf, nmax = compare(s1t, fuzz(rng, 3000), m=m)
    if m == 1:
        assert nmax > 24                                # lists beyond kS1ListCap: the sorted overflow path
    if m < 64:                                          # (64 residues need 192 nt)
        assert nf > 100


@pytest.mark.parametrize("m", [1, 11, 12, 20, 64])
def test_fuzzed_pairs(s1t, m):
    rng = np.random.default_rng(2000 + m)
    a = fuzz(rng, 2000, lo=0)
    b = fuzz(rng, 2000, lo=0)
    for i in range(0, 2000, 7):
        b[i] = b""                                      # empty second mates
    for i in range(3, 2000, 11):
        a[i] = b""                                      # ... and empty first ones
    _, _, nmax = compare(s1t, a, b, m=m)
    if m == 1:
        assert nmax > 24


def test_greedy_keys(s1t):
    """Greedy without SEG takes this stage 1 too: BLOSUM62 diagonal keys, fragments below min_score dropped"""
    rng = np.random.default_rng(7)
    for m, ms in ((11, 65), (1, 10), (12, 0), (20, 200)):
        compare(s1t, fuzz(rng, 1500), m=m, mode=1, min_score=ms)
        compare(s1t, fuzz(rng, 800, lo=0), fuzz(rng, 800, lo=0), m=m, mode=1, min_score=ms)


def test_lengths_at_unit_edges(s1t):
    rng = np.random.default_rng(11)
    lens = sorted({x for k in range(1, 64) for x in (3 * k - 1, 3 * k)} | set(range(47, 50)) | set(range(95, 98))
                  | set(range(143, 146)) | {190, 191})
    reads = [rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ln).tobytes() for ln in lens for _ in range(20)]
    reads += [rng.choice(LETTERS, size=ln).tobytes() for ln in lens for _ in range(5)]
    for m in (1, 11, 12, 20, 64):
        e, _, _ = compare(s1t, reads, m=m)
        assert e == 0
        e, _, _ = compare(s1t, reads, reads[::-1], m=m)
        assert e == 0


def test_too_long(s1t):
    """a mate of 192 nt raises kErrReadTooLong (and its read gets no fragments) in both"""
    rng = np.random.default_rng(5)
    reads = fuzz(rng, 50, lo=100, hi=191) + [b"ACGT" * 48] + fuzz(rng, 50, lo=100, hi=191)
    e, _, _ = compare(s1t, reads)
    assert e & 16
    e, _, _ = compare(s1t, fuzz(rng, 30), [b"A" * 192] + fuzz(rng, 29))
    assert e & 16
    e, _, _ = compare(s1t, fuzz(rng, 30, hi=191))
    assert e == 0
