"""What the stages behind the suffix sort must produce (kaiju_amd/csrc/kj_fmibuild.h), in numpy, from the format of the .fmi file:
given a text, its suffix array (sufsort_inputs.expected), `copies` and the checkpoint exponent - the sequence order, the samples,
the BWT (raw and byte-coded), index1, index2 and startLcode.  Shared by tests/test_fmibuild_emu.py (host emulation, host stages)
and tests/test_gpu_fmibuild.py (device); tests/test_fmibuild_expect_golden.py pins it to a file the reference's binaries wrote.

The file (bwt/bwt.c, bwt/suffixArray.c, bwt/fmicommon.h, bwt/compactfmi.c of the reference): rows 0 .. nseq-1 of the BWT are the
terminator suffixes in file order, row nseq + k is suffix SA[k]; the letter of a row is the symbol in front of its suffix, the
terminator where there is none.  Every row appears `copies` times in a row.  Sequences are numbered in the order of their
whole-sequence suffixes, empty ones first.  A sample exists for every row k >= nseq * copies that is a multiple of 2^e:
(number of the sequence << pbits) + offset, big-endian in nbytes.  index1[R][a] = C[a] + occurrences of a before row R << 16 (a
last row holds C alone), index2[q][a] = occurrences between the start of the piece and row q << 8 (a last row: up to the end).
The BWT bytes are coded per block of 256 rows: startLcode[c] + min(n, top), n = equal letters before the row in the block for the
first 128 rows, behind it for the rest."""
import functools
import struct

import numpy as np

import sufsort_inputs as si

ALEN = 21
BIG = {"big_65537": (65537, 4242), "big_131073": (131073, 4343)}        # i.i.d. texts across one and two pieces of 65 536 rows


@functools.lru_cache(maxsize=None)
def text(name):
    if name in BIG:
        t = si.iid_text(BIG[name][0], seed=BIG[name][1])
        t.setflags(write=False)
        return t
    return si.case(name)


@functools.lru_cache(maxsize=None)
def suffix_array(name):
    if name not in BIG:
        return si.expected(name)
    t = text(name)
    pos, end, raw = si._suffix_keys(t)
    order = sorted(range(len(pos)), key=lambda i: (raw[pos[i]:end[i] + 1], int(pos[i])))
    sa = pos[order].astype(np.uint32)
    sa.setflags(write=False)
    return sa


def _cases():
    out = [(n, 1, 3) for n, _ in si.cases()]
    out += [(n, c, 3) for n in ("iid_4095", "iid_4096", "iid_4097") for c in (16, 17)]      # 65 520, 65 536, 65 552 .. 69 649 rows
    out += [(n, 1, 3) for n in BIG]
    out += [(n, c, e) for n in ("iid_4097", "sequences_of_length_1") for e in (0, 2, 3, 5) for c in (1, 3, 7)]
    out += [("iid_4095", 4, 3), ("iid_4095", 2, 2)]          # nseq * copies a multiple of 2^e, the rows not: one sample more than the header counts
    return tuple(dict.fromkeys(out))


CASES = _cases()                                                          # (text, copies, exponent)
CASE_IDS = [f"{n}-c{c}-e{e}" for n, c, e in CASES]


def start_lcode(total):
    """the code table from the letter totals (find_startLcode): shares of 256 codes, at least two each"""
    tot = int(sum(total))
    maxn = [max(2, int(256 * (float(t) / tot))) for t in total]
    mx = 0
    for a in range(ALEN):
        if maxn[a] > maxn[mx]:
            mx = a
    s = sum(maxn)
    if s < 256:
        maxn[mx] += 256 - s
    while s > 256:
        mn = 0
        for a in range(1, ALEN):
            if maxn[mn] <= 2:
                mn = a
            if maxn[a] > 2 and maxn[a] < maxn[mn]:
                mn = a
        maxn[mn] -= 1
        s -= 1
    out = np.zeros(ALEN + 1, dtype=np.int32)
    out[1:] = np.cumsum(maxn)
    out[ALEN] = 256
    return out


@functools.lru_cache(maxsize=None)
def expected(name, copies=1, exponent=3):
    t, sa = text(name).astype(np.int64), suffix_array(name).astype(np.int64)
    tlen = len(t)
    term = np.flatnonzero(t == 0)
    nseq, nsuf = len(term), len(sa)
    assert nseq + nsuf == tlen and t[-1] == 0
    starts = np.concatenate(([0], term[:-1] + 1))
    lens = term - starts
    prev = np.concatenate(([0], t[:-1]))                    # the symbol in front of every position
    B = np.concatenate((prev[term], prev[sa])).astype(np.uint8)
    seq_of = lambda p: np.searchsorted(starts, p, side="right") - 1
    # the sequence order: empty sequences in file order, then the whole-sequence suffixes in row order
    whole = sa[B[nseq:] == 0]
    read_of_rank = np.concatenate((np.flatnonzero(lens == 0), seq_of(whole))).astype(np.int64)
    assert len(read_of_rank) == nseq and len(set(read_of_rank.tolist())) == nseq
    rank_of = np.empty(nseq, dtype=np.int64)
    rank_of[read_of_rank] = np.arange(nseq)
    bwt_raw = np.repeat(B, copies)
    otlen, onseq = tlen * copies, nseq * copies
    # samples
    sbits, pbits = int(onseq).bit_length(), int(lens.max()).bit_length()
    nbytes = (7 + sbits + pbits) // 8
    ncheck = (otlen >> exponent) - (onseq >> exponent)
    step = 1 << exponent
    k = np.arange(-(-onseq // step) * step, otlen, step, dtype=np.int64)[:max(ncheck, 0)]
    r, c = k // copies, k % copies
    p = sa[r - nseq]
    i = seq_of(p)
    val = ((rank_of[i] * copies + c) << pbits) + (p - starts[i])
    samples = np.zeros((max(ncheck, 0), nbytes), dtype=np.uint8)
    for b in range(nbytes):
        samples[:len(k), nbytes - 1 - b] = (val >> (8 * b)) & 0xff
    # checkpoints
    occ = np.zeros((otlen + 1, ALEN), dtype=np.int64)       # occ[j][a]: occurrences of a in rows [0, j)
    onehot = np.zeros((otlen, ALEN), dtype=np.int64)
    onehot[np.arange(otlen), bwt_raw] = 1
    np.cumsum(onehot, axis=0, out=occ[1:])
    total = occ[otlen]
    Cc = np.concatenate(([0], np.cumsum(total)[:-1]))
    N1 = ((otlen - 1) >> 16) + 2
    if (N1 << 16) == otlen:
        N1 -= 1
    N2 = ((otlen - 1) >> 8) + 2
    if (N1 << 8) == otlen:                                  # (N1: the reference's expression)
        N2 -= 1
    npieces = (otlen + 65535) >> 16
    index1 = np.zeros((N1, ALEN), dtype=np.int64)
    index1[:npieces] = occ[np.arange(npieces) << 16] + Cc
    index1[:npieces, 0] -= Cc[0]
    index1[N1 - 1] = Cc
    nblk = (otlen + 255) >> 8
    q = np.arange(nblk)
    index2 = np.zeros((N2, ALEN), dtype=np.int64)
    index2[:nblk] = occ[q << 8] - occ[(q >> 8) << 16]
    index2[N2 - 1] = total - occ[((otlen - 1) >> 16) << 16]
    sl = start_lcode(total)
    # byte coding
    blk0 = (np.arange(otlen) >> 8) << 8
    before = occ[np.arange(otlen), bwt_raw] - occ[blk0, bwt_raw]
    blk1 = np.minimum(blk0 + 256, otlen)
    after = occ[blk1, bwt_raw] - occ[np.arange(otlen), bwt_raw] - 1
    n = np.where((np.arange(otlen) & 255) < 128, before, after)
    top = sl[bwt_raw + 1] - sl[bwt_raw] - 1
    bwt = (sl[bwt_raw] + np.minimum(n, top)).astype(np.uint8)
    out = {"read_of_rank": read_of_rank.astype(np.uint32), "samples": samples.reshape(-1), "bwt_raw": bwt_raw, "bwt": bwt,
           "index1": index1.reshape(-1), "index2": index2.astype(np.uint16).reshape(-1), "startLcode": sl,
           "nseq": nseq, "bwtlen": otlen, "ncheck": ncheck, "nbytes": nbytes, "sbits": sbits, "pbits": pbits, "N1": N1, "N2": N2}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


ARRAYS = ("read_of_rank", "samples", "bwt", "index1", "index2", "startLcode")
SCALARS = ("nseq", "bwtlen", "ncheck", "nbytes", "sbits", "pbits", "N1", "N2")


def first_difference(got, want, recode=True):
    """None, or (what, index, got, want) of the first element that differs"""
    for k in SCALARS:
        if int(got[k]) != int(want[k]):
            return (k, 0, int(got[k]), int(want[k]))
    for k in ARRAYS:
        w = want["bwt_raw" if k == "bwt" and not recode else k]
        g = np.asarray(got[k])
        if len(g) != len(w):
            return (k + " length", 0, len(g), len(w))
        bad = np.flatnonzero(g != w)
        if len(bad):
            return (k, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))
    return None


def read_fmi(path):
    """the sections of a .fmi file"""
    raw = open(path, "rb").read()
    at = 0

    def take(fmt):
        nonlocal at
        v = struct.unpack_from("<" + fmt, raw, at)
        at += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def arr(dtype, n):
        nonlocal at
        v = np.frombuffer(raw, dtype=dtype, count=n, offset=at)
        at += v.nbytes
        return v

    out = {}
    out["bwtlen"], out["nseq"], alen = take("qii")
    out["alphabet"] = raw[at:at + alen]
    at += alen
    bwtlen2, out["ncheck"], out["exponent"], out["nbytes"], out["sbits"], out["pbits"], out["mask"], out["check"], nseq2 = take("qqiiiiqqi")
    names = []
    for _ in range(out["nseq"]):
        l = raw[at]
        names.append(raw[at + 1:at + 1 + l])
        at += 1 + l
    out["names"] = names
    out["read_of_rank"] = arr(np.int32, out["nseq"]).astype(np.uint32)
    out["lengths"] = arr(np.int64, out["nseq"])
    out["samples"] = arr(np.uint8, out["ncheck"] * out["nbytes"])
    alen2, bwtlen3, out["N1"], out["N2"] = take("iqii")
    out["bwt"] = arr(np.uint8, out["bwtlen"])
    out["index1"] = arr(np.int64, out["N1"] * alen)
    out["index2"] = arr(np.uint16, out["N2"] * alen)
    out["startLcode"] = arr(np.int32, alen + 1)
    assert at == len(raw) and alen == alen2 == ALEN and bwtlen2 == bwtlen3 == out["bwtlen"] and nseq2 == out["nseq"]
    return out
