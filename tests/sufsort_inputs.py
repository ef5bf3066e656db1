"""Texts for the suffix sorter (kaiju_amd/csrc/kj_sufsort.h), shared by tests/test_sufsort_emu.py (host emulation) and
tests/test_gpu_sufsort.py (device): the smallest ones at which each rule of the definition can break, and the naive
expectation - positions sorted by (symbols up to and including the terminator, position).  A text is a uint8 array of letter
codes 1 .. 20 with a terminator 0 behind every sequence."""
import functools
import math
import os

import numpy as np

K = 12                # symbols in the key of the first round (KJ_SS_K; the tests compare it with the header's)
TILE = 4096           # text bytes per block of the key kernel (KJ_SS_TILE; likewise)
ALPHABET = "*ACDEFGHIKLMNPQRSTVWY"
GOLDEN_FAA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "db.faa")


def encode(seqs):
    """letter strings -> text"""
    out = bytearray()
    for s in seqs:
        out += bytes(ALPHABET.index(c) for c in s) + b"\0"
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def iid_text(length, seed, mean_len=40):
    """`length` symbols: i.i.d. letters, a terminator with probability 1 / mean_len, the last symbol a terminator"""
    rng = np.random.default_rng(seed)
    t = rng.integers(1, 21, size=length, dtype=np.uint8)
    t[rng.random(length) < 1.0 / mean_len] = 0
    t[-1] = 0
    return t


def golden_text():
    """the golden database as the builder reads it: letters outside the alphabet become the last letter"""
    code = {c: i for i, c in enumerate(ALPHABET) if i}
    seqs = []
    with open(GOLDEN_FAA) as f:
        for line in f:
            if line.startswith(">"):
                seqs.append(bytearray())
            else:
                seqs[-1] += bytes(code.get(c, 20) for c in line.strip().upper() if c.isalpha())
    return np.frombuffer(b"".join(bytes(s) + b"\0" for s in seqs), dtype=np.uint8).copy()


def _substituted_family():
    rng = np.random.default_rng(77)
    base = rng.integers(1, 21, size=900, dtype=np.uint8)
    parts = []
    for i in range(30):
        s = base.copy()
        at = int(rng.integers(0, 900))
        s[at] = (int(s[at]) % 20) + 1          # another letter
        parts += [s, np.zeros(1, dtype=np.uint8)]
    return np.concatenate(parts)


IID_LENGTHS = tuple(dict.fromkeys((2, 255, 256, 257, 4095, 4096, 4097, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)))
IID_NAMES = tuple(f"iid_{n}" for n in IID_LENGTHS)


@functools.lru_cache(maxsize=None)
def cases():
    """(name, text) - built once, never modified (the arrays are read-only)"""
    out = [("len_1", np.zeros(1, dtype=np.uint8))]
    for n in IID_LENGTHS:
        out.append((f"iid_{n}", iid_text(n, seed=1000 + n)))
    out.append(("terminators_only", np.zeros(37, dtype=np.uint8)))
    out.append(("sequences_of_length_1", encode(["A", "C", "A", "Y", "A", "", "C", "Y", "Y"])))
    out.append(("code_20_only", encode(["Y" * 75])))
    out.append(("ends_at_tlen_16", encode(["ACDEFGHIKLMNPQR"])))            # the terminator is byte 15 of the only lane
    out.append(("ends_at_tlen_17", encode(["ACDEFGHIKLMNPQRS"])))           # ... byte 0 of a second lane
    out.append(("identical_40x300A", encode(["A" * 300] * 40)))
    out.append(("one_5000xAC", encode(["AC" * 5000])))
    out.append(("family_30x900", _substituted_family()))
    out.append(("proper_prefix", encode(["ACDEFGHIKLMNPQRSTVWYACD", "ACDEFGHIKLMNPQRSTVWYACDEF", "ACDEFGHIKLMNPQRSTVWY"])))
    out.append(("term_inside_key", encode(["ACDEFGHIKLM", "ACDEFGHIKLM", "ACDEFGHIKLMN", "ACDEFGHIKLMNA", "ACDEFGHIKLMN"])))   # 11, 12, 13 letters
    out.append(("golden_db", golden_text()))
    for _, t in out:
        t.setflags(write=False)
    return tuple(out)


def case(name):
    return dict(cases())[name]


def _suffix_keys(text):
    term = np.flatnonzero(text == 0)
    raw = text.tobytes()
    pos = np.flatnonzero(text != 0)
    end = term[np.searchsorted(term, pos)]
    return pos, end, raw


@functools.lru_cache(maxsize=None)
def expected(name):
    """the suffix array by the definition: positions of the letters sorted by (symbols up to and including the terminator, position)"""
    text = case(name)
    pos, end, raw = _suffix_keys(text)
    order = sorted(range(len(pos)), key=lambda i: (raw[pos[i]:end[i] + 1], int(pos[i])))
    sa = np.array([pos[i] for i in order], dtype=np.uint32)
    sa.setflags(write=False)
    return sa


@functools.lru_cache(maxsize=None)
def expected_active_after_first_round(name):
    """suffixes that the first round cannot finish: their first K symbols hold no terminator and are not unique"""
    text = case(name)
    pos, end, raw = _suffix_keys(text)
    count = {}
    for p, e in zip(pos.tolist(), end.tolist()):
        if e - p >= K:
            w = raw[p:p + K]
            count[w] = count.get(w, 0) + 1
    return sum(c for c in count.values() if c > 1)


def maxlen(text):
    term = np.flatnonzero(text == 0)
    return int(np.diff(np.concatenate(([-1], term))).max() - 1) if len(term) else 0


def round_bound(text):
    """Rounds the sorter may take.  Round r has compared K * 2^(r-1) symbols, and a suffix whose compared part holds its
    terminator is final: nothing is active once K * 2^(r-1) >= maxlen + 1.  A text with a letter takes at least the first round."""
    if not np.any(text != 0):
        return 0
    return max(1, math.ceil(math.log2((maxlen(text) + 1) / K)) + 1)
