"""The interval records of the sampled row -> taxon table's tests (test_row_tax_sampled_emu.py on the host twin,
test_gpu_row_tax_sampled.py through kaiju_gpu_locate_intervals) and the ids they must get, from index_truth.Truth alone."""
import numpy as np

import index_truth as it
from kaiju_amd import api

ID_CAP, MAX_IDS = 1, 21
LENS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 100)


def make_cases(bwtlen, seed):
    """(lo, len, first): every lo in 0 .. 63 and in the last 64 rows with every length of LENS that stays inside, 2000 random
    intervals - one record each - and records of 2, 3 and 16 intervals"""
    rng = np.random.default_rng(seed)
    lo, ln, first = [], [], [0]
    for a in list(range(64)) + list(range(bwtlen - 64, bwtlen)):
        for l in LENS:
            if a + l <= bwtlen:
                lo.append(a); ln.append(l); first.append(len(lo))
    rl = rng.integers(0, bwtlen, size=2000)
    rn = np.minimum(rng.choice([1, 1, 1, 2, 3, 5, 8, 13, 21, 40, 77], size=2000), bwtlen - rl)
    for a, l in zip(rl.tolist(), rn.tolist()):
        lo.append(a); ln.append(l); first.append(len(lo))
    for k in (2, 3, 16):
        for _ in range(150):
            a = rng.integers(0, bwtlen, size=k)
            l = np.minimum(rng.choice([1, 1, 2, 3, 4, 9, 17], size=k), bwtlen - a)
            lo += a.tolist(); ln += l.tolist(); first.append(len(lo))
    return np.asarray(lo, dtype=np.uint64), np.asarray(ln, dtype=np.uint32), np.asarray(first, dtype=np.uint32)


def expected_records(T, lo, ln, first, cap, skip=None):
    """ids_from_SI over the intervals of every record, from Truth alone: rows in order, the limit `nids > cap` in front of
    every row, first seen first, rows of unusable names (and `skip`) giving nothing; 21 slots"""
    contributes = T.seq_valid[T.row_seq].astype(bool) & ~T.beyond
    if skip is not None:
        contributes = contributes & ~skip
    row_taxon = T.seq_taxid[T.row_seq]
    out = np.zeros(len(first) - 1, dtype=api.HIT_DTYPE)
    for r in range(len(first) - 1):
        ids, flags, done = [], 0, False
        for i in range(int(first[r]), int(first[r + 1])):
            if done:
                break
            for row in range(int(lo[i]), int(lo[i]) + int(ln[i])):
                if len(ids) > cap:
                    flags, done = ID_CAP, True
                    break
                if contributes[row]:
                    t = int(row_taxon[row])
                    if t not in ids and len(ids) < MAX_IDS:
                        ids.append(t)
        out[r]["n_ids"], out[r]["flags"] = len(ids), flags
        out[r]["taxid"][:len(ids)] = ids
    return out


def special_rows(T):
    """rows below nseq on a 2^e boundary (module docstring)"""
    r = np.arange(T.bwtlen)
    return (r < T.nseq) & (r % (1 << T.chpt_exp) == 0)


def records_with(mask, lo, ln, first):
    cum = np.concatenate([[0], np.cumsum(mask)])
    per_iv = cum[lo.astype(np.int64) + ln] - cum[lo.astype(np.int64)]
    return np.add.reduceat(per_iv, first[:-1].astype(np.int64)) > 0


def same_records(a, b, what):
    bad = np.nonzero(a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1))[0]
    assert len(bad) == 0, (what, "first record", int(bad[0]), a[bad[0]], b[bad[0]])


def build_world(oracle, d, which=("C", "D")):
    """indexes C, D (and B: the short sample array) of index_truth with their Truth, the interval records and what Truth says they
    give at the limits 20 and 3 - `want` as it stands, `want_walk` with the rows below nseq on a 2^e boundary skipped"""
    make = {"B": lambda: it.make_index_b(d), "C": lambda: it.make_index_c(d), "D": lambda: it.make_index_b(d, align64=True)}
    out = {}
    for name in which:
        fmi, faa = make[name]()
        T = it.Truth(oracle, fmi, faa)
        assert T.chpt_exp == 3 and T.sa_short == (name == "B")
        lo, ln, first = make_cases(T.bwtlen, 77 + ord(name))
        want = {cap: expected_records(T, lo, ln, first, cap) for cap in (20, 3)}
        want_walk = {cap: expected_records(T, lo, ln, first, cap, skip=special_rows(T)) for cap in (20, 3)}
        out[name] = dict(fmi=fmi, T=T, cases=(lo, ln, first), want=want, want_walk=want_walk)
    return out
