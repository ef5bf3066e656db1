"""The sampled row -> taxon table (DevIndex::row_tax_s) on the host: the policy that picks it (kj_rowtax_plan.h), the table the
host twin builds (PackedIndex::build_text_wide with KAIJU_EMU_ROW_TAX_SHIFT), the locate that walks to it
(mem_locate_read_team<true, T, true>) and its place in the flow plan.  tests/emu/locate_sampled_emu.cpp runs records that hold
given suffix-array intervals through the locate on the full table, the walk to the suffix array's sample and the walk to the
sampled table; the ids every record must get are derived in Python from index_truth.Truth alone.

Rows below nseq that are a multiple of 2^chpt_exp: no search ends in such a row (the suffixes there begin with a terminator),
and the reference's get_suffix has no answer for one - it indexes in front of the sample array (bwt.c:115-116).  The walk to
the suffix array's sample skips such a row ("beyond the samples", kj_core.h), the two tables hold the taxon of the row's
sequence, which is what Truth says.  The intervals lo = 0 .. 63 meet eight of them: the expected records of the WALK are
computed with these rows skipped, those of the tables from Truth as it stands, and the three locators must give identical
records wherever no such row is met."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index_truth as it
import util
from kaiju_amd import api
from row_tax_sampled_cases import ID_CAP, MAX_IDS, build_world, records_with, same_records, special_rows

EMU_SRC = [os.path.join(util.ROOT, "tests", "emu", "locate_sampled_emu.cpp"), os.path.join(util.CSRC, "host_index.cpp")]
FULL, WALK, SAMPLED, MANYROWS = 0, 1, 2, 3                     # lse_locate's `which`
NONE, KIND_FULL, KIND_SAMPLED = 0, 1, 2                        # RowTaxPlan::Kind
# kj_flow.h
IN_LANE, ROW_TAX, ROW_TAX_WIDE, TEAM, WIDE_WALK, FUSED, SAMPLED_WIDE = range(7)


def bind(L):
    L.lse_load.restype = C.c_void_p
    L.lse_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.lse_free.argtypes = [C.c_void_p]
    L.lse_info.argtypes = [C.c_void_p, C.c_void_p]
    L.lse_table.restype = C.c_void_p
    L.lse_table.argtypes = [C.c_void_p]
    L.lse_tax_of_dense.restype = C.c_void_p
    L.lse_tax_of_dense.argtypes = [C.c_void_p]
    L.lse_locate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.lse_plan_row_tax.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_char_p, C.c_char_p, C.c_void_p]
    L.lse_inline_rule.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64]
    L.lse_flow.argtypes = [C.c_int] * 5 + [C.c_void_p]
    return L


@pytest.fixture(scope="module")
def lse(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("locate_sampled_emu") / "liblocate_sampled_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-pthread", "-o", so] + EMU_SRC, check=True)
    return bind(C.CDLL(so))


# ---- the policy -----------------------------------------------------------------------------------------------------------
def plan(lse, bwtlen, nseq, e, free, row_tax=None, shift=None):
    out = np.zeros(4, dtype=np.uint64)
    enc = lambda v: None if v is None else str(v).encode()
    lse.lse_plan_row_tax(int(bwtlen), int(nseq), e, int(free), enc(row_tax), enc(shift), out.ctypes.data)
    return tuple(int(x) for x in out)


GB = 10 ** 9
HBM = 288 * GB
# (rows, sequences, footprint without the table): DESIGN.md section 2 - measured at 28.10 G and 60.20 G rows (14.3 M proteins x 7 /
# x 15), 2.56 B per row + the 20.48 GB k-mer table in between
REFSEQ_REF = (28_100_000_000, 100_100_000, 92.37 * GB)
MID = (45_000_000_000, 160_000_000, 45e9 * 2.56 + 20.48 * GB)
REFSEQ = (60_200_000_000, 214_500_000, 174.53 * GB)


def table_bytes(bwtlen, s):
    return bwtlen * 4 + 64 if s == 0 else ((bwtlen >> s) + 1) * 4 + 64


def test_policy_table(lse):
    for (rows, nseq, fp), want in ((REFSEQ_REF, (KIND_FULL, 0)), (MID, (KIND_SAMPLED, 1)), (REFSEQ, (KIND_SAMPLED, 2))):
        kind, s, nbytes, ignored = plan(lse, rows, nseq, 3, HBM - fp)
        assert (kind, s) == want and nbytes == table_bytes(rows, s) and not ignored, (rows, kind, s)
    assert table_bytes(REFSEQ[0], 2) == 60_200_000_068                      # (the 60 GB next to 174.5 GB)
    # a card with no room: nothing, whatever the index
    for rows, nseq, fp in (REFSEQ_REF, MID, REFSEQ):
        assert plan(lse, rows, nseq, 3, 9 * GB)[:3] == (NONE, 0, 0)
        assert plan(lse, rows, nseq, 3, 0)[:3] == (NONE, 0, 0)
    # the exponent of the suffix array's sample caps the shift: s < e
    rows, nseq, fp = REFSEQ
    assert plan(lse, rows, nseq, 3, HBM - fp)[:2] == (KIND_SAMPLED, 2)
    assert plan(lse, rows, nseq, 2, HBM - fp)[:2] == (NONE, 0)              # (s = 1 does not fit, s = 2 is not below e)
    assert plan(lse, rows, nseq, 1, HBM - fp)[:2] == (NONE, 0)
    assert plan(lse, MID[0], MID[1], 2, HBM - MID[2])[:2] == (KIND_SAMPLED, 1)
    assert plan(lse, MID[0], MID[1], 1, HBM - MID[2])[:2] == (NONE, 0)
    assert plan(lse, REFSEQ_REF[0], REFSEQ_REF[1], 1, HBM - REFSEQ_REF[2])[:2] == (KIND_FULL, 0)
    assert plan(lse, REFSEQ_REF[0], REFSEQ_REF[1], 0, HBM - REFSEQ_REF[2])[:2] == (KIND_FULL, 0)
    # s = 3 is the last one tried (e = 4: a table of every eighth row where every fourth does not fit)
    free3 = int((table_bytes(rows, 3) + nseq * 20 + 64 + (8 << 30)) / 0.7) + 2
    assert plan(lse, rows, nseq, 4, free3)[:2] == (KIND_SAMPLED, 3)
    assert plan(lse, rows, nseq, 5, free3 // 2)[:2] == (NONE, 0)


def test_policy_overrides(lse):
    rows, nseq, fp = REFSEQ
    free = HBM - fp
    assert plan(lse, rows, nseq, 3, free, row_tax=0)[:2] == (NONE, 0)                       # the way back
    assert plan(lse, rows, nseq, 3, free, row_tax=0, shift=2)[:2] == (NONE, 0)
    assert plan(lse, rows, nseq, 3, free, row_tax=1)[:3] == (KIND_FULL, 0, table_bytes(rows, 0))    # as before: forced, fitting or not
    assert plan(lse, REFSEQ_REF[0], REFSEQ_REF[1], 3, 0, row_tax=1)[:2] == (KIND_FULL, 0)
    for s in (1, 2):
        for rt in (None, 1):
            assert plan(lse, rows, nseq, 3, 0, row_tax=rt, shift=s) == (KIND_SAMPLED, s, table_bytes(rows, s), 0)
    assert plan(lse, rows, nseq, 3, 0, shift=0)[:3] == (KIND_FULL, 0, table_bytes(rows, 0))
    assert plan(lse, rows, nseq, 4, 0, shift=3)[:2] == (KIND_SAMPLED, 3)
    # values outside 0 .. 3, or not below the exponent: ignored (and said so), the decision is what it is without the variable
    for bad, e in ((3, 3), (2, 2), (1, 1), (4, 8), (-1, 3), ("x", 3), ("", 3), ("2x", 3)):
        assert plan(lse, rows, nseq, e, free, shift=bad) == plan(lse, rows, nseq, e, free)[:3] + (1,), (bad, e)
        assert plan(lse, rows, nseq, e, free, row_tax=1, shift=bad) == (KIND_FULL, 0, table_bytes(rows, 0), 1)
        assert plan(lse, rows, nseq, e, free, row_tax=0, shift=bad)[:2] == (NONE, 0)


def test_policy_full_flips_where_the_inline_rule_did(lse):
    """the byte at which `bwtlen * 4 + 64 + nseq * 20 + 64 + 8 GiB <= 0.7 * free` becomes true is the byte at which the plan
    says `full`"""
    for rows, nseq in ((REFSEQ_REF[0], REFSEQ_REF[1]), (4_390_000_001, 14_300_001), (1 << 32, 1), (70_001, 345)):
        lo, hi = 0, 1 << 50
        while hi - lo > 1:                                       # the smallest free_bytes of the old rule
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if lse.lse_inline_rule(rows, nseq, mid) else (mid, hi)
        assert lse.lse_inline_rule(rows, nseq, hi) and not lse.lse_inline_rule(rows, nseq, hi - 1)
        assert abs(hi - (table_bytes(rows, 0) + nseq * 20 + 64 + (8 << 30)) / 0.7) < 4096
        for free in range(hi - 3, hi + 4):
            for e in (1, 3):
                assert (plan(lse, rows, nseq, e, free)[0] == KIND_FULL) == bool(lse.lse_inline_rule(rows, nseq, free)) == (free >= hi)
        assert plan(lse, rows, nseq, 3, hi - 1)[:2] == (KIND_SAMPLED, 1)


# ---- the flow plan --------------------------------------------------------------------------------------------------------
def test_flow_plan(lse):
    def flow(row_tax, sampled, mode, verbose, records16=1):
        out = np.zeros(4, dtype=np.uint64)
        lse.lse_flow(row_tax, sampled, mode, verbose, records16, out.ctypes.data)
        return dict(locate=int(out[0]), fused=int(out[1]), lane=int(out[2]), mem_verbose=int(out[3]))
    for mode in (0, 1):
        for verbose in (0, 1):
            for records16 in (0, 1):
                f = flow(0, 1, mode, verbose, records16)
                assert f["locate"] == SAMPLED_WIDE and f["fused"] == 0 and f["mem_verbose"] == verbose, (mode, verbose)
                assert flow(1, 1, mode, verbose, records16)["locate"] == ROW_TAX_WIDE          # the full table wins
                assert flow(1, 0, mode, verbose, records16)["locate"] == ROW_TAX_WIDE
                assert flow(0, 0, mode, verbose, records16)["locate"] == WIDE_WALK
                assert flow(0, 1, mode, verbose, records16)["lane"] == flow(0, 0, mode, verbose, records16)["lane"]


# ---- the locate -----------------------------------------------------------------------------------------------------------
class Loaded:
    def __init__(self, lse, fmi, shift):
        env = {"KAIJU_GPU_FORCE_WIDE": "16", "KAIJU_EMU_ROW_TAX_SHIFT": None if shift is None else str(shift), "KAIJU_EMU_NO_ROW_TAX": None}
        old = {k: os.environ.pop(k, None) for k in env}
        os.environ.update({k: v for k, v in env.items() if v is not None})
        try:
            err = C.create_string_buffer(512)
            self.h = lse.lse_load(fmi.encode(), err, 512)
            assert self.h, err.value
        finally:
            for k, v in old.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        self.lse = lse
        info = np.zeros(6, dtype=np.uint64)
        lse.lse_info(self.h, info.ctypes.data)
        self.bwtlen, self.shift, self.has_full, self.has_sampled, self.entries, self.n_dense = (int(x) for x in info)

    def table(self):
        return np.ctypeslib.as_array(C.cast(self.lse.lse_table(self.h), C.POINTER(C.c_uint32)), shape=(self.entries,)).copy()

    def tax_of_dense(self):
        return np.ctypeslib.as_array(C.cast(self.lse.lse_tax_of_dense(self.h), C.POINTER(C.c_uint64)), shape=(self.n_dense,)).copy()

    def locate(self, which, lo, ln, first, cap, steps=False):
        out = np.zeros(len(first) - 1, dtype=api.HIT_DTYPE)
        st = np.zeros(len(out), dtype=np.uint64)
        rc = self.lse.lse_locate(self.h, which, lo.ctypes.data, ln.ctypes.data, first.ctypes.data, len(out), cap, out.ctypes.data,
                                 st.ctypes.data)
        assert rc == 0, rc
        return (out, st.astype(np.int64)) if steps else out

    def close(self):
        self.lse.lse_free(self.h)


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle, lse):
    """indexes C and D with their Truth, the interval records and what Truth says they give (computed once)"""
    return build_world(oracle, tmp_path_factory.mktemp("row_tax_sampled"))


def test_cases_meet_what_they_are_for(world):
    """from Truth alone: index D has 37 taxa and five unusable names; the records meet the limit (both values), skipped rows,
    all 21 slots, rows on and off every sample boundary, and records of 1, 2, 3 and 16 intervals"""
    T = world["D"]["T"]
    valid = T.seq_valid.astype(bool)
    assert len(set(T.seq_taxid[valid].tolist())) == 37 and int((~valid).sum()) == 5
    for name, w in world.items():
        T = w["T"]
        lo, ln, first = w["cases"]
        assert set(np.diff(first).tolist()) == {1, 2, 3, 16}
        assert set((lo % 8).tolist()) == set(range(8)) and set(((lo + ln) % 8).tolist()) == set(range(8))
        assert int(lo.min()) == 0 and int((lo + ln).max()) == T.bwtlen
        skipped = ~(T.seq_valid[T.row_seq].astype(bool))
        assert records_with(skipped, lo, ln, first).any() == (name == "D")
        special = records_with(special_rows(T), lo, ln, first)
        assert special.sum() >= 8
        for cap in (20, 3):                                       # (and only there does the walk's answer differ from the tables')
            differ = (w["want"][cap].view(np.uint8).reshape(len(special), -1) != w["want_walk"][cap].view(np.uint8).reshape(len(special), -1)).any(axis=1)
            assert differ.any() and not (differ & ~special).any()
        assert (w["want"][3]["flags"] == ID_CAP).any() and (w["want"][3]["n_ids"] == 4).any()
        assert (w["want"][20]["flags"] == 0).any() and (w["want"][3]["flags"] == 0).any()
    assert (world["D"]["want"][20]["flags"] == ID_CAP).any()
    assert (world["D"]["want"][20]["n_ids"] == MAX_IDS).any()


@pytest.mark.parametrize("name", ["C", "D"])
def test_three_locators_agree(world, lse, name):
    w = world[name]
    lo, ln, first = w["cases"]
    plain = ~records_with(special_rows(w["T"]), lo, ln, first)
    full = Loaded(lse, w["fmi"], None)
    try:
        assert full.has_full and not full.has_sampled and full.shift == 0
        got_full = {cap: full.locate(FULL, lo, ln, first, cap) for cap in (20, 3)}
        got_walk = {cap: full.locate(WALK, lo, ln, first, cap) for cap in (20, 3)}
        for cap in (20, 3):
            same_records(got_full[cap], w["want"][cap], ("full table against Truth", cap))
            same_records(full.locate(MANYROWS, lo, ln, first, cap), w["want"][cap], ("full table, many-rows instantiation", cap))
            same_records(got_walk[cap], w["want_walk"][cap], ("walk to the suffix array's sample against Truth", cap))
            same_records(got_walk[cap][plain], got_full[cap][plain], ("walk against full table", cap))
    finally:
        full.close()
    for s in (1, 2):
        smp = Loaded(lse, w["fmi"], s)
        try:
            assert smp.has_sampled and not smp.has_full and smp.shift == s
            for cap in (20, 3):
                got = smp.locate(SAMPLED, lo, ln, first, cap)
                same_records(got, w["want"][cap], ("sampled table against Truth", s, cap))
                same_records(got, got_full[cap], ("sampled against full table", s, cap))
                same_records(got[plain], got_walk[cap][plain], ("sampled against the walk", s, cap))
                same_records(smp.locate(WALK, lo, ln, first, cap), got_walk[cap], ("the walk on an index with the sampled table", s, cap))
        finally:
            smp.close()


def steps_to(T, stop):
    """LF steps from every row to the first row where `stop` holds or whose BWT letter is the terminator (from Truth's LF alone)"""
    n = T.bwtlen
    d = np.full(n, -1, dtype=np.int64)
    d[stop | (T.L == 0)] = 0
    while (d < 0).any():
        todo = np.nonzero(d < 0)[0]
        nxt = d[T.LF[todo]]
        d[todo[nxt >= 0]] = nxt[nxt >= 0] + 1
    return d


@pytest.mark.parametrize("name", ["C", "D"])
def test_walk_lengths(world, lse, name):
    """the walk to the sampled table takes, row by row, the LF steps to the first multiple of 2^s (or to a terminator): never
    more than the walk to the suffix array's sample, and on the i.i.d. index D 2^s - 1 a row on average where that walk takes
    2^e - 1 (a row is on a boundary with probability 2^-s at every step; index C's forty copies of one homopolymer keep a walk
    off the boundaries for up to 2000 steps - either walk).  Records of one interval of up to 17 rows: every row is walked, the
    limit of 20 ids cannot end them early"""
    w = world[name]
    T = w["T"]
    lo, ln, first = w["cases"]
    one = np.nonzero((np.diff(first) == 1) & (ln[first[:-1]] <= 17))[0]
    lo1, ln1 = lo[first[one]].astype(np.int64), ln[first[one]].astype(np.int64)
    f1 = np.arange(len(one) + 1, dtype=np.uint32)
    rows = np.arange(T.bwtlen)
    # (the walk to the suffix array's sample: a row below nseq on a boundary stops at once, as any row on a boundary)
    d_e = steps_to(T, rows % 8 == 0)
    cum_e = np.concatenate([[0], np.cumsum(d_e)])
    for s in (1, 2):
        d_s = steps_to(T, rows % (1 << s) == 0)
        assert (d_s <= d_e).all()
        cum_s = np.concatenate([[0], np.cumsum(d_s)])
        smp = Loaded(lse, w["fmi"], s)
        try:
            _, got_s = smp.locate(SAMPLED, lo[first[one]], ln[first[one]], f1, 20, steps=True)
            _, got_e = smp.locate(WALK, lo[first[one]], ln[first[one]], f1, 20, steps=True)
        finally:
            smp.close()
        assert (got_s == cum_s[lo1 + ln1] - cum_s[lo1]).all(), s
        assert (got_e == cum_e[lo1 + ln1] - cum_e[lo1]).all()
        assert (got_s <= got_e).all() and got_s.sum() < got_e.sum()
        if name == "D":
            assert abs(got_s.sum() / ln1.sum() / ((1 << s) - 1) - 1) < 0.15 and abs(got_e.sum() / ln1.sum() / 7 - 1) < 0.15


@pytest.mark.parametrize("name", ["C", "D"])
def test_host_built_sampled_table(world, lse, name, capfd):
    T = world[name]["T"]
    contributes = T.seq_valid[T.row_seq].astype(bool) & ~T.beyond
    row_taxon = T.seq_taxid[T.row_seq]
    for s in (1, 2):
        smp = Loaded(lse, world[name]["fmi"], s)
        try:
            n_e = (T.bwtlen >> s) + 1
            assert smp.entries == n_e + 16                       # ((bwtlen >> s) + 1) * 4 + 64 bytes
            tab, tod = smp.table(), smp.tax_of_dense()
            rows = np.arange(0, T.bwtlen, 1 << s)
            assert len(rows) in (n_e, n_e - 1)
            got = tab[:len(rows)]
            assert ((got == it.NONE32) == ~contributes[rows]).all()
            assert (tab[len(rows):] == it.NONE32).all()          # (the entry behind the last row, the slack)
            ok = contributes[rows]
            assert got[ok].max() < len(tod) and (tod[got[ok]] == row_taxon[rows][ok]).all()
            assert len(np.unique(tod)) == len(tod)
        finally:
            smp.close()
    capfd.readouterr()
    # e = 3: a shift of 3 is refused - the index gets the full table - and the loader says so
    smp = Loaded(lse, world[name]["fmi"], 3)
    try:
        assert smp.has_full and not smp.has_sampled and smp.shift == 0 and smp.entries == T.bwtlen + 16
        assert "KAIJU_EMU_ROW_TAX_SHIFT=3 ignored" in capfd.readouterr().err
    finally:
        smp.close()


def test_standalone_build_with_sanitizers(world, lse, tmp_path):
    """the same source as a program of its own under the address and undefined-behaviour sanitizers, over the same records: it
    must run clean and print the digests of the records the library gives"""
    exe = str(tmp_path / "locate_sampled_emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", "-pthread", "-DLSE_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe] + EMU_SRC, check=True)

    def fnv(a):
        h = 1469598103934665603
        for b in a.tobytes():
            h = ((h ^ b) * 1099511628211) & 0xffffffffffffffff
        return h
    for name, w in world.items():
        lo, ln, first = w["cases"]
        path = str(tmp_path / f"cases_{name}.bin")
        with open(path, "wb") as f:
            f.write(np.asarray([len(first) - 1, len(lo)], dtype=np.uint32).tobytes() + first.tobytes() + ln.tobytes() + lo.tobytes())
        # (the environment as it is; the program sets KAIJU_GPU_FORCE_WIDE and KAIJU_EMU_ROW_TAX_SHIFT itself)
        env = {k: v for k, v in os.environ.items() if k not in ("KAIJU_EMU_ROW_TAX_SHIFT", "KAIJU_EMU_NO_ROW_TAX")}
        for s in (1, 2):
            p = subprocess.run([exe, w["fmi"], path, str(s)], env=env, capture_output=True, text=True)
            assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
            lines = [tuple(x.split()) for x in p.stdout.split("\n") if x]
            # (locators 0, 1, 3 on the full table, then 1, 2 on the sampled one; the limit 20 and 3 each)
            assert [x[:3] for x in lines] == [("0", str(wh), str(cap)) for wh in (FULL, WALK, MANYROWS) for cap in (20, 3)] + \
                                             [(str(s), str(wh), str(cap)) for wh in (WALK, SAMPLED) for cap in (20, 3)]
            for shift, which, cap, dig in lines:
                want = w["want_walk" if int(which) == WALK else "want"][int(cap)]
                assert int(dig, 16) == fnv(want), (name, s, which, cap)
