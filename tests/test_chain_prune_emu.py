"""Greedy chain pruning on the host (the inputs: chain_inputs.py; the reference walk: chain_expect.py; the device's half, with the
same expectations: test_gpu_chain_prune.py).

Layer 1: kj_chain_hopeless, the host's compilation (emu_chain_hopeless), against the plain walk over the sweep and the random
set.  What is asserted, all of it exact:
  SOUND everywhere: `hopeless` implies that no stopping point of the walk holds m letters with a score of thr.  One
    counter-example is a wrong record in production.
  TIGHT where the rule sees everything the length depends on - the window shows all sixteen letters in front of the match or
    the fragment's start (a >= 16, or wq == 0): there a chain whose longest match stays below m letters must be called hopeless.
  Elsewhere the rule is conservative BY DESIGN and only soundness holds: with 0 < a < 16 letters in a window that does not start
    with the fragment (it answers "reachable" without looking), for a chain that is still alive behind the sixteenth letter,
    and in the score test (eleven for every letter gained, four for every substitution - bounds, not the BLOSUM62 entries the
    walk adds up).  No equality with the walk is asserted there.
Layer 2: the designed reads through the emulation with and without the rule (-DKJ_NO_CHAIN_PRUNE) against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import chain_expect as X
import chain_inputs as CI
import util

CASE_DTYPE = np.dtype([("win", "u1", (CI.ROW,)), ("tx", "u1", (16,)), ("wq", "<i4"), ("pz", "<i4"), ("j", "<i4"), ("sc0", "<i4"),
                       ("thr", "<i4"), ("nmm", "<u4"), ("m", "<u4"), ("mismatches", "<u4")])      # kaiju_gpu_chain_case


def host_rule(emu, c):
    emu.lib.emu_chain_hopeless.restype = C.c_int
    emu.lib.emu_chain_hopeless.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    recs = CI.pack_cases(c, CASE_DTYPE)
    out = np.zeros(len(recs), dtype=np.uint8)
    assert emu.lib.emu_chain_hopeless(recs.ctypes.data, len(recs), out.ctypes.data) == 0
    return out.astype(bool)


def check_rule(c, hopeless, what):
    """soundness everywhere, tightness in the exact classes (see the module's docstring); prints a counter-example as a case"""
    assert len(hopeless) == len(c["a"])
    unsound = np.nonzero(hopeless & c["reachable"])[0]
    assert len(unsound) == 0, (what, "hopeless, but the walk reaches a match", len(unsound), CI.show_case(c, int(unsound[0])))
    exact = np.isin(c["cls"], [CI.CLASSES.index(k) for k in CI.EXACT_CLASSES])
    assert (exact == ((c["a"] >= 16) | (c["wq"] == 0))).all()
    loose = np.nonzero(exact & (c["max_len"] < c["m"]) & ~hopeless)[0]
    assert len(loose) == 0, (what, "never m letters, but not hopeless", len(loose), CI.show_case(c, int(loose[0])))


def test_rule_cases_census():
    """the set holds what the issue of the rule asks for, and every cell of (class of a) x (substitutions left) x (answer)"""
    c = CI.rule_cases()
    table = CI.rule_census(c)
    assert table.shape == (9, 6, 2) and table.min() >= 1
    s = slice(0, c["n_sweep"])
    assert set(c["a"][s].tolist()) == set(CI.A_SWEEP) and {(a - 16) & 3 for a in CI.A_SWEEP if a > 16} == {0, 1, 2, 3}
    assert {(int(m), int(q)) for m, q in zip(c["mismatches"][s], c["nmm"][s])} == {(m, q) for m in CI.MISMATCHES for q in range(m + 1)}
    # the domain: pz in the window, the match behind it, letters 1 .. 20 in front of it
    assert ((c["pz"] - c["wq"] >= 0) & (c["pz"] - c["wq"] < CI.WIN) & (c["j"] >= c["pz"]) & (c["nmm"] <= c["mismatches"])).all()
    k = np.arange(16)[None, :]
    assert ((c["front"] >= 1) & (c["front"] <= 20) | (k >= c["pz"][:, None])).all() and (c["text"] == 0).any()
    # the walk meets its thresholds from both sides in the exact classes: max_len at m - 1, m and m + 1
    exact = (c["a"] >= 16) | (c["wq"] == 0)
    for d in (-1, 0, 1):
        assert (exact & ~c["open"] & (c["max_len"] == c["m"] + d)).sum() >= 1000, d
    assert c["open"].sum() >= 1000 and (c["reachable"] & ~c["open"]).sum() >= 1000
    # the terminator rung (the case the first form of the rule missed): a text byte that is no letter ends a chain that the
    # substitutions left would have carried to m letters - tightness holds the rule to it
    cut = exact & (c["max_len"] < c["m"]) & ((c["text"] == 0) & (k < np.minimum(c["pz"], 16)[:, None])).any(axis=1)
    assert cut.sum() >= 300, int(cut.sum())


def test_walk_all_is_the_plain_walk():
    """the array form of the walk against the letter-by-letter one, on a sample that has every class"""
    c = CI.rule_cases()
    rng = np.random.default_rng(7)
    idx = np.concatenate([rng.choice(len(c["a"]), 4000, replace=False)] +
                         [np.nonzero(c["cls"] == k)[0][:60] for k in range(len(CI.CLASSES))])
    for i in idx:
        i = int(i)
        nf = min(16, int(c["pz"][i]))
        got = X.walk(c["front"][i][:nf], c["text"][i], int(c["pz"][i]), int(c["l0"][i]), int(c["nmm"][i]), int(c["sc0"][i]), int(c["thr"][i]),
                     int(c["m"][i]), int(c["mismatches"][i]))
        assert got == (bool(c["reachable"][i]), int(c["max_len"][i]), bool(c["open"][i])), CI.show_case(c, i)


def test_blosum62_is_the_librarys(oracle, tmp_path):
    """the table restated in chain_expect.py scores a fragment as the oracle does: a database of one protein, protein reads that
    are exact stretches of it - `best` is the diagonal sum of the stretch"""
    from kaiju_amd import mkfmi, synth
    rng = np.random.default_rng(3)
    prot = "".join(X.ALPHABET[int(i)] for i in rng.permutation(np.arange(400) % 20))
    lines, leaves = synth.make_taxonomy(2, 2, 2)
    faa, fmi, nodes = (str(tmp_path / f) for f in ("db.faa", "db.fmi", "nodes.dmp"))
    with open(faa, "w") as f:
        f.write(f">p_{int(leaves[0])}\n{prot}\n>q_{int(leaves[1])}\n{prot[::-1]}\n>r_{int(leaves[2])}\n{prot[100:300][::-1]}\n")
    synth.write_nodes_dmp(nodes, lines)
    mkfmi.build_fmi(faa, fmi, threads=1, exponent=3)
    reads = [prot[s: s + 20] for s in range(0, 380, 7)]
    seqs, off = util.pack([r.encode() for r in reads])
    got = oracle.classify(oracle.load_fmi(fmi), oracle.load_nodes(nodes), oracle.params("greedy", seg=0, use_evalue=0, protein=1, min_score=30),
                          seqs, off)
    assert [int(g["best"]) for g in got] == [X.score(X.code(r)) for r in reads]


def test_blosum62_every_entry_is_the_librarys(D, emu):
    """all 400 entries of the restated table against the tables the lanes read (host_tables.cpp: the substitution scores by
    index-alphabet code, the diagonal)"""
    emu.lib.emu_b62.restype = C.c_int
    emu.lib.emu_b62.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    for c in range(1, 21):
        assert emu.lib.emu_b62(D.h, c, c, 1) == int(X.B62[c, c]), c
        for d in range(1, 21):
            assert emu.lib.emu_b62(D.h, c, d, 0) == int(X.B62[c, d]), (c, d)
    assert emu.lib.emu_b62(D.h, 0, 3, 0) == -128 and int(X.B62[1:, 1:].max()) == 11
    off = X.B62[1:, 1:] - np.diag(np.diag(X.B62[1:, 1:])) - 99 * np.eye(20, dtype=np.int64)
    assert int(off.max()) <= 4                    # (the rule's bounds: 11 a letter gained, 4 a substitution)


def emu_array(emu, h, name):
    """one array of the emulation's index, as kaiju_gpu_index_read_array hands out the device's"""
    from kaiju_amd import api
    lay = api.IndexLayout()
    emu.lib.emu_index_get_layout.argtypes = [C.c_void_p, C.POINTER(api.IndexLayout)]
    emu.lib.emu_index_read_array.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    assert emu.lib.emu_index_get_layout(h, C.byref(lay)) == 0
    which = api.INDEX_ARRAYS.index(name)
    out = np.zeros(int(lay.bytes[which]), dtype=np.uint8)
    assert emu.lib.emu_index_read_array(h, which, 0, len(out), out.ctypes.data) == 0
    return out


class Designed:
    """layer 2, built once: the database, the oracle's records of every parameter tuple, the census"""

    def __init__(self, oracle, emu, workdir):
        self.W = W = CI.designed()
        self.faa, self.fmi, self.nodes = CI.write_db(W, workdir)
        self.oracle, self.ix, self.tax = oracle, oracle.load_fmi(self.fmi), oracle.load_nodes(self.nodes)
        self.h = emu.load(self.fmi)
        text, sa = emu_array(emu, self.h, "text"), emu_array(emu, self.h, "sa_full").view(np.uint32)
        self.nrows = len(sa)
        self.where = CI.locate(W, text, sa)
        self._want = {}
        self.kept, self.dropped = CI.census(W, {t: self.want(t, 0) for t in ("mm1", "mm3", "mm5")}, self.where, self.nrows)

    def want(self, tup, seg):
        if (tup, seg) not in self._want:
            s, o = CI.pack_reads(CI.reads_of(self.W.reads, tup))
            self._want[tup, seg] = self.oracle.classify(self.ix, self.tax, CI.oracle_params(self.oracle, tup, seg), s, o)
        return self._want[tup, seg]

    def kept_mask(self, tup):
        names = {rd.name for rd, _ in self.kept}
        return np.array([r.name in names for r in CI.reads_of(self.W.reads, tup)])


@pytest.fixture(scope="module")
def D(oracle, emu, tmp_path_factory):
    return Designed(oracle, emu, str(tmp_path_factory.mktemp("chain")))


def test_designed_reads_census(D):
    """every rung keeps a near-side and a far-side read that the walk and the oracle confirm; at most 10 % of the designed reads
    are dropped (another match was better, a site was not unique, no letter gave the score)"""
    import collections
    W = D.W
    assert 300 <= len(W.db) <= 400 and len(W.db) % 8 != 0 and len(W.reads) >= 200
    assert len(D.dropped) <= 0.10 * len(W.reads), [(rd.name, rung) for rd, rung in D.dropped]
    have = collections.Counter((rung, rd.side) for rd, rung in D.kept)
    missing = [(rung, side) for rung in CI.required_rungs() for side in ("near", "far") if have[rung, side] < 1]
    assert not missing, missing
    # the near side is classified by the designed match alone, the far side is not classified by the site
    by_name = {rd.name: rung for rd, rung in D.kept}
    for tup in ("mm1", "mm3", "mm5"):
        for rd, rec in zip(CI.reads_of(W.reads, tup), D.want(tup, 0)):
            if rd.name in by_name and rd.side == "near" and not rd.extra:
                assert int(rec["best"]) == CI.TUPLES[tup][2] and int(rec["n_ids"]) == (5 if rd.hopeful is None else 1), rd.name
    # without substitutions nothing of it is found (but the exact match that the reads of the `best` rung carry behind R)
    for rd, rec in zip(CI.reads_of(W.reads, "mm0"), D.want("mm0", 0)):
        assert int(rec["best"]) == (rd.extra[1] if rd.extra else 0), rd.name


@pytest.mark.parametrize("seg", [0, 1])
def test_designed_reads_emulation_equals_oracle(D, emu, seg):
    """the lane with the rule and the lane built without it (-DKJ_NO_CHAIN_PRUNE): both the oracle's records on every set and
    parameter tuple, and each other's"""
    plain = util.Emu(so=os.path.join(util.EMU_DIR, "libkaiju_kernel_emu_noprune.so"), defines=("KJ_NO_CHAIN_PRUNE",))
    h0 = plain.load(D.fmi)
    for tup, (m, M, T) in CI.TUPLES.items():
        reads = CI.reads_of(D.W.reads, tup)
        s, o = CI.pack_reads(reads)
        want = D.want(tup, seg)
        gp = util.gp("greedy", m=m, mismatches=M, min_score=T, seg=seg, use_evalue=0, protein=1)
        a, _ = emu.classify(D.h, gp, s, o)
        b, _ = plain.classify(h0, gp, s, o)
        assert (a == b).all(), (tup, seg)
        bad = [reads[i].name for i in range(len(reads)) if not util.same_hit(want[i], a[i])]      # (the dropped reads too)
        assert not bad, (tup, seg, bad[:5])
    plain.lib.emu_index_free(h0)


def test_long_fragments_show_the_rule_the_designed_window(D):
    """the window rungs: which letters the lane's window shows when the rule is asked is the lane's business, so the designer's
    claim is checked where it can be seen - a build of the emulation with the workload histograms (-DKJ_HIST) counts a = pz - wq
    and wq > 0 at the rule's call site.  Every rung's reads ask the rule with the a they were built for (chain_inputs.WIN_RUNGS
    says which windows a read can produce at all)"""
    hist = util.Emu(so=os.path.join(util.EMU_DIR, "libkaiju_kernel_emu_hist.so"), defines=("KJ_HIST",))
    hist.lib.emu_hist.restype = C.POINTER(C.c_ulonglong * (16 * 64))
    h = hist.load(D.fmi)
    m, M, T = CI.TUPLES["mm3"]
    gp = util.gp("greedy", m=m, mismatches=M, min_score=T, seg=0, use_evalue=0, protein=1)
    table = lambda: np.array(hist.lib.emu_hist().contents, dtype=np.int64).reshape(16, 64)      # noqa: E731
    for cls, a, tail in CI.WIN_RUNGS:
        reads = [rd for rd, rung in D.kept if rung == ("win", cls, a)]
        assert reads and all((len(rd.pep) > CI.WIN) == (tail > 0) for rd in reads), (cls, a)
        before = table()
        s, o = CI.pack_reads(reads)
        hist.classify(h, gp, s, o)
        d = table() - before
        assert d[13][a] >= len(reads) and d[14][1 if cls == "refill" else 0] >= len(reads), (cls, a, np.nonzero(d[13])[0].tolist(), d[14][:2].tolist())
        assert cls == "refill" or d[14][1] == 0, (cls, a)
    # two seeds in one long fragment: any a in a window that does NOT start with the fragment (one substitution: tuple mm1)
    m1, M1, T1 = CI.TUPLES["mm1"]
    gp1 = util.gp("greedy", m=m1, mismatches=M1, min_score=T1, seg=0, use_evalue=0, protein=1)
    for cls, a in CI.TWO_SEED_RUNGS:
        reads = [rd for rd, rung in D.kept if rung == ("win2", cls, a)]
        assert len(reads) >= 2 and all(len(rd.pep) > CI.WIN for rd in reads), (cls, a)
        before = table()
        s, o = CI.pack_reads(reads)
        hist.classify(h, gp1, s, o)
        d = table() - before
        # (core B is on five rows: nobody asks about it, its variant only moves the window)
        assert d[13][a] == len(reads) == d[13].sum() and d[14][1] == len(reads) and d[14][0] == 0, (cls, a, np.nonzero(d[13])[0].tolist(), d[14][:2].tolist())
    # pz == 0: the lane does not ask (chain_inputs.design says why)
    reads = [rd for rd, rung in D.kept if rung == ("pz0",)]
    before = table()
    s, o = CI.pack_reads(reads)
    hist.classify(h, gp, s, o)
    assert len(reads) >= 2 and all(rd.pz == 0 for rd in reads) and (table() - before)[13].sum() == 0
    # ... and the short reads ask it in a window that starts with the fragment
    reads = [rd for rd, rung in D.kept if rung[0] == "len" and rd.tup == "mm3"]
    before = table()
    s, o = CI.pack_reads(reads)
    hist.classify(h, gp, s, o)
    d = table() - before
    assert d[14][0] >= len(reads) and d[14][1] == 0 and d[13][16:].sum() == 0
    hist.lib.emu_index_free(h)


def nucleotide_sets(D, seg):
    """(name, reads, packed, paired, the oracle's records) of the nucleotide singles and pairs (tuple mm3), computed once"""
    key = ("nt", seg)
    if key not in D._want:
        singles, pairs = CI.nucleotide_reads(D.W)
        out = []
        for name, reads, pe in (("singles", singles, False), ("pairs", pairs, True)):
            s, o = util.pack([r[1].encode() for r in reads], [r[2].encode() for r in reads] if pe else None)
            out.append((name, reads, (s, o), pe, D.oracle.classify(D.ix, D.tax, CI.oracle_params(D.oracle, "mm3", seg, protein=0), s, o, paired=pe)))
        D._want[key] = out
    return D._want[key]


@pytest.mark.parametrize("seg", [0, 1])
def test_nucleotide_reads_emulation_equals_oracle(D, emu, seg):
    """the chains behind the six-frame translation, one long read and pairs with mates on different rungs: the census (SEG off) -
    a kept near-side read is classified by its site from nucleotides too, a pair by its near-side mates' sites alone - and both
    lanes against the oracle"""
    plain = util.Emu(so=os.path.join(util.EMU_DIR, "libkaiju_kernel_emu_noprune.so"), defines=("KJ_NO_CHAIN_PRUNE",))
    h0 = plain.load(D.fmi)
    m, M, T = CI.TUPLES["mm3"]
    kept = {rd.name for rd, _ in D.kept}
    for name, reads, (s, o), pe, want in nucleotide_sets(D, seg):
        if seg == 0:
            miss = 0
            for (nm, _, _, mates), rec in zip(reads, want):
                ids = {int(x) for x in rec["taxid"][: int(rec["n_ids"])]}
                exp = {rd.site.members[rd.hopeful or 0][1] for rd in mates if rd.side == "near" and rd.name in kept and rd.hopeful is not None}
                if all(rd.name in kept for rd in mates):
                    miss += ids != exp or int(rec["best"]) != (T if exp else 0)
            assert miss <= 0.1 * len(reads), (name, miss)
            assert any(len(r[1]) > 3 * CI.WIN for r in reads) or pe
        gp = util.gp("greedy", m=m, mismatches=M, min_score=T, seg=seg, use_evalue=0)
        a, _ = emu.classify(D.h, gp, s, o, paired=pe)
        b, _ = plain.classify(h0, gp, s, o, paired=pe)
        assert (a == b).all(), (name, seg)
        bad = [reads[i][0] for i in range(len(reads)) if not util.same_hit(want[i], a[i])]
        assert not bad, (name, seg, bad[:5])
    plain.lib.emu_index_free(h0)


def test_rule_on_the_host(emu):
    c = CI.rule_cases()
    hopeless = host_rule(emu, c)
    check_rule(c, hopeless, "host")
    # the rule does prune: a rule that always answered "reachable" would be sound too
    assert hopeless.sum() >= len(hopeless) // 5
    # and it refuses what the lane cannot pass instead of reading outside the row
    bad = CI.pack_cases({k: (v[:1] if hasattr(v, "__len__") else v) for k, v in c.items()}, CASE_DTYPE)
    bad["pz"], bad["wq"], bad["j"] = 70, 6, 80
    out = np.zeros(1, dtype=np.uint8)
    assert emu.lib.emu_chain_hopeless(bad.ctypes.data, 1, out.ctypes.data) == -1
