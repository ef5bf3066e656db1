"""Greedy chain pruning on the device (the inputs: chain_inputs.py; the reference walk: chain_expect.py; the host's half, with the
same expectations and the census of the inputs: test_chain_prune_emu.py).

Layer 1: kj_chain_hopeless as the DEVICE compiles it (kaiju_gpu_chain_hopeless_check: one lane per case, the lane's window row
in LDS) - its difference mask comes from __brev there and from a loop on the host - case by case against the host's answers,
and against the plain walk: sound everywhere, tight where the window shows all sixteen letters (test_chain_prune_emu.py says
where the rule is conservative by design; nothing is asserted equal to the walk there).
Layer 2: the designed reads through api.Classifier on the index layouts that switch the rule on and off."""
import numpy as np
import pytest

import chain_inputs as CI
import util
from test_chain_prune_emu import check_rule, host_rule

pytestmark = pytest.mark.gpu


# index layouts (read when an index is loaded): where the rule can look
LAYOUTS = {
    "default": {},                                                            # the narrow rule, text position from the hint or sa_full
    "no_text": {"KAIJU_GPU_NO_TEXT": "1"},                                    # no text array: the rule is off
    "wide17_tv0": {"KAIJU_GPU_FORCE_WIDE": "17", "KAIJU_GPU_TV_SHIFT": "0"},  # the wide rule over sa_tpos5, a position for every row
    "wide17_tv1": {"KAIJU_GPU_FORCE_WIDE": "17", "KAIJU_GPU_TV_SHIFT": "1"},  # a sampled position table: the wide rule is off
}
RULE_ON = ("default", "wide17_tv0")
INTERNAL = 0xE0000000            # KAIJU_HIT_INEXACT, kHitRetry, kHitLocPending: none of them leaves the library


class Device:
    """the designed database on the device: every layout loaded once, the host's census (test_chain_prune_emu.Designed)"""

    def __init__(self, api, D):
        from test_gpu_postsearch import Env
        self.api, self.D, self.idx = api, D, {}
        for name, env in LAYOUTS.items():
            with Env(env):
                self.idx[name] = api.Index(D.fmi)
            assert self.idx[name].info.warnings == 0

    def classifier(self, layout, tup, seg):
        m, M, T = CI.TUPLES[tup]
        return self.api.Classifier(self.idx[layout], self.api.default_params("greedy", seg=seg, use_evalue=0, input_is_protein=1, min_fragment_length=m,
                                                                             mismatches=M, min_score=T))

    def run(self, clf, reads, count):
        clf.count_ops(count)
        s, o = CI.pack_reads(reads)
        hits = clf.classify(s, o).copy()
        assert clf.stats().error_flags == 0 and not (hits["flags"] & INTERNAL).any()
        return hits

    def pruned(self, layout, tup, reads):
        """(records, chains the counting lane left unqueued) of ONE batch, from a context of its own"""
        clf = self.classifier(layout, tup, 0)
        hits = self.run(clf, reads, True)
        n = clf.op_counts()["pruned_chains"]
        clf.close()
        return hits, n

    def pruned_each(self, layout, tup, reads):
        """(records, chains left unqueued per read): every read a batch of its own on one context - the counters are cleared when a
        batch starts"""
        clf = self.classifier(layout, tup, 0)
        hits, n = [], []
        for rd in reads:
            hits.append(self.run(clf, [rd], True)[0])
            n.append(clf.op_counts()["pruned_chains"])
        clf.close()
        return hits, n

    def close(self):
        for ix in self.idx.values():
            ix.close()


@pytest.fixture(scope="module")
def G(gpu_lib, oracle, emu, tmp_path_factory):
    from test_chain_prune_emu import Designed
    g = Device(gpu_lib, Designed(oracle, emu, str(tmp_path_factory.mktemp("chain_gpu"))))
    yield g
    g.close()


def far_side_the_rule_prunes(D, tup):
    """kept far-side reads whose designed chain the rule MUST call hopeless wherever it looks: one letter short behind a
    difference, on one to four rows, the whole chain in a window that starts with the fragment (a short read), the text
    position behind the head of the text.  From the census alone.  Other far-side reads are not counted: one score point
    short (the rule's score test is a bound), a fragment that starts one letter late (shorter than m up to the seed's end: no
    variant is made, nobody asks the rule); long fragments have tests of their own (test_two_seeds_in_one_fragment)"""
    return [rd for rd, rung in D.kept if rd.tup == tup and rd.side == "far" and rd.lookable and
            rung[0] in ("len", "rows", "gword", "last3") and len(rd.pep) <= CI.WIN]


def nothing_to_prune(D, tup):
    """kept reads none of whose items the rule may look at: both sides of the five-row families (every item of their chains lies
    on five rows) and of the site at the head of the text (every text position of its chain lies in front of 16 + kTextPad).
    (A near-side read elsewhere is NOT free of hopeless chains: the shorter matches that end inside its seed root chains of their
    own, one letter short each - the rule takes those.)"""
    return [rd for rd, rung in D.kept if rd.tup == tup and rung in (("rows", 5, "all"), ("head",))]


def test_layouts_hold_what_the_rule_needs(G):
    """from the layout read-back: the text array and a text position for every row where the rule is on, one of them missing where
    it is off; the default layout's arrays are the ones the census located the sites in"""
    from test_chain_prune_emu import emu_array
    A = G.api.INDEX_ARRAYS
    lay = {k: ix.layout() for k, ix in G.idx.items()}
    text = lambda l, a: int(l.bytes[A.index(a)])                              # noqa: E731  (bytes of an array of a layout)
    d = lay["default"]
    assert d.wide == 0 and text(d, "text") > 0 and text(d, "sa_full") == 4 * int(d.bwtlen)
    assert text(lay["no_text"], "text") == 0 and text(lay["no_text"], "sa_full") == 0
    w0, w1 = lay["wide17_tv0"], lay["wide17_tv1"]
    assert w0.wide == 1 and w0.tv_shift == 0 and text(w0, "text") > 0 and 0 <= text(w0, "sa_full") - 5 * int(w0.bwtlen) < 64   # (sa_tpos5: 5 bytes a row, slack for the 8-byte loads)
    assert w1.wide == 1 and w1.tv_shift == 1 and 0 < text(w1, "sa_full") < 5 * int(w1.bwtlen)
    emu_lib = util.Emu()                                                      # (the emulation's arrays: the same bytes)
    for name in ("text", "sa_full"):
        assert (G.idx["default"].read_array(name) == emu_array(emu_lib, G.D.h, name)).all(), name
    # the rungs that depend on where the index put a site, on THIS index
    nrows = int(d.bwtlen)
    rungs = {rung for _, rung in G.D.kept}
    assert {("gword", q) for q in range(4)} <= rungs and ("last3",) in rungs and ("head",) in rungs and nrows == G.D.nrows


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_designed_reads_on_the_device(G, layout):
    """every parameter tuple, SEG off (mm3: and on), the plain and the counting instantiation of the lane (two kernels): the oracle's
    records, all fields.  Counting, SEG off: no chain is pruned where the rule is off, or without substitutions; where it is on,
    every far-side read the rule must catch, a batch of its own, loses at least one chain (an inequality: the census cannot say
    how many more - the shorter matches inside a seed root chains of their own)"""
    D = G.D
    for tup in CI.TUPLES:
        reads = CI.reads_of(D.W.reads, tup)
        for seg in ((0, 1) if tup == "mm3" else (0,)):          # (SEG on with the tuple that holds every rung)
            want = D.want(tup, seg)
            clf = G.classifier(layout, tup, seg)
            for count in (False, True):
                hits = G.run(clf, reads, count)
                bad = [reads[i].name for i in range(len(reads)) if not util.same_hit(want[i], hits[i])]
                assert not bad, (layout, tup, seg, count, len(bad), bad[:5])
            clf.close()
        if layout not in RULE_ON or tup == "mm0":
            assert G.pruned(layout, tup, reads)[1] == 0, (layout, tup)
        else:
            must = far_side_the_rule_prunes(D, tup)
            hits, pruned = G.pruned_each(layout, tup, must)
            at = {r.name: i for i, r in enumerate(reads)}
            want = D.want(tup, 0)
            assert all(util.same_hit(want[at[r.name]], h) for r, h in zip(must, hits)), (layout, tup)
            missed = [r.name for r, n in zip(must, pruned) if n < 1]
            assert len(must) >= 3 and not missed, (layout, tup, missed)


@pytest.mark.parametrize("layout", RULE_ON)
def test_two_seeds_in_one_fragment(G, layout):
    """long protein reads with two seeds: the rule is asked about the first core in a window that does NOT start with the fragment
    (chain_inputs.TWO_SEED_RUNGS; test_chain_prune_emu.py checks the a of every rung).  Read by read, one substitution: with
    0 <= a < 16 the conservative exit answers - the far side is NOT pruned (and changes nothing); with a >= 16 the shifted
    window load shows all sixteen letters - the far side is pruned; the near side stays classified either way (the records of
    all of them: test_designed_reads_on_the_device)"""
    D = G.D
    reads = CI.reads_of(D.W.reads, "mm1")
    at = {r.name: i for i, r in enumerate(reads)}
    want = D.want("mm1", 0)
    mine = [(rd, rung[2]) for rd, rung in D.kept if rung[0] == "win2"]
    for cls, a in CI.TWO_SEED_RUNGS:
        assert {rd.side for rd, q in mine if q == a} == {"near", "far"}, (cls, a)
    hits, pruned = G.pruned_each(layout, "mm1", [rd for rd, _ in mine])
    for (rd, a), h, n in zip(mine, hits, pruned):
        assert util.same_hit(want[at[rd.name]], h), (layout, rd.name)
        if rd.side == "near":
            assert int(h["best"]) == CI.TUPLES["mm1"][2] and int(h["n_ids"]) == 1, (layout, rd.name)
        else:
            assert (n == 0) if a < 16 else (n >= 1), (layout, rd.name, n)


@pytest.mark.parametrize("layout", RULE_ON)
def test_nothing_to_prune(G, layout):
    """a batch that holds only what the rule does not look at (the census says which): the counter stays at zero, the records are
    the oracle's"""
    D = G.D
    reads = nothing_to_prune(D, "mm3")
    assert {(rd.rung, rd.side) for rd in reads} == {(r, s) for r in (("rows", 5, "all"), ("head",)) for s in ("near", "far")} and len(reads) >= 6
    at = {r.name: i for i, r in enumerate(CI.reads_of(D.W.reads, "mm3"))}
    hits, pruned = G.pruned(layout, "mm3", reads)
    want = D.want("mm3", 0)
    bad = [r.name for r, h in zip(reads, hits) if not util.same_hit(want[at[r.name]], h)]
    assert not bad and pruned == 0, (layout, pruned, bad[:5])


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_nucleotide_reads_on_the_device(G, layout):
    """the same chains behind stage 1 (six-frame translation), a fragment longer than the window from a long nucleotide read,
    pairs whose mates sit on different rungs; SEG off and on, plain and counting lanes: the oracle's records"""
    from test_chain_prune_emu import nucleotide_sets
    m, M, T = CI.TUPLES["mm3"]
    for seg in (0, 1):
        clf = G.api.Classifier(G.idx[layout], G.api.default_params("greedy", seg=seg, use_evalue=0, min_fragment_length=m, mismatches=M, min_score=T))
        for name, reads, (s, o), pe, want in nucleotide_sets(G.D, seg):
            for count in (False, True):
                clf.count_ops(count)
                hits = clf.classify(s, o, paired=pe).copy()
                assert clf.stats().error_flags == 0 and not (hits["flags"] & INTERNAL).any()
                bad = [reads[i][0] for i in range(len(reads)) if not util.same_hit(want[i], hits[i])]
                assert not bad, (layout, name, seg, count, bad[:5])
        clf.close()


def test_rule_on_the_device(gpu_lib, emu):
    api = gpu_lib
    c = CI.rule_cases()
    CI.rule_census(c)
    assert api.CHAIN_CASE_DTYPE.itemsize == 116 and api.CHAIN_WIN == CI.ROW
    got = api.chain_hopeless_check(CI.pack_cases(c, api.CHAIN_CASE_DTYPE)).astype(bool)
    want = host_rule(emu, c)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, ("device != host", len(bad), bool(got[bad[0]]), CI.show_case(c, int(bad[0])))
    check_rule(c, got, "device")
    # partial blocks, a single case, none
    recs = CI.pack_cases(c, api.CHAIN_CASE_DTYPE)
    for n in (0, 1, 255, 257):
        assert (api.chain_hopeless_check(recs[:n]).astype(bool) == want[:n]).all(), n
    # what the lane cannot pass is refused, not read: the word loads of the rule would leave the window row
    bad = recs[:1].copy()
    bad["pz"], bad["wq"], bad["j"] = 70, 6, 80
    with pytest.raises(api.KaijuGpuError):
        api.chain_hopeless_check(bad)
