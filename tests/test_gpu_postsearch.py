"""What sits between a finished search and a finished record, on the device, rung by rung (the inputs and their census:
tests/postsearch_inputs.py; the host's half, with the same expectations: test_postsearch_emu.py).

Code that only the device compiles and that these reads drive from both sides of its thresholds:
  mem_locate_read's device branches - two matches in registers, three and more handed on (k_mem_locate -> k_mem_locate_list,
    k_mem_post1 -> todo -> k_mem_post2), rows > kLocDeferRows = 8 handed to the many-rows instantiation
  the ballot compaction of k_mem_post1 (seglist, todo) and k_mem_locate (list): wavefronts with 0, 1, a few and 64 listed lanes
  mem_locate_read_team with a wavefront's shuffles (k_mem_locate_team on an index without the text arrays, k_mem_locate_wide on
    a wide index without its row -> taxon table)
  the lazy-SEG hand-off: kWinForce / kWinMulti -> seglist -> second search -> retry list
  the retry pass (k_mem_retry): entered by exactly the reads with more than si_cap = 16 longest matches
  k_lca / compact_hit / k_mem_post1<true> on records with 0, 1, 2, 21 and capped ids and ids that nodes.dmp does not have
The expected record is always the oracle's, all fields (util.same_hit); the expected LCA the host's of the oracle's ids."""
import os

import numpy as np
import pytest

import postsearch_inputs as P
import util

pytestmark = pytest.mark.gpu

INTERNAL = 0xE0000000            # KAIJU_HIT_INEXACT, kHitRetry, kHitLocPending: none of them leaves the library

# index layouts (read when an index is loaded): what locates the ids there
LAYOUTS = {
    "default": {},                                                      # k_mem_post1 / _post2; k_mem_locate<false> + _list
    "row_tax0": {"KAIJU_GPU_ROW_TAX": "0"},                             # decides on wide indexes only: a narrow one keeps its table (asserted)
    "no_text": {"KAIJU_GPU_NO_TEXT": "1"},                              # k_mem_locate_team
    "wide17": {"KAIJU_GPU_FORCE_WIDE": "17"},                           # k_mem_locate<true> + k_mem_locate_list<true>
    "wide17_row_tax0": {"KAIJU_GPU_FORCE_WIDE": "17", "KAIJU_GPU_ROW_TAX": "0"},   # k_mem_locate_wide
}
# context switches (read when a context is created)
SWITCHES = {"lazy_seg_off": {"KAIJU_GPU_LAZY_SEG": "0"}, "fused_post_off": {"KAIJU_GPU_FUSED_POST": "0"}, "mem_lane_v1": {"KAIJU_GPU_MEM_LANE": "v1"}}
MEM_SETS = (("ladder", 11), ("rows", 11), ("pairs", 8), ("short", 8))


class Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class World:
    """the database, the oracle's handles and records (each computed once), the indexes (each loaded once)"""

    def __init__(self, api, oracle, workdir):
        self.api, self.oracle = api, oracle
        self.I = P.inputs()
        _, self.fmi, self.nodes = P.write_db(self.I, workdir)
        self.ix, self.otax = oracle.load_fmi(self.fmi), oracle.load_nodes(self.nodes)
        self.tax = api.Taxonomy(self.nodes)
        self.dtax = api.DeviceTaxonomy(self.tax, 0)
        self.base, self.orders = P.layout_orders(self.I)
        self._want, self._idx, self._packed, self._default = {}, {}, {}, {}

    def reads(self, name):
        return self.base if name == "base" else self.I.kept[name]

    def packed(self, name):
        if name not in self._packed:
            s, o = P.pack(self.reads(name))
            self._packed[name] = (s, o, any(r.nt2 for r in self.reads(name)))
        return self._packed[name]

    def want(self, name, mode, seg, m=11, mm=3, kaijux=0, msi=20):
        key = (name, mode, seg, m, mm, kaijux, msi)
        if key not in self._want:
            s, o, pe = self.packed(name)
            p = self.oracle.params(mode, seg=seg, use_evalue=0, min_fragment_length=m, mismatches=mm, kaijux=kaijux, max_matches_SI=msi)
            self._want[key] = self.oracle.classify(self.ix, self.otax, p, s, o, paired=pe)
        return self._want[key]

    def index(self, layout, id_mode=0):
        key = (layout, id_mode)
        if key not in self._idx:
            with Env(LAYOUTS[layout]):
                self._idx[key] = self.api.Index(self.fmi, id_mode=id_mode)
            assert self._idx[key].info.warnings == 0
        return self._idx[key]

    def classifier(self, layout, mode, seg, m=11, mm=3, env=None, id_mode=0, msi=20):
        with Env(env or {}):
            return self.api.Classifier(self.index(layout, id_mode), self.api.default_params(mode, seg=seg, min_fragment_length=m, mismatches=mm,
                                                                                           max_matches_SI=msi))

    def default_records(self, seg):
        """the default configuration's records of sets 1, 2, 3 (computed once per seg)"""
        if seg not in self._default:
            self._default[seg] = run_mem_sets(self, "default", seg)
        return self._default[seg]

    def close(self):
        for ix in self._idx.values():
            ix.close()


@pytest.fixture(scope="module")
def W(gpu_lib, oracle, tmp_path_factory):
    w = World(gpu_lib, oracle, str(tmp_path_factory.mktemp("postsearch")))
    yield w
    w.close()


def over(reads, cap=16):
    return sum(r.k > cap for r in reads)


def check(clf, hits, want, reads, retries, what):
    """records == the oracle's, nothing inexact, the retry pass entered by `retries` reads"""
    st = clf.stats()
    assert st.error_flags == 0, what
    assert not (hits["flags"] & INTERNAL).any(), what
    bad = [reads[i].name for i in range(len(reads)) if not util.same_hit(want[i], hits[i])]
    assert not bad, (what, len(bad), bad[:5])
    assert st.n_overflow_retries == retries, (what, st.n_overflow_retries, retries)


def run_mem_sets(W, layout, seg, env=None, id_mode=0, what=""):
    """sets 1, 2, 3 through MEM on one layout; returns the records per set"""
    out = {}
    for m in (11, 8):
        clf = W.classifier(layout, "mem", seg, m=m, env=env, id_mode=id_mode)
        for name, mm_ in MEM_SETS:
            if mm_ != m:
                continue
            s, o, pe = W.packed(name)
            hits = clf.classify(s, o, paired=pe).copy()
            # more than si_cap = 16 equally long matches set ovf (the 17th does): those reads, and no others, take the retry pass
            check(clf, hits, W.want(name, "mem", seg, m=m, kaijux=id_mode), W.reads(name), over(W.reads(name)), (what or layout, "mem", seg, name))
            out[name] = hits
        clf.close()
    return out


@pytest.mark.parametrize("seg", [1, 0])
def test_mem_default(W, seg):
    """sets 1, 2, 3 in the default configuration.  Long reads with SEG: eager SEG, k_mem_locate + k_mem_locate_list; without:
    k_mem_post1 / _post2.  Short pairs with SEG: the lazy flow - a pair with more than 16 matches goes kWinForce -> seglist ->
    second search -> retry list."""
    W.default_records(seg)
    # batches that stay on the near side of si_cap: 16 matches and fewer (the 16-rung included) never enter the retry pass
    for name, m in (("ladder", 11), ("pairs", 8)):
        reads = [r for r in W.reads(name) if r.k <= 16]
        keep = [i for i, r in enumerate(W.reads(name)) if r.k <= 16]
        assert max(r.k for r in reads) == 16
        s, o = P.pack(reads)
        clf = W.classifier("default", "mem", seg, m=m)
        hits = clf.classify(s, o, paired=name == "pairs")
        check(clf, hits, W.want(name, "mem", seg, m=m)[keep], reads, 0, ("near side", seg, name))
        clf.close()


@pytest.mark.parametrize("mm", [0, 3])
def test_greedy_default(W, mm):
    """set 4 (one motif k = 1 .. 22 times: k best matches of one score) and sets 1, 2 through Greedy: the records' matches are
    located by k_mem_locate + k_mem_locate_list behind the search.  At the default max_matches_SI = 20 no read takes the retry
    pass: greedy_lane2 keeps at most 20 best matches, which fit the record's 21 slots, and these reads come nowhere near the
    queue and match capacities.  What tells the two sides of max_matches_SI apart here is KAIJU_HIT_SI_CAP; the way into
    k_greedy_retry is a max_matches_SI raised by the caller: test_greedy_more_best_matches_than_slots."""
    clf = W.classifier("default", "greedy", 1, mm=mm)
    for name in ("greedy", "ladder", "rows"):
        s, o, pe = W.packed(name)
        hits = clf.classify(s, o, paired=pe).copy()
        check(clf, hits, W.want(name, "greedy", 1, mm=mm), W.reads(name), 0, ("greedy", mm, name))
        if name == "greedy" and mm == 0:
            assert [bool(int(h["flags"]) & 2) for h in hits] == [r.k > 20 for r in W.reads(name)]
    reads = [r for r in W.reads("greedy") if r.k <= 20]
    keep = [i for i, r in enumerate(W.reads("greedy")) if r.k <= 20]
    s, o = P.pack(reads)
    hits = clf.classify(s, o)
    check(clf, hits, W.want("greedy", "greedy", 1, mm=mm)[keep], reads, 0, ("greedy near side", mm))
    assert not (hits["flags"] & 2).any() or mm != 0
    clf.close()


@pytest.mark.parametrize("mm", [0, 3])
@pytest.mark.parametrize("msi", [22, 64])
def test_greedy_more_best_matches_than_slots(W, msi, mm):
    """max_matches_SI raised by the caller (the library takes 1 .. 64): greedy_lane2 then keeps more than kMaxIds = 21 best
    matches of a read, the record cannot hold them (nbest > kMaxIds), the read goes on the retry list with best = 0 and
    k_greedy_retry writes its record.  Set 4 at k = 21 and fewer stays in the main pass, k = 22 enters the retry pass."""
    clf = W.classifier("default", "greedy", 1, mm=mm, msi=msi)
    all_reads = W.reads("greedy")
    want = W.want("greedy", "greedy", 1, mm=mm, msi=msi)
    for top in (22, 21):
        keep = [i for i, r in enumerate(all_reads) if r.k <= top]
        reads = [all_reads[i] for i in keep]
        assert max(r.k for r in reads) == top
        s, o = P.pack(reads)
        hits = clf.classify(s, o).copy()
        st = clf.stats()
        assert st.error_flags == 0 and not (hits["flags"] & INTERNAL).any()
        bad = [reads[i].name for i in range(len(reads)) if not util.same_hit(want[keep][i], hits[i])]
        assert not bad, (msi, mm, top, len(bad), bad[:5])
        beyond = sum(r.k > 21 for r in reads)
        if mm == 0:
            # exact matches only: the best matches of a read are its k occurrences of the motif, one score
            assert st.n_overflow_retries == beyond, (msi, top, st.n_overflow_retries, beyond)
            assert not (hits["flags"] & 2).any()                 # (nobody has more than max_matches_SI)
        elif top == 22:
            # with substitutions several variants of one occurrence reach the best score: a read has more best matches than
            # occurrences (the emulation sends 15 of these reads to the retry pass for the census's 8), never fewer
            assert st.n_overflow_retries >= beyond >= 1, (msi, st.n_overflow_retries, beyond)
    clf.close()


@pytest.mark.parametrize("layout", [k for k in LAYOUTS if k != "default"])
def test_index_layouts(W, layout):
    """the same records from every way an index can hold what the locate needs: the team of lanes (shuffles) without the text
    arrays and on a wide index without its row -> taxon table, the wide instantiations of k_mem_locate / _list with it"""
    idx = W.index(layout)
    if not os.environ.get("KAIJU_GPU_FORCE_WIDE"):
        assert idx.footprint.wide == (1 if layout.startswith("wide") else 0)
    if layout == "row_tax0" and not os.environ.get("KAIJU_GPU_FORCE_WIDE"):
        # the switch is read for wide indexes only: this narrow index is the default one, table and all, and the sets below run
        # through the default's kernels once more - what the team locate gets is "no_text"
        assert int(idx.layout().bytes[W.api.INDEX_ARRAYS.index("row_tax")]) != 0 and idx.digest() == W.index("default").digest()
    if layout in ("no_text", "wide17_row_tax0"):                  # no row -> taxon table: the ids come from walks by teams of lanes
        assert int(idx.layout().bytes[W.api.INDEX_ARRAYS.index("row_tax")]) == 0
    for seg in (1, 0):
        run_mem_sets(W, layout, seg)
    clf = W.classifier(layout, "greedy", 1)
    for name in ("greedy", "ladder", "rows"):
        s, o, pe = W.packed(name)
        check(clf, clf.classify(s, o, paired=pe), W.want(name, "greedy", 1), W.reads(name), 0, (layout, "greedy", name))
    clf.close()


@pytest.mark.parametrize("seg", [1, 0])
def test_sequence_ids(W, seg):
    """kaijux: the ids are sequence numbers in the order maxMatches(.., 1) lists the matches (kParamXOrder: no swap of two
    matches of one fragment, the list head first) - against the oracle's kaijux records"""
    run_mem_sets(W, "default", seg, id_mode=W.api.IDS_SEQUENCE, what="kaijux")


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_context_switches(W, switch):
    """KAIJU_GPU_LAZY_SEG=0 (stage 1 finds the SEG triggers, an overflowing read goes to the retry list directly),
    KAIJU_GPU_FUSED_POST=0 (k_trigcheck, k_mem_locate, k_mem_locate_list, k_lca as passes of their own) and
    KAIJU_GPU_MEM_LANE=v1 (lanes that walk to the ids themselves; si_cap = 16 as well): the oracle's records, the default
    configuration's records, the same reads in the retry pass"""
    for seg in (1, 0):
        got = run_mem_sets(W, "default", seg, env=SWITCHES[switch], what=switch)
        ref = W.default_records(seg)
        for name in got:
            for f in ("best", "n_ids", "flags", "taxid"):
                assert (got[name][f] == ref[name][f]).all(), (switch, seg, name, f)


@pytest.mark.parametrize("fused", ["default", "fused_post_off"])
@pytest.mark.parametrize("seg", [1, 0])
def test_records_three_ways(W, seg, fused):
    """classify (184-byte records), classify_compact (k_mem_post1<true> / _post2<true> where the configuration allows: short
    pairs with SEG, everything without SEG; k_lca elsewhere and with KAIJU_GPU_FUSED_POST=0) and lca() of the records (k_lca):
    lca, best and info agree with each other and with the host LCA of the oracle's ids"""
    api = W.api
    env = SWITCHES[fused] if fused != "default" else None
    nids_seen = set()
    for name, m in MEM_SETS + (("base", 11),):
        clf = W.classifier("default", "mem", seg, m=m, env=env)
        s, o, pe = W.packed(name)
        want = W.want(name, "mem", seg, m=m)
        hits = clf.classify(s, o, paired=pe).copy()
        compact = clf.classify_compact(W.dtax, s, o, paired=pe).copy()
        assert clf.stats().error_flags == 0
        by_lca = clf.lca(W.dtax, hits).copy()
        exp = np.zeros(len(want), dtype=api.COMPACT_DTYPE)
        for i, w in enumerate(want):
            n = int(w["n_ids"])
            exp[i] = (W.tax.lca(w["taxid"][:n]) if n and int(w["best"]) else 0, int(w["best"]), (int(w["flags"]) & 3) << 8 | n)
            nids_seen.add((n, int(w["flags"]) & 1))
        for f in ("lca", "best", "info"):
            bad = [W.reads(name)[i].name for i in np.nonzero(compact[f] != exp[f])[0]]
            assert not bad, ("classify_compact", seg, fused, name, f, bad[:5])
            bad = [W.reads(name)[i].name for i in np.nonzero(by_lca[f] != exp[f])[0]]
            assert not bad, ("lca", seg, fused, name, f, bad[:5])
        clf.close()
    assert {(0, 0), (1, 0), (2, 0), (21, 0), (21, 1)} <= nids_seen
    # ids that nodes.dmp does not have: alone (returned as it is), next to a known id (dropped), two of them
    x = {r.name: i for i, r in enumerate(W.reads("rows")) if r.rung[:2] in (("rows", 1), ("rows", 2))}
    ids = {tuple(int(t) for t in W.want("rows", "mem", seg)[i]["taxid"][:2]) for i in x.values()}
    assert any(P.MISSING[0] in t for t in ids) and any(P.MISSING[1] in t for t in ids) and any(P.MISSING[2] in t and P.MISSING[3] in t for t in ids)


@pytest.mark.parametrize("seg", [1, 0])
def test_wavefront_layout(W, seg):
    """set 5: about 1000 reads with the list-bound ones (three to sixteen matches, or more than eight rows) all in front, one at
    the head of every wavefront, and permuted; batches of 1, 63, 64, 65 and 257 reads.  Every read's record is the record it has
    in the large batch, and the oracle's: the ballot compaction of k_mem_locate (SEG) and k_mem_post1 (no SEG) with 0, 1, a few
    and 64 listed lanes and partial last blocks."""
    want = W.want("base", "mem", seg)
    clf = W.classifier("default", "mem", seg)
    large, large_c = None, None
    for name, order in W.orders.items():
        reads = [W.base[i] for i in order]
        s, o = P.pack(reads)
        hits = clf.classify(s, o).copy()
        check(clf, hits, want[order], reads, over(reads), ("layout", seg, name))
        comp = clf.classify_compact(W.dtax, s, o).copy()
        if name == "front":
            inv = np.argsort(np.array(order))
            large, large_c = hits[inv], comp[inv]            # (indexed by the read's place in the base list)
        assert (hits == large[order]).all(), (seg, name)
        assert (comp == large_c[order]).all(), (seg, name)
    clf.close()


@pytest.mark.parametrize("fused", ["default", "fused_post_off"])
def test_pair_layout(W, fused):
    """the short pairs under lazy SEG with the listed ones in front (70 pairs with more than 16 matches: kWinForce, listed whatever
    their fragments look like; then 70 without a match, which nobody lists), one at the head of every wavefront, and permuted:
    the seglist ballot of k_mem_post1 (of k_trigcheck with KAIJU_GPU_FUSED_POST=0) with 64, one, a few and no listed lanes and a
    partial last block.  Every read's record is the oracle's, wherever it stands."""
    pairs = W.reads("pairs")
    want = W.want("pairs", "mem", 1, m=8)
    clf = W.classifier("default", "mem", 1, m=8, env=SWITCHES[fused] if fused != "default" else None)
    for name, order in P.pair_orders(W.I).items():
        reads = [pairs[i] for i in order]
        s, o = P.pack(reads)
        hits = clf.classify(s, o, paired=True).copy()
        check(clf, hits, want[order], reads, over(reads), ("pair layout", fused, name))
        comp = clf.classify_compact(W.dtax, s, o, paired=True)
        assert (comp["best"] == hits["best"]).all() and ((comp["info"] & 255) == hits["n_ids"]).all(), (fused, name)
    clf.close()
