"""The sampled row -> taxon table on the device: the table k_seq_walk_fill builds for KAIJU_GPU_ROW_TAX_SHIFT = 1, 2 (read back and
compared with index_truth.Truth), k_mem_locate_sampled over interval records (kaiju_gpu_locate_intervals; the same records and
expectations as test_row_tax_sampled_emu.py, and the same entry point over the kernels that were there before: the full table,
the walk to the suffix array's sample, a narrow index) and whole classifications on a forced-wide index with the sampled table
against the oracle (the database, read sets and census of tests/postsearch_inputs.py).

Rows below nseq on a 2^chpt_exp boundary: see test_row_tax_sampled_emu.py - the walk to the suffix array's sample skips them,
the tables answer with the taxon of the row's sequence."""
import os

import numpy as np
import pytest

import index_truth as it
import postsearch_inputs as P
import test_gpu_postsearch as TP
import util
from row_tax_sampled_cases import build_world, same_records

pytestmark = pytest.mark.gpu

KNOBS = ("KAIJU_GPU_FORCE_WIDE", "KAIJU_GPU_FMI_STREAM", "KAIJU_GPU_STREAM_PIECE_KB", "KAIJU_GPU_KMER", "KAIJU_GPU_TV_SHIFT",
         "KAIJU_GPU_ROW_TAX", "KAIJU_GPU_ROW_TAX_SHIFT", "KAIJU_GPU_NO_TEXT")


def load(api, fmi, env, id_mode=0):
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update({k: v for k, v in env.items() if v is not None})
    try:
        return api.Index(fmi, device=0, id_mode=id_mode)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    return build_world(oracle, tmp_path_factory.mktemp("row_tax_sampled_gpu"), which=("B", "C", "D"))


def wide_env(s=None, stream="0", row_tax=None):
    return {"KAIJU_GPU_FORCE_WIDE": "16", "KAIJU_GPU_KMER": "3", "KAIJU_GPU_FMI_STREAM": stream,
            "KAIJU_GPU_STREAM_PIECE_KB": "16" if stream == "1" else None, "KAIJU_GPU_ROW_TAX_SHIFT": None if s is None else str(s),
            "KAIJU_GPU_ROW_TAX": row_tax}


# ---- the arrays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("name", ["C", "D"])
def test_sampled_table(gpu_lib, world, name, s):
    api, T, fmi = gpu_lib, world[name]["T"], world[name]["fmi"]
    contributes = T.seq_valid[T.row_seq].astype(bool) & ~T.beyond
    row_taxon = T.seq_taxid[T.row_seq]
    full = load(api, fmi, wide_env())
    digests = []
    try:
        for stream in ("0", "1"):
            ix = load(api, fmi, wide_env(s, stream))
            try:
                lay = ix.layout()
                assert ix.row_tax_shift == s == lay.row_tax_shift and lay.wide == 1
                n_e = (T.bwtlen >> s) + 1
                assert int(lay.bytes[api.INDEX_ARRAYS.index("row_tax")]) == n_e * 4 + 64
                assert int(lay.bytes[api.INDEX_ARRAYS.index("tax_of_dense")]) == lay.n_dense * 8
                tab = ix.read_array("row_tax").view("<u4")
                tod = ix.read_array("tax_of_dense").view("<u8")
                rows = np.arange(0, T.bwtlen, 1 << s)
                got = tab[:len(rows)]
                assert ((got == it.NONE32) == ~contributes[rows]).all()
                assert (tab[len(rows):] == it.NONE32).all()          # (the entry behind the last row, the slack)
                ok = contributes[rows]
                assert got[ok].max() < len(tod) and (tod[got[ok]] == row_taxon[rows][ok]).all()
                assert len(np.unique(tod)) == len(tod)
                fp, fp_full = ix.footprint.as_dict(), full.footprint.as_dict()
                assert fp_full["sa_full"] - fp["sa_full"] == (T.bwtlen * 4 + 64) - (n_e * 4 + 64)
                assert fp_full["total"] - fp["total"] == fp_full["sa_full"] - fp["sa_full"]
                digests.append(ix.digest())
            finally:
                ix.close()
        assert digests[0] == digests[1]                              # host pack / streamed .fmi: every array, slot 11 included
        ref = full.digest()
        assert digests[0]["row_seq"] != ref["row_seq"] and {k: v for k, v in digests[0].items() if k != "row_seq"} == \
            {k: v for k, v in ref.items() if k != "row_seq"}
    finally:
        full.close()


@pytest.mark.parametrize("name", ["C", "D"])
def test_shift_0_is_the_layout_as_it_was(gpu_lib, world, name):
    api, fmi, T = gpu_lib, world[name]["fmi"], world[name]["T"]
    a = load(api, fmi, wide_env())
    b = load(api, fmi, wide_env(0))
    c = load(api, fmi, wide_env(3))              # (e = 3: refused with a line on stderr, the decision is as without the variable)
    try:
        for ix in (a, b, c):
            assert ix.row_tax_shift == 0 and int(ix.layout().bytes[api.INDEX_ARRAYS.index("row_tax")]) == T.bwtlen * 4
        assert a.digest() == b.digest() == c.digest() and bytes(a.layout()) == bytes(b.layout()) == bytes(c.layout())
        assert a.footprint.as_dict() == b.footprint.as_dict()
    finally:
        for ix in (a, b, c):
            ix.close()


def locate_all(api, ix, w, want_key, modes=(("mem", 20), ("mem", 3), ("greedy", 20))):
    lo, ln, first = w["cases"]
    for mode, cap in modes:
        clf = api.Classifier(ix, api.default_params(mode, max_match_ids=cap))
        try:
            got = clf.locate_intervals(lo, ln, first)
            same_records(got, w[want_key][cap], (want_key, mode, cap))
        finally:
            clf.close()


def test_no_table_where_it_was_excluded(gpu_lib, world):
    """index B (the reference's short sample array) forced wide, and a narrow load, with the variable set: no sampled table, the
    shift reported as 0, the records of the locate still right (B: the rows behind the missing sample give nothing, Truth.beyond)"""
    api = gpu_lib
    ix = load(api, world["B"]["fmi"], wide_env(1))
    try:
        assert ix.info.warnings & it.WARN_SA_SHORT and world["B"]["T"].beyond.any()
        lay = ix.layout()
        assert ix.row_tax_shift == 0 and int(lay.bytes[api.INDEX_ARRAYS.index("row_tax")]) == 0 and lay.n_dense == 0
        locate_all(api, ix, world["B"], "want_walk")
    finally:
        ix.close()
    for name in ("C", "D"):
        T = world[name]["T"]
        ix = load(api, world[name]["fmi"], {"KAIJU_GPU_KMER": "3", "KAIJU_GPU_ROW_TAX_SHIFT": "2"})
        try:
            lay = ix.layout()
            assert lay.wide == 0 and ix.row_tax_shift == 0 and int(lay.bytes[api.INDEX_ARRAYS.index("row_tax")]) == T.bwtlen * 4
            locate_all(api, ix, world[name], "want")
        finally:
            ix.close()


# ---- the locate over interval records -------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["s1", "s2", "full", "row_tax0"])
@pytest.mark.parametrize("name", ["C", "D"])
def test_intervals(gpu_lib, world, name, config):
    """s1 / s2: k_mem_locate_sampled.  full (k_mem_locate<true> + k_mem_locate_list<true>) and row_tax0 (k_mem_locate_wide) pin the
    entry point itself against kernels that were there before it"""
    api = gpu_lib
    env = {"s1": wide_env(1), "s2": wide_env(2), "full": wide_env(), "row_tax0": wide_env(row_tax="0")}[config]
    ix = load(api, world[name]["fmi"], env)
    try:
        assert ix.row_tax_shift == {"s1": 1, "s2": 2}.get(config, 0)
        assert (int(ix.layout().bytes[api.INDEX_ARRAYS.index("row_tax")]) == 0) == (config == "row_tax0")
        locate_all(api, ix, world[name], "want_walk" if config == "row_tax0" else "want")
    finally:
        ix.close()


def test_intervals_bad_arguments(gpu_lib, world):
    api, T = gpu_lib, world["C"]["T"]
    ix = load(api, world["C"]["fmi"], wide_env(1))
    clf = api.Classifier(ix, api.default_params("mem"))
    try:
        n = T.bwtlen
        ok = clf.locate_intervals([n - 1], [1], [0, 1])
        assert len(ok) == 1 and not (int(ok[0]["flags"]) & TP.INTERNAL)
        assert len(clf.locate_intervals([], [], [0])) == 0
        empty = clf.locate_intervals([5], [1], [0, 0, 1, 1])        # (records without an interval: no ids)
        assert [int(x) for x in empty["n_ids"]] == [0, int(empty[1]["n_ids"]), 0] and not empty["flags"].any()
        for lo, ln, first in (([n], [1], [0, 1]), ([n - 1], [2], [0, 1]), ([0], [n + 1], [0, 1]), ([3], [0], [0, 1]),
                              (list(range(17)), [1] * 17, [0, 17]), ([1, 2], [1, 1], [1, 2]), ([1, 2], [1, 1], [0, 2, 1])):
            with pytest.raises(api.KaijuGpuError, match="bad argument"):
                clf.locate_intervals(lo, ln, first)
        assert len(clf.locate_intervals(list(range(16)), [1] * 16, [0, 16])) == 1
        # more records than a call takes: refused before anything is read or allocated
        L = api.lib()
        assert L.kaiju_gpu_locate_intervals(clf._h, None, None, np.zeros(2, dtype=np.uint32).ctypes.data, (1 << 24) + 1, None) != 0
        assert b"KAIJU_GPU_LOCATE_MAX_RECORDS" in L.kaiju_gpu_last_error()
    finally:
        clf.close()
        ix.close()


# ---- whole classifications ------------------------------------------------------------------------------------------------
LAYOUTS = dict(TP.LAYOUTS, wide17_s1={"KAIJU_GPU_FORCE_WIDE": "17", "KAIJU_GPU_ROW_TAX_SHIFT": "1"},
               wide17_s2={"KAIJU_GPU_FORCE_WIDE": "17", "KAIJU_GPU_ROW_TAX_SHIFT": "2"})


class World(TP.World):
    def index(self, layout, id_mode=0):
        key = (layout, id_mode)
        if key not in self._idx:
            with TP.Env(LAYOUTS[layout]):
                self._idx[key] = self.api.Index(self.fmi, id_mode=id_mode)
            assert self._idx[key].info.warnings == 0
        return self._idx[key]


@pytest.fixture(scope="module")
def W(gpu_lib, oracle, tmp_path_factory):
    w = World(gpu_lib, oracle, str(tmp_path_factory.mktemp("postsearch_sampled")))
    yield w
    w.close()


@pytest.mark.parametrize("s", [1, 2])
def test_end_to_end(W, s):
    """sets 1 - 4 on a forced-wide index with the sampled table, as test_gpu_postsearch.py runs them for wide17_row_tax0: MEM with
    and without SEG (long reads, short pairs), Greedy at max_matches_SI 20 and 22, the 184-byte and the 16-byte records - every
    record the oracle's (util.same_hit), the retry pass entered by the reads of the census"""
    layout = f"wide17_s{s}"
    idx = W.index(layout)
    assert idx.row_tax_shift == s and idx.footprint.wide == 1
    for seg in (1, 0):
        TP.run_mem_sets(W, layout, seg)
    clf = W.classifier(layout, "greedy", 1)
    for name in ("greedy", "ladder", "rows"):
        sq, o, pe = W.packed(name)
        TP.check(clf, clf.classify(sq, o, paired=pe), W.want(name, "greedy", 1), W.reads(name), 0, (layout, "greedy", name))
    clf.close()
    # more best matches than the record has slots: k = 22 enters k_greedy_retry, which locates its reads itself
    clf = W.classifier(layout, "greedy", 1, mm=0, msi=22)
    reads = W.reads("greedy")
    sq, o = P.pack(reads)
    hits = clf.classify(sq, o).copy()
    TP.check(clf, hits, W.want("greedy", "greedy", 1, mm=0, msi=22), reads, sum(r.k > 21 for r in reads), (layout, "greedy msi 22"))
    clf.close()
    # the 16-byte records (k_lca behind k_mem_locate_sampled): the host LCA of the oracle's ids
    api = W.api
    for name, m in TP.MEM_SETS:
        clf = W.classifier(layout, "mem", 1, m=m)
        sq, o, pe = W.packed(name)
        want = W.want(name, "mem", 1, m=m)
        compact = clf.classify_compact(W.dtax, sq, o, paired=pe).copy()
        assert clf.stats().error_flags == 0
        exp = np.zeros(len(want), dtype=api.COMPACT_DTYPE)
        for i, w in enumerate(want):
            n = int(w["n_ids"])
            exp[i] = (W.tax.lca(w["taxid"][:n]) if n and int(w["best"]) else 0, int(w["best"]), (int(w["flags"]) & 3) << 8 | n)
        for f in ("lca", "best", "info"):
            assert (compact[f] == exp[f]).all(), (layout, name, f)
        clf.close()


@pytest.mark.parametrize("s", [1, 2])
def test_end_to_end_verbose_and_sequence_ids(W, s):
    """kaiju -v (k_mem_verbose keeps its own walk: columns 6 and 7 are those of the default index, the records the oracle's) and
    kaijux ids (the dense index of a row is its sequence) on the sampled table"""
    layout = f"wide17_s{s}"
    for mode, names in (("mem", ("rows", "ladder")), ("greedy", ("greedy",))):
        clf, ref = W.classifier(layout, mode, 1), W.classifier("default", mode, 1)
        for name in names:
            sq, o, pe = W.packed(name)
            hits, accs, peps = clf.classify_verbose(sq, o, paired=pe)
            hits0, accs0, peps0 = ref.classify_verbose(sq, o, paired=pe)
            want = W.want(name, mode, 1)
            bad = [W.reads(name)[i].name for i in range(len(want)) if not util.same_hit(want[i], hits[i])]
            assert not bad, (layout, mode, name, bad[:5])
            assert accs == accs0 and peps == peps0, (layout, mode, name)
            assert any(accs) and any(peps)
        clf.close()
        ref.close()
    assert W.index(layout, W.api.IDS_SEQUENCE).row_tax_shift == s
    for seg in (1, 0):
        TP.run_mem_sets(W, layout, seg, id_mode=W.api.IDS_SEQUENCE, what=f"kaijux {layout}")


@pytest.mark.parametrize("s", [1, 2])
def test_wavefront_layouts(W, s):
    """set 5 in batches of 1, 63, 64, 65 and 257 reads (and the large ones): a partly filled last team and block of
    k_mem_locate_sampled; every record the oracle's, and the record the read has in the large batch"""
    layout = f"wide17_s{s}"
    want = W.want("base", "mem", 1)
    clf = W.classifier(layout, "mem", 1)
    sizes, large = set(), None
    for name, order in W.orders.items():
        reads = [W.base[i] for i in order]
        sq, o = P.pack(reads)
        hits = clf.classify(sq, o).copy()
        TP.check(clf, hits, want[order], reads, TP.over(reads), (layout, "layout", name))
        if name == "front":
            large = hits[np.argsort(np.array(order))]
        assert (hits == large[order]).all(), (layout, name)
        sizes.add(len(order))
    clf.close()
    assert {1, 63, 64, 65, 257} <= sizes
