"""The window-probability table of s_Trim on the device (kj_core.h: seg_prob_lookup; capi.hip: k_seg, k_seg_teams<T>,
k_seg_table_check).  kaiju_gpu_seg_table_check computes every entry of the uploaded table again with the device's
seg_prob_of_counts: the doubles the host built are the device's, bit for bit.  Then the SEG regions of the peptides of
tests/test_seg_prob_table.py - fragments of 12 to 150 residues: the lookup, the windows past kSegTabMax, the last lane of the
prefix counts, a second round of sub-windows - with the table and with KAIJU_GPU_SEG_TABLE=0, by one wavefront and by teams of
16 lanes, SEG pass and exact pass: identical records, equal to the oracle's.  Integers and bit patterns: every comparison is exact."""
import numpy as np
import pytest

import seg_inputs as si
import util
from test_gpu_seg_regions import check_batch
from test_seg_prob_table import ENTRIES, build, info, region_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tab_max():
    import os
    return info(build(os.path.join(util.EMU_DIR, "libkaiju_seg_table_emu.so"), ()))["tab_max"]


@pytest.fixture(scope="module")
def indexes(gpu_lib, golden):
    """the golden index loaded with the table and with KAIJU_GPU_SEG_TABLE=0 (read when an index is loaded)"""
    mp = pytest.MonkeyPatch()
    mp.delenv("KAIJU_GPU_SEG_TABLE", raising=False)
    on = gpu_lib.Index(golden.fmi)
    mp.setenv("KAIJU_GPU_SEG_TABLE", "0")
    off = gpu_lib.Index(golden.fmi)
    mp.undo()
    return {"on": on, "off": off}


@pytest.fixture(scope="module")
def expected(oracle, emu, golden):
    """peptide -> (the oracle's regions, the overflow flag of the one-lane host emulation's record), computed once"""
    seg_oracle = si.SegOracle(oracle)
    h = emu.load(golden.fmi)
    cache = {}

    def get(aa):
        e = cache.get(aa)
        if e is None:
            e = cache[aa] = (np.array(seg_oracle(aa), dtype=np.int32).reshape(-1, 2), emu.seg_rec(h, aa)[1] if len(aa) >= 12 else 0)
        return e
    return get


def test_table_is_the_devices(indexes, tab_max):
    """every entry of the uploaded table == the device's seg_prob_of_counts as 64-bit patterns, found by the device's lookup"""
    for which in ("on", "off"):
        entries, mismatches = indexes[which].seg_table_check()
        assert (entries, mismatches) == (ENTRIES[tab_max], 0), which


def records(clf, reads, exact):
    seqs, off = util.pack(reads)
    frags, lr = clf.seg_regions(seqs, off, exact=exact)
    order = np.lexsort((frags["start"], frags["read"]))
    g = frags[order]
    first = g["first"].astype(np.int64)
    return g[["read", "start", "len", "flagged", "n", "overflow", "n_lr"]], [lr[first[i]: first[i] + g["n_lr"][i]].tobytes() for i in range(len(g))]


def test_regions_with_and_without_the_table(gpu_lib, indexes, expected, tab_max, monkeypatch):
    reads = region_cases(tab_max)
    assert {tab_max - 1, tab_max, tab_max + 1, 63, 64} <= {si.first_raw_segment(aa) for aa in reads}
    params = gpu_lib.default_params("greedy", seg=1, input_is_protein=1, min_fragment_length=1, min_score=0)
    got = {}
    for which, team in (("on", 64), ("off", 64), ("on", 16)):
        monkeypatch.setenv("KAIJU_GPU_SEG_TEAM", str(team))
        clf = gpu_lib.Classifier(indexes[which], params)
        try:
            # SEG pass and exact pass against the oracle, region by region
            n, flagged, small = check_batch(gpu_lib, clf, expected, team, reads, f"table {which}")
            assert n == len(reads) and flagged > len(reads) * 2 // 3 and small == 0
            got[which, team] = [records(clf, reads, exact) for exact in (False, True)]
        finally:
            clf.close()
    for key in (("off", 64), ("on", 16)):
        for exact in (0, 1):
            a, b = got["on", 64][exact], got[key][exact]
            assert np.array_equal(a[0], b[0]) and a[1] == b[1], (key, exact)
