"""The device SEG pass, region by region: kaiju_gpu_seg_regions (stage 1 of protein reads, then launch_seg - k_seg or
k_seg_teams<T> by KAIJU_GPU_SEG_TEAM - or k_redo_seg of the exact pass) against the oracle's SeqBufferSeg for every fragment.
The other GPU tests see classification records only, which an off-by-one region, a lost tie-break or a stale LDS slice
rarely changes.  SEG results are integers: every comparison is exact.  tests/test_seg_lanes.py runs the same inputs through
the same code with several lanes on the host."""
import time

import numpy as np
import pytest

import seg_inputs as si
import util

pytestmark = pytest.mark.gpu

TEAMS = (64, 32, 16, 8)
REC = 15             # regions of a record of the SEG pass (kj_core.h: kSegRecRegions)


@pytest.fixture(scope="module")
def gidx(gpu_lib, golden):
    return gpu_lib.Index(golden.fmi)


@pytest.fixture(scope="module")
def expected(oracle, emu, golden):
    """peptide -> (the oracle's regions, the overflow flag of the one-lane host emulation's record), computed once"""
    seg_oracle = si.SegOracle(oracle)
    h = emu.load(golden.fmi)
    cache = {}

    def get(aa):
        e = cache.get(aa)
        if e is None:
            regs = seg_oracle(aa)
            e = cache[aa] = (np.array(regs, dtype=np.int32).reshape(-1, 2), emu.seg_rec(h, aa)[1] if len(aa) >= 12 else 0)
        return e
    return get


@pytest.fixture
def clf(gpu_lib, gidx, monkeypatch, request):
    team = request.node.callspec.params["team"]
    monkeypatch.setenv("KAIJU_GPU_SEG_TEAM", str(team))
    # the Greedy flow (stage 1, SEG pass, no split in between) with every run of residues a fragment
    c = gpu_lib.Classifier(gidx, gpu_lib.default_params("greedy", seg=1, input_is_protein=1, min_fragment_length=1, min_score=0))
    t0 = time.time()
    yield c
    print(f"[seg regions] team {team}: {request.node.name} {time.time() - t0:.2f} s")
    c.close()


def check_batch(api, clf, expected, team, reads, what):
    """every fragment of the batch, SEG pass proper and exact pass; returns (fragments, flagged ones, records with the overflow
    flag among fragments of at most 15 regions and 65535 residues)"""
    seqs, off = util.pack(reads)
    want = [(r, start, frag) for r, read in enumerate(reads) for start, frag in si.fragments_of(read)]
    w_read = np.array([w[0] for w in want], dtype=np.uint32)
    w_start = np.array([w[1] for w in want], dtype=np.uint32)
    w_len = np.array([len(w[2]) for w in want], dtype=np.uint32)
    exp = [expected(w[2]) for w in want]
    e_n = np.array([len(e[0]) for e in exp], dtype=np.uint32)
    e_ov = np.array([e[1] for e in exp], dtype=np.uint32)
    e_flag = (e_n > 0).astype(np.uint32)
    assert not e_flag[w_len < 12].any()
    small_overflows = 0
    for exact in (False, True):
        frags, lr = clf.seg_regions(seqs, off, exact=exact)
        st = clf.stats()
        assert st.error_flags == 0, (what, team, exact, st.error_flags)
        assert len(frags) == len(want), (what, team, exact, len(frags), len(want))
        g = frags[np.lexsort((frags["start"], frags["read"]))]
        assert np.array_equal(g["read"], w_read) and np.array_equal(g["start"], w_start) and np.array_equal(g["len"], w_len), (what, team)
        first = g["first"].astype(np.int64)

        def explain(i, why):
            got = lr[first[i]: first[i] + g["n_lr"][i]].tolist()
            return (f"{what}, team {team}, {'exact pass' if exact else 'SEG pass'}: {why}\n  read {want[i][0]} start {want[i][1]} "
                    f"peptide {want[i][2].decode() if len(want[i][2]) < 400 else str(len(want[i][2])) + ' residues'}\n"
                    f"  device flagged {g['flagged'][i]} n {g['n'][i]} overflow {g['overflow'][i]} {got}\n"
                    f"  oracle {exp[i][0].tolist()}  (overflow flag of the one-lane emulation {exp[i][1]})")

        # 1. flagged <=> the oracle reports a region (never below 12 residues)
        bad = np.flatnonzero(g["flagged"] != e_flag)
        assert not len(bad), explain(bad[0], "flagged <=> the oracle reports a region")
        assert st.n_seg_fragments == int(e_flag.sum())
        fl = np.flatnonzero(e_flag)
        if not exact:
            assert (g["n_lr"][fl] == REC).all() and not g["n_lr"][e_flag == 0].any()
            # 3. the overflow flag is the one-lane emulation's
            bad = np.flatnonzero(g["overflow"] != e_ov)
            assert not len(bad), explain(bad[0], "overflow flag != the one-lane emulation's")
            small_overflows = int(((g["overflow"] == 1) & (e_n <= REC) & (w_len <= 65535)).sum())
            # 2. without overflow: the oracle's list, unused entries 0
            ok = fl[g["overflow"][fl] == 0]
            bad = ok[g["n"][ok] != e_n[ok]]
            assert not len(bad), explain(bad[0], "region count")
            got15 = lr[first[ok][:, None] + np.arange(REC)[None, :]]
            exp15 = np.zeros((len(ok), REC, 2), dtype=np.int32)
            for k, i in enumerate(ok):
                exp15[k, : e_n[i]] = exp[i][0]
            bad = ok[(got15 != exp15).any(axis=(1, 2))]
            assert not len(bad), explain(bad[0], "regions (unused entries are 0)")
        else:
            # 4. the exact pass: the oracle's full list whatever the count, nothing lost
            assert not (g["n"][fl] == api.SEG_LOST).any(), (what, team)
            bad = np.flatnonzero((g["n"] != e_n) | (g["n_lr"] != e_n))
            assert not len(bad), explain(bad[0], "region count")
            for i in fl:
                if not np.array_equal(lr[first[i]: first[i] + e_n[i]], exp[i][0]):
                    raise AssertionError(explain(i, "regions"))
    return len(want), int(e_flag.sum()), small_overflows


@pytest.mark.parametrize("team", TEAMS)
def test_window_ties_and_limits(gpu_lib, clf, expected, team):
    """lengths round the 12-window; repeats whose sub-windows tie in s_Trim (the tie-break of reduce_min decides the trimmed
    ends); raw segments round the packed-count limit (63) and the trim limit (50 window lengths)"""
    n, flagged, _ = check_batch(gpu_lib, clf, expected, team, si.window_cases(), "window")
    assert (n, flagged) == (10, 3)                    # the homopolymers of 12, 13 and 24 residues
    ties = si.tie_cases()
    n, flagged, small = check_batch(gpu_lib, clf, expected, team, ties, "ties")
    assert n == flagged == 2580 and small == 0
    # ... and palindromes where the minimum of s_Trim IS tied between a window and its mirror image
    wit = si.tie_witnesses(lambda aa: [tuple(r) for r in expected(aa)[0].tolist()])
    n, flagged, small = check_batch(gpu_lib, clf, expected, team, wit, "tied minimum of s_Trim")
    assert n == flagged == len(wit) == 32 and small == 0
    limits = si.limit_cases()
    assert {62, 63, 64, 65} <= {si.first_raw_segment(aa) for aa in limits}
    n, flagged, small = check_batch(gpu_lib, clf, expected, team, limits, "limits")
    assert n == flagged == len(limits) and small == 0


@pytest.mark.parametrize("team", TEAMS)
def test_stage_limits(gpu_lib, clf, expected, team):
    """fragments of 255 .. 2049 residues, on both sides of every team's LDS stage (past it the fragment is read from device
    memory and scanned without the window classes): alone in a batch, and between short fragments whose teams' slices of
    the stage, the classes and the lists lie next to theirs"""
    cases = si.stage_cases()
    assert [len(aa) for aa in cases] == list(si.STAGE_LENGTHS)
    for aa in cases:
        assert len(expected(aa)[0]) >= 3
        n, flagged, small = check_batch(gpu_lib, clf, expected, team, [aa], f"stage, {len(aa)} residues alone")
        assert (n, flagged, small) == (1, 1, 0)
    short = [aa for aa in si.short_flagged_candidates() if len(expected(aa)[0])]
    reads = []
    for k, aa in enumerate(cases):
        reads += short[7 * k: 7 * k + 7] + [aa]
    reads += short[84: 84 + 7]
    n, flagged, small = check_batch(gpu_lib, clf, expected, team, reads, "stage, between short fragments")
    assert n == flagged == len(reads) and small == 0


@pytest.mark.parametrize("team", TEAMS)
def test_record_limits(gpu_lib, clf, expected, team):
    """fragments with 14, 15, 16 (a record holds 15 regions), 31, 32, 33 (the scan lists hold 32 segments) and 43 regions, and a
    protein of more than 65535 residues (16-bit positions): the record where it holds the list, its overflow flag, the
    exact pass's list always"""
    cases = si.record_cases()
    assert [len(expected(aa)[0]) for aa in cases.values()] == [14, 15, 16, 31, 32, 33, 43] == sorted(cases)
    assert [expected(aa)[1] for aa in cases.values()] == [0, 0, 1, 1, 1, 1, 1]
    n, flagged, small = check_batch(gpu_lib, clf, expected, team, list(cases.values()), "record limits")
    assert (n, flagged, small) == (7, 7, 0)
    long = si.long_case()
    regs, ov = expected(long)
    assert len(long) > 65535 and len(regs) >= 4 and regs[-1][0] > 65535 and regs[-2][0] < 65535 < regs[-2][1] and ov == 1
    n, flagged, small = check_batch(gpu_lib, clf, expected, team, [cases[14], long, cases[16]], "long protein")
    assert (n, flagged, small) == (3, 3, 0)


@pytest.mark.parametrize("team", TEAMS)
def test_grid_stride_and_partial_teams(gpu_lib, clf, expected, team):
    """more fragments than the SEG grid takes in one trip (CUs * 32 blocks of 64 / team fragments; 256 CUs assumed: with that
    many or fewer every block takes a second trip) plus 3, so that the last group of teams is partly empty"""
    short = [aa for aa in si.short_flagged_candidates() if len(expected(aa)[0])]
    assert len(short) >= 150 and all(14 <= len(aa) <= 40 for aa in short)
    count = 256 * 32 * (64 // team) + 3
    reads = [short[k % len(short)] for k in range(count)]
    n, flagged, small = check_batch(gpu_lib, clf, expected, team, reads, "grid stride")
    assert n == flagged == count and small == 0


@pytest.mark.parametrize("team", TEAMS)
def test_fuzz_and_known_answers(gpu_lib, clf, expected, team):
    """1500 peptides of 12 .. 150 residues with a planted stretch (the generator and seed of
    test_kernel_emu.py::test_seg_known_answers) and the known answers of tests/golden/kat_seg.json"""
    kat = si.kat_cases()
    for aa, regs in kat:
        assert expected(aa)[0].tolist() == [list(r) for r in regs], aa
    fuzz = si.fuzz_cases()
    reads = fuzz + [aa for aa, _ in kat]
    n, flagged, small = check_batch(gpu_lib, clf, expected, team, reads, "fuzz")
    assert n == len(reads) and flagged > 1000
    # no record of a fragment with at most 15 regions overflows (none does in the one-lane emulation, checked on the host)
    assert small == 0


@pytest.mark.parametrize("team", TEAMS)
def test_separators(gpu_lib, clf, expected, team):
    """reads that stage 1 cuts at X, * and letters that are no amino acid, residues in lower case: several fragments per
    read, region positions relative to each fragment's start"""
    reads = si.separator_cases()
    per_read = [len(si.fragments_of(r)) for r in reads]
    assert max(per_read) >= 4 and min(per_read) == 0
    n, flagged, small = check_batch(gpu_lib, clf, expected, team, reads, "separators")
    assert n == sum(per_read) and flagged >= 40 and small == 0
