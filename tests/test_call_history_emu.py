"""Records do not depend on what the working memory held before a call - the host's half (the device's: test_gpu_call_history.py).

The emulation (tests/emu/kernel_emu.cpp) allocates fresh arrays for every call, so a context's history is put into them by
hand: emu_set_fill() starts every working array (peptide area, fragment lists, read descriptors, SegRecs, the scratch of the
lanes, of the retry pass and of the exact pass) as a byte pattern repeated, emu_set_hits() starts the hit records as the
records of another call wherever the product's plan does not clear them (kj_flow.h: clear_out - the fused MEM path with the
16-byte records).  Every result must equal the oracle's and the run on zeroed memory.

Every call of the emulation allocates its arrays afresh, so the cases that are about memory carried from one call to the next
(layout_*, shrink* with its empty call, routes_*) reduce here to pattern runs of each call with the other calls' records as
the residue of hit records; carried memory itself is the device test's.  The exception is the peptide area of the
continuation cases, which emu_set_carry() hands from A to B.

On the plan that does not clear, the comparison covers best, n_ids, flags and the first n_ids ids of every record: what
include/kaiju_gpu.h specifies there.  The id slots behind n_ids are unspecified and the only thing left out."""
import ctypes as C
import os

import numpy as np
import pytest

import history_cases as H
import postsearch_inputs as P
import util

LAYOUTS = {"narrow": {}, "wide16": {"KAIJU_GPU_FORCE_WIDE": "16"}}
K_HIT_RETRY, K_HIT_LOC_PENDING, K_WIN_MULTI, K_WIN_FORCE = 0x40000000, 0x20000000, 0x80000000, 0xffffffff    # kj_core.h


@pytest.fixture(scope="module")
def worlds(oracle, golden, tmp_path_factory):
    I = P.inputs()
    _, fmi, nodes = P.write_db(I, str(tmp_path_factory.mktemp("history")))
    return {"golden": {"fmi": golden.fmi, "ix": oracle.load_fmi(golden.fmi), "tax": oracle.load_nodes(golden.nodes)},
            "motif": {"fmi": fmi, "ix": oracle.load_fmi(fmi), "tax": oracle.load_nodes(nodes)}}


def db_text(emu, h):
    n = C.c_uint64(0)
    emu.lib.emu_text.restype = C.c_void_p
    emu.lib.emu_text.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    p = emu.lib.emu_text(h, C.byref(n))
    return bytes(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,))) if p and n.value else b""


def patterns(emu, h):
    """zeros, ones, a mixed byte, one residue code repeated (A, L, W and the last code: what a window that reads too far
    would take for more of the read) and a slice of the database text itself (narrow indexes keep it)"""
    out = {"00": b"\x00", "ff": b"\xff", "a5": b"\xa5", "A": b"\x01", "L": b"\x0a", "W": b"\x13", "Y": b"\x14"}
    text = db_text(emu, h)
    if text:
        out["text"] = text[70: 70 + 4099]
    return out


def poison(n, seed=3):
    """hit records as a search could have left them in the middle of its work: the internal flags, the lazy-SEG notes, id
    counts up to the cap"""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=util.GPU_HIT)
    r["best"] = rng.integers(11, 300, n)
    r["n_ids"] = rng.integers(0, 22, n)
    r["flags"] = rng.choice([K_HIT_RETRY, K_HIT_LOC_PENDING, K_HIT_RETRY | K_HIT_LOC_PENDING, 1, 3, 0xffffffff], n)
    r["reserved"] = rng.choice([K_WIN_FORCE, K_WIN_MULTI | 1, K_WIN_MULTI | 7, 1, 2, 900], n)
    r["taxid"] = rng.integers(1, 1 << 40, (n, 21))
    return r


def check_call(emu, h, oracle, w, call, mode, seg, m, protein, pats, residues, tag, emu_kw=None):
    """one call on zeroed memory == the oracle; under every pattern and every residue of hit records == the zeroed run"""
    emu_kw = emu_kw or {}
    gp = util.gp(mode, m=m, seg=seg, protein=protein)
    emu.set_fill(b"")
    emu.set_hits(None)
    zero, nretry = emu.classify(h, gp, call.seqs, call.off, paired=call.paired, **emu_kw)
    want = oracle.classify(w["ix"], w["tax"], oracle.params(mode, seg=seg, use_evalue=0, min_fragment_length=m, protein=protein),
                           call.seqs, call.off, paired=call.paired)
    bad = [i for i in range(call.n) if not util.same_hit(want[i], zero[i])]
    assert not bad, (tag, "zeroed memory vs the oracle", bad[:5])
    unclear = 0
    clears = False        # the plan clears the hit records whatever they held (Greedy, wide, eager SEG): a residue changes nothing
    try:
        for pname, pat in pats.items():
            for rname, res in [("none", None)] + ([] if clears else list(residues.items())):
                emu.set_fill(pat)
                emu.set_hits(res)
                got, nr = emu.classify(h, gp, call.seqs, call.off, paired=call.paired, **emu_kw)
                assert nr == nretry, (tag, pname, rname, nr, nretry)
                if emu.lib.emu_last_clear_out():
                    clears = clears or res is not None
                    assert (got == zero).all(), (tag, pname, rname, np.nonzero(got != zero)[0][:5])
                else:
                    unclear += res is not None
                    assert H.specified_equal(got, zero), (tag, pname, rname)
                    assert not (got["flags"] & 0xe0000000).any(), (tag, pname, rname)     # no internal flag leaves the library
    finally:
        emu.set_fill(b"")
        emu.set_hits(None)
    return zero, nretry, unclear


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_golden_reads_under_every_pattern(oracle, golden, worlds, layout, monkeypatch):
    """the golden reads (all of them: the general stage 1; the short ones: the fast stage 1 and lazy SEG; the pairs), MEM and
    Greedy, SEG on and off; the hit records start as the same call's records rotated by one read and as poisoned records"""
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    emu = util.Emu()
    h = emu.load(golden.fmi)
    pats = patterns(emu, h)
    short = [r for r in golden.reads if len(r) <= 150]
    unclear = 0
    try:
        for call in (H.Call("all", golden.reads), H.Call("short", short), H.Call("pairs", golden.p1, golden.p2)):
            for mode in ("mem", "greedy"):
                for seg in (1, 0):
                    emu.set_fill(b"")
                    emu.set_hits(None)
                    own, _ = emu.classify(h, util.gp(mode, seg=seg), call.seqs, call.off, paired=call.paired)
                    res = {"rotated": np.roll(own, 1), "poison": poison(call.n)}
                    unclear += check_call(emu, h, oracle, worlds["golden"], call, mode, seg, 11, 0, pats, res, (layout, call.name, mode, seg))[2]
    finally:
        emu.lib.emu_index_free(h)
    # the plan that leaves the hit records alone was among them: the fused MEM path of a narrow index
    assert (unclear > 0) == (layout == "narrow"), unclear


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("world", ["golden", "motif"])
def test_history_cases(oracle, worlds, world, layout, monkeypatch):
    """every case of history_cases.py: each call under every pattern, the hit records starting as those of the case's other
    calls (a longer list wraps, a shorter one is repeated)"""
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    emu = util.Emu()
    w = worlds[world]
    h = emu.load(w["fmi"])
    pats = patterns(emu, h)
    # (every pattern: test_golden_reads_under_every_pattern; here the ones that differ in kind)
    pats = {k: pats[k] for k in (("ff", "a5", "L", "text") if layout == "narrow" else ("ff", "L"))}
    cases = [c for c in (H.golden_cases() if world == "golden" else H.motif_cases()) if c.host]
    assert len(cases) >= 4
    try:
        for case in cases:
            for mode in case.modes:
                for seg in case.segs:
                    first, retries = {}, {}
                    for call in case.calls:
                        emu.set_fill(b"")
                        emu.set_hits(None)
                        first[call.name], retries[call.name] = emu.classify(h, util.gp(mode, m=case.m, seg=seg, protein=int(case.protein)), call.seqs, call.off, paired=call.paired)
                    for call in case.calls if case.chain else case.calls[-1:]:
                        res = {"of " + k: v for k, v in first.items() if k != call.name and len(v)}
                        res["poison"] = poison(max(call.n, 1))
                        check_call(emu, h, oracle, w, call, mode, seg, case.m, int(case.protein), pats, res, (layout, case.name, call.name, mode, seg))
                    # the routes are entered: the retry pass by the reads with more than 16 longest matches
                    if case.name in ("routes_pairs", "routes_single"):
                        assert retries[case.calls[0].name] > 0 and retries[case.victim.name] == 0, (case.name, retries)
        # ... the lazy-SEG listing and the second search by reads whose answer SEG changes ('lc', 'across'), the many-rows locate
        # by reads with more than kLocDeferRows = 8 rows, the exact pass by fragments with more than 15 SEG regions
        by = H.by_name(cases)
        if world == "motif":
            A = by["routes_pairs"].calls[0]
            o1, o0 = (oracle.classify(w["ix"], w["tax"], oracle.params("mem", seg=sg, use_evalue=0, min_fragment_length=8), A.seqs, A.off, paired=True) for sg in (1, 0))
            assert any(int(a["n_ids"]) != int(b["n_ids"]) for a, b in zip(o1, o0))
            I = P.inputs()
            assert sum(r.rows > 8 for r in I.kept["rows"] if P.list_bound(r)) >= 10 and sum(r.rung[0] == "pairrows" for r in I.kept["pairs"]) >= 3
        else:
            assert max(len(oracle.seg(s)) for s in util.many_region_reads()[0]) > 15
    finally:
        emu.lib.emu_index_free(h)


@pytest.mark.parametrize("name,q,e,kind,mode,seg,stage1,env", H.CONTINUATION, ids=[c[0] for c in H.CONTINUATION])
def test_continuation_cases_are_armed(oracle, worlds, golden, name, q, e, kind, mode, seg, stage1, env, monkeypatch):
    """the over-read trap, for every stage 1 (Team, Fast, FastTrig, Long, LongTrig, Old): B runs on the peptide area as A
    left it, and AFTER B the bytes behind the fragment that ends its match are stale letters that continue the match in the
    database (asserted on the memory B's lanes saw, history_cases.continuation_armed).  B's records of that very run == the
    oracle's - in MEM mode the match keeps its length; and B under every fill pattern"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    emu = util.Emu()
    h = emu.load(golden.fmi)
    w = worlds["golden"]
    case = H.by_name(H.golden_cases())[name]
    try:
        got = H.continuation_armed(emu, h, case, mode, seg, stage1)
        B = case.victim
        want = oracle.classify(w["ix"], w["tax"], oracle.params(mode, seg=seg, use_evalue=0), B.seqs, B.off, paired=B.paired)
        assert all(util.same_hit(a, b) for a, b in zip(want, got))
        assert int(got[B.n - 1]["best"]) == q if mode == "mem" else int(got[B.n - 1]["best"]) > 0      # (found, and not a letter longer)
        for md in ("mem", "greedy"):
            for sg in (1, 0):
                check_call(emu, h, oracle, w, B, md, sg, 11, 0, patterns(emu, h), {"poison": poison(B.n)}, (name, md, sg))
    finally:
        emu.lib.emu_index_free(h)


def test_small_bounds_build_spills_and_retries(oracle, golden, worlds):
    """the lanes built with tiny bounds (-DKJ_G_SMALL): match lists spill from the rows to global scratch and reads take the
    retry pass, whose scratch starts as a pattern too"""
    small = util.Emu(so=os.path.join(util.EMU_DIR, "libkaiju_kernel_emu_small.so"), defines=("KJ_G_SMALL",))
    h = small.load(golden.fmi)
    pats = {k: v for k, v in patterns(small, h).items() if k in ("ff", "L", "text")}
    total = 0
    try:
        for call in (H.Call("all", golden.reads), H.Call("pairs", golden.p1, golden.p2), H.Call("long", util.long_reads(n=40))):
            for mode in ("greedy", "mem"):
                for seg in (1, 0):
                    total += check_call(small, h, oracle, worlds["golden"], call, mode, seg, 11, 0, pats, {"poison": poison(call.n)}, ("small", call.name, mode, seg))[1]
    finally:
        small.lib.emu_index_free(h)
    assert total > 0


@pytest.mark.parametrize("lanes", ["v2", "v1"])
@pytest.mark.parametrize("mode", ["mem", "greedy"])
def test_verbose_buffers_under_every_pattern(golden, mode, lanes, monkeypatch):
    """kaiju -v: the accession and text buffers start as a pattern, the counts cleared as the product clears them (n * 4 bytes
    of each); the counts, the accessions announced and the text of every read == the run on zeroed buffers, with the working
    memory filled as well.  Second-generation lanes + mem_verbose_read and the first-generation lanes"""
    if lanes == "v1":
        monkeypatch.setenv("KAIJU_EMU_VERBOSE_V1", "1")
    emu = util.Emu()
    h = emu.load(golden.fmi)
    E = emu.lib
    E.emu_set_verbose.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    cap = 8192
    short = H.Call("short", [r for r in golden.reads if len(r) <= 150][:200])
    try:
        for call in (short, H.Call("pairs", golden.p1, golden.p2), H.Call("all", golden.reads[-120:])):
            n = call.n
            runs = {}
            for pname, pat in patterns(emu, h).items():
                nacc, tlen = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
                acc = np.resize(np.frombuffer(pat * 4, dtype=np.uint32), n * 20).copy()
                text = np.resize(np.frombuffer(pat, dtype=np.uint8), n * cap).copy()
                E.emu_set_verbose(nacc.ctypes.data, acc.ctypes.data, tlen.ctypes.data, text.ctypes.data, cap)
                emu.set_fill(b"" if pname == "00" else pat)
                gh, _ = emu.classify(h, util.gp(mode, seg=1), call.seqs, call.off, paired=call.paired)
                runs[pname] = (gh.tobytes(), nacc.tobytes(), tlen.tobytes(), [acc[r * 20: r * 20 + int(nacc[r])].tobytes() for r in range(n)],
                               [text[r * cap: r * cap + int(tlen[r])].tobytes() for r in range(n)])
            assert sum(len(t) for t in runs["00"][4]) > 0
            for pname, got in runs.items():
                assert got == runs["00"], (mode, lanes, call.name, pname, [i for i in range(5) if got[i] != runs["00"][i]])
    finally:
        E.emu_set_verbose(None, None, None, None, 0)
        emu.set_fill(b"")
        emu.lib.emu_index_free(h)
