"""The post-search inputs on the host (tests/postsearch_inputs.py; the device's half: test_gpu_postsearch.py): the census
conditions - the reads are what they were designed to be, by a count that knows nothing of the code under test - and
oracle == emulation on every set, narrow and forced wide, with the retry pass entered exactly where the device test expects
it.  The emulation compiles the host branches of mem_locate_read and walks a team's rows one after the other: what only the
device compiles is the device test's."""
import collections
import ctypes as C

import numpy as np
import pytest

import postsearch_inputs as P
import util


@pytest.fixture(scope="module")
def I():
    return P.inputs()


@pytest.fixture(scope="module")
def db(I, tmp_path_factory, oracle):
    faa, fmi, nodes = P.write_db(I, str(tmp_path_factory.mktemp("postsearch")))
    return {"fmi": fmi, "nodes": nodes, "ix": oracle.load_fmi(fmi), "tax": oracle.load_nodes(nodes)}


# every rung and variant the sets are there for: (set, rung)
def required_rungs():
    out = [("ladder", ("k", k, v)) for k in list(range(1, 19)) + [21, 22] for v in ("one", "spread")]
    out += [("rows", ("rows", t, n)) for t, n in ((1, 1), (2, 1), (2, 2), (7, 1), (7, 2), (8, 1), (8, 2), (9, 1), (9, 2), (10, 1), (10, 2),
                                                   (16, 1), (16, 2), (40, 1), (40, 2), (80, 2), (20, 1), (20, 2), (21, 2), (24, 1))]
    out += [("pairs", ("pair", k)) for k in (0, 1, 2, 3, 8, 16, 17, 18)]
    out += [("pairs", r) for r in (("multi", "mates"), ("multi", "stop"), ("lc", "beside"), ("lc", "across"), ("pairrows", 9), ("pairrows", 10))]
    out += [("short", ("single", k)) for k in (1, 2, 3)] + [("short", ("force", k)) for k in (17, 18, 40)]
    out += [("greedy", ("greedy", k, kind)) for k in range(1, 23) for kind in ("g1", "g9")]
    return out


def test_census_conditions(I):
    """at most 5 % of the designed reads differ from their design (a chance match); every rung keeps at least 3 reads"""
    designed = sum(len(v) for v in I.designed.values())
    dropped = sum(len(v) for v in I.dropped.values())
    assert dropped <= 0.05 * designed, {k: [r.name for r in v] for k, v in I.dropped.items() if v}
    for name in ("ladder", "rows", "pairs", "short", "greedy"):
        assert len(I.dropped[name]) <= 0.05 * len(I.designed[name]), name
    kept = collections.Counter((s, r.rung) for s, v in I.kept.items() for r in v)
    short = [(key, kept[key]) for key in required_rungs() if kept[key] < 3]
    assert not short, short
    assert min(kept[("ladder", ("k", k, v))] for k in list(range(1, 19)) + [21, 22] for v in ("one", "spread")) >= 4
    # the database: a few hundred proteins of 50 .. 120 residues; not the reference's short sample array (no row -> taxon table)
    assert 300 <= len(I.db) <= 900 and len(I.db) % 8 != 0 and all(50 <= len(s) <= 120 for _, _, s in I.db)
    for c in P.COPIES[1:]:
        assert I.motifs[f"c{c}one"].copies == c and len(set(I.motifs[f"c{c}one"].taxa)) == 1
        few = I.motifs[f"c{c}{'five' if c >= 24 else 'few'}"]
        assert few.copies == c and len(set(few.taxa)) == min(c, 5)
    assert all(len(set(I.motifs[f"c{c}many"].taxa)) == c > 21 for c in (24, 40))
    # every read set is long / short as its flow needs
    assert all(len(r.nt1) > 287 for s in ("ladder", "rows", "fill") for r in I.kept[s])
    assert all(len(r.nt1) <= 287 and len(r.nt2) <= 287 for s in ("pairs", "short") for r in I.kept[s])
    # the layouts of set 5: wavefronts with 64, one, a few and no list-bound reads; partial last blocks
    base, orders = P.layout_orders(I)
    lb = [P.list_bound(base[i]) for i in orders["front"]]
    assert all(lb[:65]) and not any(lb[-64:]) and 900 <= len(base) <= 1100
    per = [P.list_bound(base[i]) for i in orders["one_per_64"]]
    assert all(sum(per[w: w + 64]) == 1 and per[w] for w in range(0, len(per), 64)) and len(per) % 64
    assert sorted(orders["perm"]) == list(range(len(base)))
    po = P.pair_orders(I)
    pk = [I.kept["pairs"][i].k for i in po["front"]]
    assert all(k > 16 for k in pk[:70]) and all(k == 0 for k in pk[70:140]) and len(pk) % 64 and sorted(po["perm"]) == sorted(po["front"])
    pk = [I.kept["pairs"][i].k for i in po["one_per_64"]]
    assert all(pk[w] > 16 and not any(pk[w + 1: w + 64]) for w in range(0, len(pk), 64)) and len(pk) % 64


def test_taxonomy_depths(I, db):
    """the LCAs of the motifs' taxa land on species, genera, families, the root - and on ids that nodes.dmp does not have"""
    from kaiju_amd import api
    tax = api.Taxonomy(db["nodes"])
    lcas = {m.name: tax.lca(sorted(set(m.taxa))) for m in I.motifs.values()}
    levels = collections.Counter("root" if v == 1 else "family" if v < 1000 else "genus" if v < 100000 else "species" if v < 900000 else "missing"
                                 for v in lcas.values())
    assert all(levels[k] >= 2 for k in ("root", "family", "genus", "species")), levels
    assert lcas["x1"] == P.MISSING[0] and lcas["x2"] == I.motifs["x2"].taxa[1]      # alone: as it is; next to a known id: dropped


def expect(oracle, db, mode, seg, reads, m=11, mm=3, kaijux=0, msi=20):
    s, o = P.pack(reads)
    pe = any(r.nt2 for r in reads)
    return oracle.classify(db["ix"], db["tax"], oracle.params(mode, seg=seg, use_evalue=0, min_fragment_length=m, mismatches=mm, kaijux=kaijux,
                                                               max_matches_SI=msi), s, o, paired=pe), s, o, pe


MEM_SETS = (("ladder", 11), ("rows", 11), ("fill", 11), ("pairs", 8), ("short", 8))


def test_census_is_what_the_oracle_finds(I, db, oracle):
    """MEM without SEG: the longest match of every read has the motif's length exactly when the census counted one; with the
    low-complexity run ACROSS a motif SEG changes the answer, with the run beside it the answer stays"""
    for name, m in MEM_SETS:
        want = expect(oracle, db, "mem", 0, I.kept[name], m=m)[0]
        bad = [r.name for r, w in zip(I.kept[name], want) if int(w["best"]) != (r.mlen if r.k else 0)]
        assert not bad, bad[:5]
    w0, w1 = (expect(oracle, db, "mem", seg, I.kept["pairs"], m=8)[0] for seg in (0, 1))
    for r, a, b in zip(I.kept["pairs"], w0, w1):
        if r.rung == ("lc", "across"):
            assert int(b["n_ids"]) < int(a["n_ids"]) and int(b["best"]) == 8, r.name
        elif r.rung == ("lc", "beside"):      # (the fragment is shorter behind the cut: searched at another turn, the same ids)
            assert int(a["best"]) == int(b["best"]) and sorted(a["taxid"]) == sorted(b["taxid"]), r.name
        else:
            assert util.same_hit(a, b), r.name
    # ids: none, one, two, 21 without the cap's flag, the cap
    w = expect(oracle, db, "mem", 0, I.kept["rows"] + I.kept["fill"])[0]
    seen = {(int(x["n_ids"]), int(x["flags"]) & 1) for x in w}
    assert {(0, 0), (1, 0), (2, 0), (20, 0), (21, 0), (21, 1)} <= seen, sorted(seen)


@pytest.mark.parametrize("layout", ["narrow", "wide17", "wide17_walks", "no_text", "lazy_off"])
def test_emulation_equals_oracle(I, db, oracle, layout, monkeypatch):
    """MEM (SEG on and off) over sets 1, 2, 3 and the plain reads of set 5, Greedy over set 4 (mismatches 0 and the default) and
    sets 1 and 2; the retry pass takes exactly the reads with more than 16 longest matches (MEM).  Greedy at the default
    max_matches_SI = 20: none - the 20 best matches fit a record's 21 slots, KAIJU_HIT_SI_CAP marks the reads with more.  Greedy
    with max_matches_SI raised to 22 and to 64: the reads with more than 21 best matches (nbest > kMaxIds)"""
    for k, v in {"narrow": {}, "lazy_off": {"KAIJU_EMU_LAZY_OFF": "1"}, "wide17": {"KAIJU_GPU_FORCE_WIDE": "17"}, "no_text": {"KAIJU_EMU_NO_TEXT": "1"},
                 "wide17_walks": {"KAIJU_GPU_FORCE_WIDE": "17", "KAIJU_EMU_NO_ROW_TAX": "1"}}[layout].items():
        monkeypatch.setenv(k, v)
    emu = util.Emu()
    h = emu.load(db["fmi"])
    assert emu.lib.emu_index_warnings(h) == 0
    try:
        for seg in (0, 1):
            for name, m in MEM_SETS:
                reads = I.kept[name]
                want, s, o, pe = expect(oracle, db, "mem", seg, reads, m=m)
                got, nretry = emu.classify(h, util.gp("mem", m=m, seg=seg), s, o, paired=pe)
                bad = [reads[i].name for i in range(len(reads)) if not util.same_hit(want[i], got[i])]
                assert not bad, (layout, seg, name, bad[:5])
                over = sum(r.k > 16 for r in reads)
                assert nretry == over and (nretry > 0) == (name in ("ladder", "pairs", "short")), (layout, seg, name, nretry, over)
        for mm in (0, 3):
            for name in ("greedy", "ladder", "rows"):
                reads = I.kept[name]
                want, s, o, pe = expect(oracle, db, "greedy", 1, reads, mm=mm)
                got, nretry = emu.classify(h, util.gp("greedy", mismatches=mm, seg=1), s, o, paired=pe)
                bad = [reads[i].name for i in range(len(reads)) if not util.same_hit(want[i], got[i])]
                assert not bad, (layout, mm, name, bad[:5])
                assert nretry == 0, (layout, mm, name, nretry)
                if name == "greedy" and mm == 0:      # exact matches only: k best matches of one score, the flag from the 21st on
                    assert [bool(int(w["flags"]) & 2) for w in want] == [r.k > 20 for r in reads]
            # max_matches_SI raised by the caller: 22 best matches do not fit the record, the read goes to the retry pass
            for msi in (22, 64):
                reads = I.kept["greedy"]
                for keep in (21, 22):
                    sub = [r for r in reads if r.k <= keep]
                    want, s, o, pe = expect(oracle, db, "greedy", 1, sub, mm=mm, msi=msi)
                    gp = util.gp("greedy", mismatches=mm, seg=1)
                    gp.max_matches_SI = msi
                    got, nretry = emu.classify(h, gp, s, o)
                    bad = [sub[i].name for i in range(len(sub)) if not util.same_hit(want[i], got[i])]
                    assert not bad, (layout, mm, msi, bad[:5])
                    if mm == 0:       # exact matches only: the best matches are the k occurrences
                        assert nretry == sum(r.k > 21 for r in sub) and (nretry > 0) == (keep == 22), (layout, msi, keep, nretry)
                    elif keep == 22:  # (with substitutions several variants of one occurrence tie: more best matches than occurrences)
                        assert nretry >= sum(r.k > 21 for r in sub) >= 1, (layout, msi, nretry)
        # the orders of the short pairs (the seglist ballot of the device): every record is the read's own
        pairs = I.kept["pairs"]
        want = expect(oracle, db, "mem", 1, pairs, m=8)[0]
        for oname, order in P.pair_orders(I).items():
            sub = [pairs[i] for i in order]
            s, o = P.pack(sub)
            got, nretry = emu.classify(h, util.gp("mem", m=8, seg=1), s, o, paired=True)
            assert all(util.same_hit(want[i], g) for i, g in zip(order, got)) and nretry == sum(r.k > 16 for r in sub), (layout, oname)
    finally:
        emu.lib.emu_index_free(h)


def test_emulation_equals_oracle_first_generation_lane_and_kaijux(I, db, oracle, monkeypatch):
    """KAIJU_EMU_LANE=v1 (the product's KAIJU_GPU_MEM_LANE=v1: the lanes that walk to the ids themselves, si_cap = 16 as well)
    and kaijux ids (kParamXOrder: the matches in the order maxMatches(.., 1) lists them)"""
    emu = util.Emu()
    emu.lib.emu_index_load_x.restype = C.c_void_p
    emu.lib.emu_index_load_x.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    err = C.create_string_buffer(256)
    hx = emu.lib.emu_index_load_x(db["fmi"].encode(), err, 256)
    assert hx, err.value
    h = emu.load(db["fmi"])
    for seg in (0, 1):
        for name, m in MEM_SETS:
            reads = I.kept[name]
            over = sum(r.k > 16 for r in reads)
            want, s, o, pe = expect(oracle, db, "mem", seg, reads, m=m, kaijux=1)
            got, nretry = emu.classify(hx, util.gp("mem", m=m, seg=seg), s, o, paired=pe)
            bad = [reads[i].name for i in range(len(reads)) if not util.same_hit(want[i], got[i])]
            assert not bad and nretry == over, ("kaijux", seg, name, bad[:5], nretry, over)
            want = expect(oracle, db, "mem", seg, reads, m=m)[0]
            monkeypatch.setenv("KAIJU_EMU_LANE", "v1")
            got, nretry = emu.classify(h, util.gp("mem", m=m, seg=seg), s, o, paired=pe)
            monkeypatch.delenv("KAIJU_EMU_LANE")
            bad = [reads[i].name for i in range(len(reads)) if not util.same_hit(want[i], got[i])]
            assert not bad and nretry == over, ("v1", seg, name, bad[:5], nretry, over)
    emu.lib.emu_index_free(h)
    emu.lib.emu_index_free(hx)
