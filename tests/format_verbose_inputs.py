"""Inputs of the tests of the -v lines (tests/test_format_verbose_emu.py on the host, tests/test_gpu_format_verbose.py on the
device): synthetic hit records, compact records, kaiju_gpu_verbose records, packed peptides, off[], name spans and the text
the names lie in, over a small database of sequence names (DB_NAMES); nothing is classified.  Every case is the smallest shape
that can break one pass of kaiju_amd/csrc/format_verbose.hip.  cases(B, S, K, index_db) wants the constants of
format_inputs.cases and db_length of the index the contexts will have (any number for the emulation).

A case is a dict of format_inputs.make plus: hits (HIT_DTYPE), v (VERBOSE_DTYPE), text_pos (uint64), pep (bytes), text_cap.

    python tests/format_verbose_inputs.py CASES    writes the accession table and every case with its expected output, the
                                                   capacity cases included, for the stand-alone build of
                                                   tests/emu/format_verbose_emu.cpp (-DFORMAT_VERBOSE_EMU_MAIN)"""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import format_inputs
from kaiju_amd import api

LONG = b"L" * 300
# (name of the database sequence, its protein - distinct, so that an index can be built of them)
DB_NAMES = [b"ACC.1_123", b"nounderscore", b"WP_000123.1_562", b"_77", b"SAME.1_10", b"SAME.1_20", b"AB_1", b"ABC_2", b"AB._3",
            b"\xc3\xa9X\x80\xff_5", LONG + b"_9", b"ZZ.9_4"] + [b"Q%02d.1_%d" % (i, 100 + i) for i in range(14)]
I_PLAIN, I_NONE, I_MANY, I_LEAD, I_SAME_A, I_SAME_B, I_AB, I_ABC, I_ABDOT, I_HIGH, I_LONG, I_ZZ, I_Q0 = range(13)
NO_SEQ = 1000000                      # a sequence number no index of these names has
INEXACT = 0x80000000
RECORD_COUNTS = (0, 1, 2, 17, 255, 256, 257, 65537)
ID_VALUES = [10 ** k for k in range(20)] + [2 ** 64 - 1, 5, 5 + 2 ** 32, 5 + 2 ** 33, 4 + 2 ** 32, 6 + 2 ** 32, 2 ** 63, 2 ** 63 + 1]
NAME_LENGTHS = (0, 1, 15, 16, 17, 255, 256, 257, 4099)
PEP_ALPHABET = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY,", dtype=np.uint8)


def index_names():
    """DB_NAMES as an index can hold them: a .fmi stores the length of a name in one byte, so the long one has 255 bytes"""
    names = list(DB_NAMES)
    names[I_LONG] = LONG[:253] + b"_9"
    assert max(len(nm) for nm in names) == 255
    return names


def db_proteins():
    """one protein per name of DB_NAMES (i.i.d. residues, fixed seed)"""
    rng = np.random.default_rng(77)
    return [bytes(rng.choice(PEP_ALPHABET[:20], 40 + 3 * i).tolist()) for i in range(len(DB_NAMES))]


def rec(name, lca=7, best=20, info=1, ids=(7,), acc=(I_PLAIN,), pep=b"", lens=(150, 0), n_ids=None, n_acc=None, text_len=None, truncated=0):
    """one record: n_ids / n_acc / text_len default to what ids / acc / pep hold"""
    return {"name": name, "lca": lca, "best": best, "info": info, "ids": list(ids), "acc": list(acc), "pep": pep, "lens": lens,
            "n_ids": len(ids) if n_ids is None else n_ids, "n_acc": len(acc) if n_acc is None else n_acc,
            "text_len": len(pep) if text_len is None else text_len, "truncated": truncated}


def make(cid, records, text_cap=0xffffffff, pep_gap=b"", **kw):
    """pep_gap: bytes (or a list of one per record) laid in front of every record's peptides in the packed string"""
    base = format_inputs.make(cid, [r["name"] for r in records], [(r["lca"], r["best"], r["info"]) for r in records],
                              lens=[r["lens"] for r in records], **kw)
    n = len(records)
    hits = np.zeros(n, dtype=api.HIT_DTYPE)
    v = np.zeros(n, dtype=api.VERBOSE_DTYPE)
    pos = np.zeros(n, dtype=np.uint64)
    parts, at = [], 0
    for r, k in enumerate(records):
        assert len(k["ids"]) <= 21 and len(k["acc"]) <= 20
        hits[r]["best"], hits[r]["n_ids"], hits[r]["flags"] = k["best"], k["n_ids"], k["info"] >> 8
        hits[r]["taxid"][: len(k["ids"])] = np.asarray(k["ids"], dtype=np.uint64)
        hits[r]["taxid"][len(k["ids"]):] = 0xdeadbeefdeadbeef          # (slots behind n_ids are unspecified)
        v[r]["n_acc"], v[r]["text_len"], v[r]["truncated"] = k["n_acc"], k["text_len"], k["truncated"]
        v[r]["acc_iseq"][: len(k["acc"])] = np.asarray(k["acc"], dtype=np.uint32)
        v[r]["acc_iseq"][len(k["acc"]):] = NO_SEQ + 1
        g = pep_gap[r] if isinstance(pep_gap, list) else pep_gap
        parts += [g, k["pep"]]
        pos[r] = at + len(g)
        at += len(g) + len(k["pep"])
    base.update(hits=hits, v=v, text_pos=pos, pep=b"".join(parts), text_cap=text_cap)
    return base


def _pep(rng, l):
    return bytes(rng.choice(PEP_ALPHABET, l).tolist())


def _counts(n, seed):
    """mostly 'U' records when n is large; classified ones with a few ids, accessions and peptides"""
    rng = np.random.default_rng(seed)
    p_c = 0.5 if n < 1000 else 0.02
    out = []
    for i in range(n):
        if rng.random() < p_c:
            k = int(rng.integers(1, 5))
            out.append(rec(b"r%d" % i, lca=int(rng.integers(1, 10 ** 6)), best=int(rng.integers(11, 300)), info=k,
                           ids=[int(x) for x in rng.integers(1, 10 ** 7, k)], acc=[int(x) for x in rng.integers(0, len(DB_NAMES), int(rng.integers(0, 6)))],
                           pep=_pep(rng, int(rng.integers(0, 40)))))
        else:
            out.append(rec(b"r%d" % i, lca=0, best=0, info=0, ids=(), acc=()))
    return out


def _orders(vals, rng):
    return [sorted(vals), sorted(vals, reverse=True), [vals[i] for i in rng.permutation(len(vals))]]


def _ids():
    rng = np.random.default_rng(9)
    out = []
    for n_ids in (0, 1, 2, 20, 21):
        for start in (0, 7, 14):
            vals = [ID_VALUES[(start + j) % len(ID_VALUES)] for j in range(n_ids)]
            for o in _orders(vals, rng):
                out.append(rec(b"ids%d" % len(out), ids=o, info=max(1, n_ids)))
    # neighbours that differ only above bit 32, twice the same value, and a count above the cap of 21 (clamped)
    out.append(rec(b"hi32", ids=[5 + 2 ** 33, 5, 6 + 2 ** 32, 5 + 2 ** 32, 4 + 2 ** 32, 2 ** 32, 2 ** 33], info=7))
    out.append(rec(b"equal", ids=[42, 42, 41], info=3))
    out.append(rec(b"over", ids=list(range(100, 121)), n_ids=25, info=21))
    return out


def _accs():
    every = list(range(len(DB_NAMES)))
    out = [rec(b"acc0", acc=()), rec(b"acc1", acc=[I_PLAIN]), rec(b"acc20", acc=every[6:26]), rec(b"acc20r", acc=every[25:5:-1]),
           rec(b"clamp", acc=every[:20], n_acc=25), rec(b"one_rank", acc=[I_SAME_A, I_SAME_B] * 10), rec(b"two_ranks", acc=[I_ZZ, I_AB] * 10),
           rec(b"none", acc=[I_NONE]), rec(b"lead", acc=[I_LEAD]), rec(b"lead_and", acc=[I_PLAIN, I_LEAD, I_NONE, I_MANY]),
           rec(b"prefixes", acc=[I_ABC, I_ABDOT, I_AB]), rec(b"high", acc=[I_HIGH, I_ZZ, I_PLAIN]), rec(b"long", acc=[I_LONG, I_Q0, I_LONG]),
           rec(b"same", acc=[I_SAME_B, I_Q0 + 3, I_SAME_A]), rec(b"no_seq", acc=[NO_SEQ, I_PLAIN, 0xffffffff]), rec(b"only_none", acc=[I_NONE] * 20),
           rec(b"first12", acc=every[:12][::-1])]
    return out


def _texts(cap):
    rng = np.random.default_rng(4)
    out = []
    for l in (0, 1, 15, 16, 17, cap):
        out.append(rec(b"pep%d" % l, pep=_pep(rng, l)))
    out.append(rec(b"cut", pep=_pep(rng, cap + 5)))                                     # text_len = cap + 5: cut, truncated
    out.append(rec(b"flag", pep=_pep(rng, 9), truncated=1))                             # cut before it got here
    out.append(rec(b"cutU", lca=0, best=0, info=0, ids=(), acc=(), pep=_pep(rng, cap + 5)))   # not classified: not counted
    return out


def _grid():
    """classified records with random gaps in front of names and peptides: every alignment (mod 16) of a name and of the
    peptides in their source against every alignment of their place in the output occurs (checked by the caller); the middle
    of a line is copied from the shadow, where it lies at the offset of its place in the output"""
    rng = np.random.default_rng(12)
    recs, ngaps, pgaps = [], [], []
    for i in range(2600):
        recs.append(rec(bytes(rng.integers(65, 91, int(rng.integers(1, 8))).tolist()), lca=int(rng.integers(1, 2000)), best=int(rng.integers(11, 99)),
                        ids=[int(x) for x in rng.integers(1, 10 ** 5, int(rng.integers(1, 4)))],
                        acc=[int(x) for x in rng.integers(0, len(DB_NAMES), int(rng.integers(0, 3))) if x != I_LONG], pep=_pep(rng, int(rng.integers(1, 24)))))
        ngaps.append(b"\n" + b"@" * int(rng.integers(1, 17)))
        pgaps.append(b"#" * int(rng.integers(0, 16)))
    return recs, ngaps, pgaps


def cases(B, S, K, index_db):
    assert S == 256
    c = []
    for n in RECORD_COUNTS:
        c.append(make("n_%d" % n, _counts(n, 200 + n)))
    c.append(make("ids", _ids()))
    c.append(make("accs", _accs()))
    c.append(make("texts", _texts(40), text_cap=40))
    rng = np.random.default_rng(5)
    alphabet = np.asarray([b for b in range(256) if b != 10], dtype=np.uint8)
    names = [bytes(rng.choice(alphabet, l).tolist()) for l in NAME_LENGTHS] + [b"tab\there", b"\xff\x80\xfe", b"last"]
    recs = [rec(nm, lca=ID_VALUES[i % len(ID_VALUES)], best=3 + i, info=2, ids=[9, 3], acc=[I_AB, I_PLAIN], pep=b"MK,LV,") if i % 3 else
            rec(nm, lca=0, info=0, ids=(), acc=()) for i, nm in enumerate(names)]
    recs[-1] = rec(b"last", lca=12, pep=b"END,")
    c.append(make("name_lengths", recs))
    recs, ngaps, pgaps = _grid()
    c.append(make("alignment_grid", recs, gap=ngaps, pep_gap=pgaps))
    # records that stay undecided, inexact ones, the largest numbers in columns 3 and 4
    recs = [rec(b"t0", lca=2 ** 64 - 1, best=2 ** 32 - 1, info=3, ids=[2 ** 64 - 1, 1, 10 ** 19]), rec(b"t1", lca=77, info=0), rec(b"t2", lca=77, best=0, info=2),
            rec(b"t3", lca=0, info=2), rec(b"t4", lca=12, info=1 | INEXACT), rec(b"t5", lca=0, info=1 | INEXACT), rec(b"t6", lca=1, best=1, info=1)]
    c.append(make("taxon_ids", recs))
    # the E-value gate, pairs and protein input: the groups of format_inputs with columns 4 to 7 added
    for k in format_inputs.cases(B, S, K, index_db):
        if not k["id"].startswith(("gate_", "nogate_")) or k["db"] != "golden":
            continue
        n = len(k["recs"])
        recs = [rec(b"g%d" % r, lca=int(k["recs"][r]["lca"]), best=int(k["recs"][r]["best"]), info=int(k["recs"][r]["info"]), ids=[int(k["recs"][r]["lca"]), 3 + r],
                    acc=[(r + j) % len(DB_NAMES) for j in range(r % 4)], pep=b"PEPTIDE," * (r % 3),
                    lens=(int(k["off"][2 * r + 1] - k["off"][2 * r]), int(k["off"][2 * r + 2] - k["off"][2 * r + 1]))) for r in range(n)]
        c.append(make(k["id"], recs, mode=k["mode"], paired=k["paired"], protein=k["protein"], min_evalue=k["min_evalue"], db="golden"))
    return c


def capacity_cases(all_cases, expect):
    """(case, out_cap): the exact length, one byte short, the end of a line in the middle, inside the first line, 0, and
    inside a 16-byte chunk of a line in the middle; expect(case) -> dict of format_verbose_expect.expected"""
    out = []
    for case in all_cases:
        if case["id"] not in ("n_17", "n_257", "name_lengths", "alignment_grid", "accs", "texts"):
            continue
        e = expect(case)
        lo = e["line_off"]
        total, mid = len(e["text"]), int(lo[len(lo) // 2])
        assert 0 < mid < total - 1 and int(lo[1]) > 1
        inside = (mid // 16) * 16 + 24 + 7                    # not a multiple of 16, behind mid
        assert inside < total
        out += [(case, total), (case, total - 1), (case, mid), (case, int(lo[1]) - 1), (case, 0), (case, inside)]
    return out


def accession_table():
    """(rank, prefix_len, blob offsets, blob) of DB_NAMES as the library makes them"""
    import ctypes as C
    n = len(DB_NAMES)
    arr = (C.c_char_p * n)(*DB_NAMES)
    rank, plen = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    assert api.lib().kaiju_accession_ranks(arr, n, rank.ctypes.data, plen.ctypes.data) == 0
    aoff = np.concatenate([[0], np.cumsum(plen, dtype=np.uint64)]).astype(np.uint64)
    blob = b"".join(nm[: int(l)] for nm, l in zip(DB_NAMES, plen))
    return rank, plen, aoff, blob


def main(path):
    import struct

    import format_verbose_expect as fve
    index_db = 54321.0
    all_cases = cases(4096, 256, 4096, index_db)
    jobs = [(k, None) for k in all_cases] + capacity_cases(all_cases, lambda k: fve.expected(k, index_db))
    pw = np.zeros(4096)
    assert api.lib().kaiju_gpu_format_evalue_table(pw.ctypes.data, len(pw)) == 0
    rank, plen, aoff, blob = accession_table()
    with open(path, "wb") as f:
        f.write(pw.tobytes())
        f.write(struct.pack("<2Q", len(DB_NAMES), len(blob)) + aoff.tobytes() + plen.tobytes() + rank.tobytes() + blob)
        for case, cap in jobs:
            e = fve.expected(case, index_db, cap)
            cap = len(e["text"]) + 5 if cap is None else cap
            n = len(case["recs"])
            f.write(struct.pack("<10Q2d", n, int(case["paired"]), len(case["text1"]), 1 if case["mode"] == "greedy" else 0, int(case["protein"]),
                                cap, len(e["written"]), case["text_cap"], len(case["pep"]), 0, index_db, case["min_evalue"]))
            info = np.zeros(1, dtype=api.FORMAT_VERBOSE_INFO_DTYPE)
            for k, v in e["info"].items():
                info[0][k] = v
            f.write(info.tobytes() + case["hits"].tobytes() + case["recs"].tobytes() + case["off"].tobytes() + case["v"].tobytes() +
                    case["text_pos"].tobytes() + case["names"].tobytes() + case["text1"] + case["pep"] + e["written"])
    print("%d cases written to %s" % (len(jobs), path))


if __name__ == "__main__":
    main(sys.argv[1])
