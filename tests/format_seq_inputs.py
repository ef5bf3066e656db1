"""Inputs of the tests of the kaijux / kaijup lines (tests/test_format_seq_emu.py on the host, tests/test_gpu_format_seq.py on the
device): synthetic hit records of sequence numbers, kaiju_gpu_verbose records, packed peptides, reads, off[], name spans and
the text the names lie in, over a small database of sequence names (DB_NAMES); nothing is classified.  Every case is the
smallest shape that can break one pass of kaiju_amd/csrc/format_seq.hip.  cases(B, S, K, index_db) wants the constants of
format_inputs.cases and db_length of the index the contexts will have (any number for the emulation).

A case is a dict of format_inputs.make (its recs are the compact records stage 4 makes of the hits) plus: hits (HIT_DTYPE), v
(VERBOSE_DTYPE), text_pos (uint64), pep (bytes, None: no peptide column), text_cap, seqs (the reads off[] points into), u_rule,
min_frag, min_score.

    python tests/format_seq_inputs.py CASES    writes the name table and every case with its expected output, the capacity
                                               cases included, for the stand-alone build of tests/emu/format_seq_emu.cpp
                                               (-DFORMAT_SEQ_EMU_MAIN)"""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import format_inputs
from format_seq_expect import U_NUCLEOTIDE, U_PROTEIN, score
from kaiju_amd import api

_FILL = b"abcdefghijklmnopqrstuvwxyz0123456789"
TABLE_NAME_LENGTHS = (0, 1, 15, 16, 17, 33)
# names of the lengths above, one with '_', ',' and a tab, then ordinary ones
DB_NAMES = [(b"L%d_" % l + _FILL)[:l] for l in TABLE_NAME_LENGTHS] + [b"WP_1,2\tx_9"] + [b"Q%02d.1_%d" % (i, 100 + i) for i in range(23)]
I_EMPTY, I_ONE, I_15, I_16, I_17, I_33, I_ODD, I_Q0 = range(8)
NO_SEQ = 1000000                      # a sequence number no index of these names has
INEXACT = 0x80000000
RECORD_COUNTS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257)
BIG_COUNT = 256 * 256 + 1             # more records than one step of the block on top of the prefix sum takes
BEST_VALUES = (0, 9, 10, 99999, 4294967295)
M, MIN_SCORE = 11, 65                 # the defaults of -m and -s
PEP_ALPHABET = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY,", dtype=np.uint8)


def index_names():
    """DB_NAMES as an index built from a FASTA file can hold them: a header ends at its first blank, and a sequence has a name"""
    names = list(DB_NAMES)
    names[I_EMPTY] = b"E"
    names[I_ODD] = names[I_ODD].replace(b"\t", b"|")
    assert len(set(names)) == len(names)
    return names


def db_proteins():
    """one protein per name of DB_NAMES (i.i.d. residues, fixed seed)"""
    rng = np.random.default_rng(78)
    return [bytes(rng.choice(PEP_ALPHABET[:20], 40 + 3 * i).tolist()) for i in range(len(DB_NAMES))]


def rec(name, best=20, ids=(I_Q0,), pep=b"", lens=(150, 0), read=None, n_ids=None, flags=0, text_len=None, truncated=0):
    """one record: n_ids / text_len default to what ids / pep hold; read: the bytes of read 1 (lens[0] of them)"""
    l1 = lens[0] if read is None else len(read)
    return {"name": name, "best": best, "ids": list(ids), "n_ids": len(ids) if n_ids is None else n_ids, "flags": flags, "pep": pep,
            "lens": (l1, lens[1]), "read": b"A" * l1 if read is None else read, "text_len": len(pep) if text_len is None else text_len,
            "truncated": truncated}


def U(name, **kw):
    """a record without ids: never classified"""
    return rec(name, best=0, ids=(), **kw)


def make(cid, records, with_pep=True, text_cap=0xffffffff, pep_gap=b"", u_rule=U_NUCLEOTIDE, min_frag=M, min_score=MIN_SCORE, **kw):
    """pep_gap: bytes (or a list of one per record) laid in front of every record's peptides in the packed string"""
    base = format_inputs.make(cid, [r["name"] for r in records], [(1 if r["n_ids"] else 0, r["best"], r["n_ids"]) for r in records],
                              lens=[r["lens"] for r in records], **kw)
    n = len(records)
    hits = np.zeros(n, dtype=api.HIT_DTYPE)
    v = np.zeros(n, dtype=api.VERBOSE_DTYPE)
    pos = np.zeros(n, dtype=np.uint64)
    parts, reads, at = [], [], 0
    for r, k in enumerate(records):
        assert len(k["ids"]) <= 21
        hits[r]["best"], hits[r]["n_ids"], hits[r]["flags"] = k["best"], k["n_ids"], k["flags"]
        hits[r]["taxid"][: len(k["ids"])] = np.asarray(k["ids"], dtype=np.uint64)
        hits[r]["taxid"][len(k["ids"]):] = 0xdeadbeef                   # (slots behind n_ids are unspecified)
        v[r]["text_len"], v[r]["truncated"] = k["text_len"], k["truncated"]
        g = pep_gap[r] if isinstance(pep_gap, list) else pep_gap
        parts += [g, k["pep"]]
        pos[r] = at + len(g)
        at += len(g) + len(k["pep"])
        assert len(k["read"]) == k["lens"][0]
        reads += [k["read"], b"C" * k["lens"][1]]
    seqs = b"".join(reads)
    assert len(seqs) == (int(base["off"][-1]) if n else 0)
    base.update(hits=hits, v=v, text_pos=pos, pep=b"".join(parts) if with_pep else None, text_cap=text_cap, seqs=seqs, u_rule=u_rule,
                min_frag=min_frag, min_score=min_score)
    return base


def _pep(rng, l):
    return bytes(rng.choice(PEP_ALPHABET, l).tolist())


def _counts(n, seed):
    """'C' records with a few ids and peptides among 'U' records of both kinds"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        x = rng.random()
        if x < 0.5:
            k = int(rng.integers(1, 5))
            out.append(rec(b"r%d" % i, best=int(rng.integers(11, 300)), ids=[int(q) for q in rng.integers(0, len(DB_NAMES), k)],
                           pep=_pep(rng, int(rng.integers(0, 40)))))
        else:
            out.append(U(b"r%d" % i, lens=(150 if x < 0.75 else 20, 0)))
    return out


def _big(n):
    """short names, one matched sequence per record, a 'U' record now and then: n records cost little"""
    return [U(b"r%d" % i) if i % 7 == 3 else rec(b"r%d" % i, best=11 + i % 89, ids=(i % len(DB_NAMES),)) for i in range(n)]


def _ids():
    rng = np.random.default_rng(9)
    every = list(range(len(DB_NAMES)))
    out = []
    for n_ids in (1, 2, 20, 21):
        for start in (0, 5, 9):
            vals = [every[(start + j) % len(every)] for j in range(n_ids)]
            for o in (sorted(vals), sorted(vals, reverse=True), [vals[i] for i in rng.permutation(len(vals))]):
                out.append(rec(b"ids%d" % len(out), ids=o))
    out.append(rec(b"none", ids=(), n_ids=0))                                                    # no id: a 'U' line
    out.append(rec(b"equal", ids=[I_17, I_17, I_ONE, I_17, I_ONE]))                              # equal numbers: nothing is removed
    out.append(rec(b"over", ids=every[3:24], n_ids=25))                                          # a count above the cap of 21
    out.append(rec(b"no_seq", ids=[NO_SEQ, I_15, len(DB_NAMES), 0xffffffff]))                    # numbers that are no sequence
    out.append(rec(b"only_no_seq", ids=[NO_SEQ]))
    out.append(rec(b"lengths", ids=[I_33, I_17, I_16, I_15, I_ONE, I_EMPTY, I_ODD]))             # every length of a table name
    out.append(rec(b"empty_only", ids=[I_EMPTY]))
    out.append(rec(b"odd", ids=[I_ODD, I_ODD]))
    return out


def _texts(cap):
    rng = np.random.default_rng(4)
    out = []
    for l in (0, 1, 15, 16, 17, cap - 1, cap, cap + 1):                                          # cap + 1: cut, truncated
        out.append(rec(b"pep%d" % l, pep=_pep(rng, l)))
    out.append(rec(b"flag", pep=_pep(rng, 9), truncated=1))                                      # cut before it got here
    out.append(U(b"cutU", pep=_pep(rng, cap + 5)))                                               # not classified: not counted
    return out


def _names_and_best():
    """read names of 13, 14 and 15 bytes: "C\\t" name "\\t" ends just before, on and just after the first 16-byte boundary when
    the line starts a chunk (each of these lines is the first of a case of its own below, and they follow each other here)"""
    rng = np.random.default_rng(5)
    alphabet = np.asarray([b for b in range(256) if b != 10], dtype=np.uint8)
    names = [b"", b"n" * 13, b"n" * 14, b"n" * 15] + [bytes(rng.choice(alphabet, l).tolist()) for l in (1, 16, 17, 255, 256, 257)] + [b"tab\there", b"\xff\x80\xfe"]
    out = []
    for i, nm in enumerate(names):
        out.append(rec(nm, best=BEST_VALUES[1 + i % 4], ids=[I_Q0 + i, I_ONE], pep=b"MK,LV,"))
        out.append(U(nm, lens=(20 + 130 * (i % 2), 0)))
    for b in BEST_VALUES:
        out.append(rec(b"best%d" % b, best=b))                                                   # best 0: a 'U' line
    out.append(rec(b"inexact", flags=INEXACT))
    out.append(U(b"inexactU", flags=INEXACT | 1))
    return out


def _grid():
    """classified records with random gaps in front of names and peptides: every alignment (mod 16) of a name and of the peptides
    in their source against every alignment of their place in the output occurs (checked by the test)"""
    rng = np.random.default_rng(12)
    recs, ngaps, pgaps = [], [], []
    for i in range(2600):
        recs.append(rec(bytes(rng.integers(65, 91, int(rng.integers(1, 8))).tolist()), best=int(rng.integers(11, 99)),
                        ids=[int(x) for x in rng.integers(0, len(DB_NAMES), int(rng.integers(1, 4)))], pep=_pep(rng, int(rng.integers(1, 24)))))
        ngaps.append(b"\n" + b"@" * int(rng.integers(1, 17)))
        pgaps.append(b"#" * int(rng.integers(0, 16)))
    return recs, ngaps, pgaps


def _u_nucleotide():
    return [U(b"u_%d_%d" % (l1, l2), lens=(l1, l2)) for l1 in (3 * M - 1, 3 * M) for l2 in (0, 3 * M - 1, 3 * M)] + [rec(b"c", lens=(3 * M - 1, 0))]


def _u_protein():
    """reads of the kaijup rule: (name, read 1); all without ids"""
    w = b"W" * M
    s64 = b"WW" + b"A" * 7 + b"PP"                     # eleven letters that score 64
    s65 = b"WW" + b"A" * 6 + b"R" + b"PP"              # ... and 65
    assert len(s64) == len(s65) == M and score(s64) == MIN_SCORE - 1 and score(s65) == MIN_SCORE
    reads = [(b"empty", b""), (b"short", b"W" * (M - 1)), (b"exact", w), (b"lowA", b"A" * M), (b"two_short", b"W" * (M - 1) + b"*" + b"W" * (M - 1)),
             (b"short_then_m", b"W" * (M - 1) + b"*" + w), (b"s64", s64), (b"s65", s65), (b"s64_twice", s64 + b"X" + s64), (b"lower", b"w" * M),
             (b"mixed", b"wWyYcC" * 2), (b"at_end", b"**" + w), (b"at_end_short", w[:-1] + b"*" + b"W" * (M - 1)), (b"straddle31", b"*" * 26 + w),
             (b"straddle63", b"*" * 58 + w), (b"straddle31_short", b"*" * 27 + b"W" * (M - 1) + b"*" * 30), (b"long", b"A" * 100), (b"long_broken", (b"A" * 10 + b"-") * 9),
             (b"carry_reset", b"A" * 30 + b"W" * 4 + b"1" + b"W" * 6 + b"*" * 40), (b"not_letters", b"@[`{" * 8 + b"\x00\xff\xc1\xe1" * 4), (b"exact32", b"*" * 21 + w),
             (b"exact64", b"A" * 64), (b"sum_over_strides", b"A" * 16 + b"*" + b"A" * 17)]
    reads += [(b"break_" + bytes([c]), b"W" * (M - 1) + bytes([c]) + b"W" * (M - 1)) for c in b"BJOUXZbjouxz*"]
    return [U(nm, read=rd) for nm, rd in reads] + [rec(b"c", best=300, read=b"*" * 20)]


def cases(B, S, K, index_db):
    assert S == 256
    c = []
    for n in RECORD_COUNTS:
        c.append(make("n_%d" % n, _counts(n, 200 + n)))
    assert BIG_COUNT == S * S + 1
    c.append(make("n_%d" % BIG_COUNT, _big(BIG_COUNT), with_pep=False))
    c.append(make("ids", _ids()))
    c.append(make("ids_plain", _ids(), with_pep=False))                 # without -v: every 'C' line ends ",\t\n"
    c.append(make("texts", _texts(40), text_cap=40))
    c.append(make("names_best", _names_and_best()))
    c.append(make("names_best_plain", _names_and_best(), with_pep=False))
    for l in (13, 14, 15):
        c.append(make("first_name_%d" % l, [rec(b"n" * l, best=7, ids=[I_16]), U(b"n" * l), U(b"n" * l, lens=(20, 0))], with_pep=False))
    # spans that leave the text of the names: cut at its end, or empty
    k = make("names_past_end", [rec(b"inside"), U(b"u"), rec(b"last_name")], gap=b"\n@")
    k["names"][2]["len"] += 10
    k["names"][1]["pos"] = len(k["text1"]) + 7
    c.append(k)
    recs, ngaps, pgaps = _grid()
    c.append(make("alignment_grid", recs, gap=ngaps, pep_gap=pgaps))
    # the 'U' lines
    for pe in (False, True):
        for mode in ("mem", "greedy"):
            c.append(make("u_nt_%s_%s" % ("pairs" if pe else "single", mode), _u_nucleotide(), paired=pe, mode=mode, with_pep=False))
    c.append(make("u_nt_protein_input", _u_nucleotide(), protein=True, with_pep=False))            # kaijux -p: the nucleotide rule
    for mode in ("mem", "greedy"):
        c.append(make("u_protein_%s" % mode, _u_protein(), u_rule=U_PROTEIN, protein=True, mode=mode, with_pep=mode == "greedy"))
    c.append(make("u_protein_m5_s30", _u_protein(), u_rule=U_PROTEIN, protein=True, mode="greedy", with_pep=False, min_frag=5, min_score=30))
    # the E-value gate, pairs and protein input: the groups of format_inputs as hits with one or two ids; a record the gate rejects
    # is long enough for "U\tname\n"
    for k in format_inputs.cases(B, S, K, index_db):
        if not k["id"].startswith(("gate_", "nogate_")):
            continue
        n = len(k["recs"])
        recs = [rec(b"g%d" % r, best=int(k["recs"][r]["best"]), ids=[(r + j) % len(DB_NAMES) for j in range(1 + r % 2)], pep=b"PEPTIDE," * (r % 3),
                    lens=(int(k["off"][2 * r + 1] - k["off"][2 * r]), int(k["off"][2 * r + 2] - k["off"][2 * r + 1]))) for r in range(n)]
        c.append(make(k["id"], recs, mode=k["mode"], paired=k["paired"], protein=k["protein"], min_evalue=k["min_evalue"], db=k["db"],
                      u_rule=U_PROTEIN if k["protein"] else U_NUCLEOTIDE))
    return c


CAPACITY_IDS = ("n_3", "n_65", "n_257", "names_best", "alignment_grid", "ids_plain", "texts", "u_protein_greedy")


def capacity_cases(all_cases, expect):
    """(case, out_cap): 0, one byte short, the exact length, one byte more, and capacities that cut inside the first line, a line
    in the middle (not at a multiple of 16) and the last line; expect(case) -> dict of format_seq_expect.expected"""
    out = []
    for case in all_cases:
        if case["id"] not in CAPACITY_IDS:
            continue
        e = expect(case)
        lo = e["line_off"]
        total, mid = len(e["text"]), int(lo[len(lo) // 2])
        assert 0 < mid < total - 1 and int(lo[1]) > 1 and total - int(lo[-2]) > 2
        inside = mid + 1 if (mid + 1) % 16 else mid + 2
        assert inside < int(lo[len(lo) // 2 + 1])
        out += [(case, 0), (case, total - 1), (case, total), (case, total + 1), (case, int(lo[1]) - 1), (case, inside), (case, int(lo[-2]) + 1), (case, mid)]
    return out


def name_table(names=None):
    """(lengths, blob offsets, blob) of the names as the library lays them out"""
    names = DB_NAMES if names is None else names
    slen = np.asarray([len(nm) for nm in names], dtype=np.uint32)
    soff = np.concatenate([[0], np.cumsum(slen, dtype=np.uint64)]).astype(np.uint64)
    return slen, soff, b"".join(names)


def main(path):
    import struct

    import format_seq_expect as fse
    index_db = 54321.0
    all_cases = cases(4096, 256, 4096, index_db)
    dbl = lambda case: index_db if case["db"] == "golden" else case["db"]
    jobs = [(k, None) for k in all_cases] + capacity_cases(all_cases, lambda k: fse.expected(k, dbl(k)))
    pw = np.zeros(4096)
    assert api.lib().kaiju_gpu_format_evalue_table(pw.ctypes.data, len(pw)) == 0
    slen, soff, blob = name_table()
    with open(path, "wb") as f:
        f.write(pw.tobytes())
        f.write(struct.pack("<2Q", len(DB_NAMES), len(blob)) + soff.tobytes() + slen.tobytes() + blob)
        for case, cap in jobs:
            e = fse.expected(case, dbl(case), cap)
            cap = len(e["text"]) + 5 if cap is None else cap
            n = len(case["hits"])
            pep = case["pep"] or b""
            f.write(struct.pack("<16Q2d", n, int(case["paired"]), len(case["text1"]), 1 if case["mode"] == "greedy" else 0, int(case["protein"]),
                                cap, len(e["written"]), case["text_cap"], len(pep), 0 if case["pep"] is None else 1, case["u_rule"], case["min_frag"],
                                case["min_score"], 1 if case["mode"] == "greedy" else 0, len(case["seqs"]), 0, dbl(case), case["min_evalue"]))
            info = np.zeros(1, dtype=api.FORMAT_VERBOSE_INFO_DTYPE)
            for k, v in e["info"].items():
                info[0][k] = v
            f.write(info.tobytes() + case["hits"].tobytes() + case["off"].tobytes() + case["v"].tobytes() + case["text_pos"].tobytes() +
                    case["names"].tobytes() + case["text1"] + pep + case["seqs"] + e["written"])
    print("%d cases written to %s" % (len(jobs), path))


if __name__ == "__main__":
    main(sys.argv[1])
