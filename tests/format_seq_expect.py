"""What the passes of the kaijux / kaijup lines (kaiju_amd/csrc/format_seq.hip, kj_format_seq.h) must write, built without them
from the rules at the top of kj_format_seq.h: the decision per record is the library's host function kaiju_finalize_compact (it
needs no device) on the record stage 4 makes of a hit, the ids are sorted(), the fragments of the kaijup rule a regular
expression over the twenty amino-acid letters and a table of the BLOSUM62 diagonal written out here.  A case is a dict as
tests/format_seq_inputs.py makes them; db_names: the names of the database sequences the ids refer to."""
import re

import numpy as np

import format_expect

INFO_FIELDS = ("text_bytes", "n_records", "n_classified", "overflow", "n_inexact", "n_truncated", "reserved")
INEXACT = 0x80000000
U_NUCLEOTIDE, U_PROTEIN = 0, 1
# the diagonal of BLOSUM62 (B, J, O, U, X and Z count as no amino acid: their entries are 0 in the table of the command line)
BLOSUM62_DIAGONAL = {"A": 4, "R": 5, "N": 6, "D": 6, "C": 9, "Q": 5, "E": 5, "G": 6, "H": 8, "I": 4, "L": 4, "K": 5, "M": 5, "F": 6, "P": 7,
                     "S": 4, "T": 5, "W": 11, "Y": 7, "V": 4}
_LETTERS = "".join(BLOSUM62_DIAGONAL)
_RUN = re.compile(("[" + _LETTERS + _LETTERS.lower() + "]+").encode())


def score(run):
    return sum(BLOSUM62_DIAGONAL[chr(c).upper()] for c in run)


def has_fragment(read, m, greedy, min_score):
    """a maximal run of amino-acid letters of at least m, in Greedy mode scoring at least min_score"""
    return any(len(x.group()) >= m and (not greedy or score(x.group()) >= min_score) for x in _RUN.finditer(read))


def gated(case, r):
    o = case["off"]
    l1, l2 = int(o[2 * r + 1] - o[2 * r]), int(o[2 * r + 2] - o[2 * r + 1])
    m = case["min_frag"]
    if case["u_rule"] == U_PROTEIN:
        read = case["seqs"][int(o[2 * r]): int(o[2 * r + 1])]
        return l1 < m or not has_fragment(read, m, case["mode"] == "greedy", case["min_score"])
    return (l1 < 3 * m and l2 < 3 * m) if case["paired"] else l1 < 3 * m


def seq_line(name, best, ids, db_names, pep):
    col = b"".join((db_names[q] if q < len(db_names) else b"") + b"," for q in sorted(ids))
    return b"C\t" + name + b"\t" + str(best).encode() + b"\t" + col + b"\t" + pep + b"\n"


def compact_of(hits):
    recs = np.zeros(len(hits), dtype=format_expect.api.COMPACT_DTYPE)
    recs["lca"], recs["best"], recs["info"] = (hits["n_ids"] != 0).astype(np.uint64), hits["best"], hits["n_ids"]
    return recs


def lines_of(case, res, db_names):
    out, n_trunc = [], 0
    text1, cap = case["text1"], case["text_cap"]
    for r in range(len(res)):
        p, l = int(case["names"][r]["pos"]), int(case["names"][r]["len"])
        name = bytes(text1[p:p + l])
        if not res[r]["classified"]:
            out.append(b"U\t" + name + (b"\t0\n" if gated(case, r) else b"\n"))
            continue
        h = case["hits"][r]
        ids = [int(x) for x in h["taxid"][: min(int(h["n_ids"]), 21)]]
        pep = b""
        if case["pep"] is not None:
            v = case["v"][r]
            tl, at = int(v["text_len"]), int(case["text_pos"][r])
            n_trunc += 1 if (tl > cap or int(v["truncated"])) else 0
            pep = case["pep"][at: at + min(tl, cap)]
        out.append(seq_line(name, int(h["best"]), ids, db_names, pep))
    return out, n_trunc


def expected(case, db_length, out_cap=None, db_names=None):
    """text: all lines; written: the whole lines that fit out_cap (None: everything fits); info: the fields of
    kaiju_gpu_format_verbose_info; line_off: where every line starts"""
    if db_names is None:
        import format_seq_inputs
        db_names = format_seq_inputs.DB_NAMES
    res = format_expect.finalize(format_expect.params_of(case), db_length, compact_of(case["hits"]), case["off"], case["paired"])
    lines, n_trunc = lines_of(case, res, db_names)
    text = b"".join(lines)
    line_off = np.concatenate([[0], np.cumsum([len(l) for l in lines], dtype=np.int64)]).astype(np.int64)
    cap = len(text) if out_cap is None else out_cap
    fit = int(np.searchsorted(line_off, cap, side="right")) - 1
    info = {"text_bytes": len(text), "n_records": len(lines), "n_classified": int(np.count_nonzero(res["classified"])),
            "overflow": 1 if len(text) > cap else 0, "n_inexact": int(np.count_nonzero(case["hits"]["flags"] & INEXACT)), "n_truncated": n_trunc,
            "reserved": 0}
    return {"text": text, "written": text[: int(line_off[fit])], "info": info, "line_off": line_off, "res": res, "lines": lines}
