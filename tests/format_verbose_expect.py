"""What the passes of the -v lines (kaiju_amd/csrc/format_verbose.hip, kj_format_verbose.h) must write, built without them from
the rules at the top of kj_format_verbose.h: the decision per record is the library's host function kaiju_finalize_compact (it
needs no device), the ids are sorted(), the accessions sorted(set()) of the prefixes as bytes.  A case is a dict as
tests/format_verbose_inputs.py makes them; db_names: the names of the database sequences the accession numbers refer to."""
import numpy as np

import format_expect

INFO_FIELDS = ("text_bytes", "n_records", "n_classified", "overflow", "n_inexact", "n_truncated", "reserved")
INEXACT = 0x80000000


def prefix(name):
    """the accession of a sequence name: up to, not including, its last '_'; None: the name has none"""
    k = name.rfind(b"_")
    return None if k < 0 else name[:k]


def verbose_line(name, taxon, best, ids, acc_names, pep):
    accs = sorted({p for p in (prefix(nm) for nm in acc_names if nm is not None) if p is not None})
    return (b"C\t" + name + b"\t" + str(taxon).encode() + b"\t" + str(best).encode() + b"\t" + b"".join(str(i).encode() + b"," for i in sorted(ids)) +
            b"\t" + b"".join(a + b"," for a in accs) + b"\t" + pep + b"\n")


def lines_of(case, res, db_names):
    out, n_trunc = [], 0
    text1, cap = case["text1"], case["text_cap"]
    for r in range(len(res)):
        p, l = int(case["names"][r]["pos"]), int(case["names"][r]["len"])
        name = bytes(text1[p:p + l])
        if not res[r]["classified"]:
            out.append(b"U\t" + name + b"\t0\n")
            continue
        h, v = case["hits"][r], case["v"][r]
        ids = [int(x) for x in h["taxid"][: min(int(h["n_ids"]), 21)]]
        seqs = [int(x) for x in v["acc_iseq"][: min(int(v["n_acc"]), 20)]]
        tl, at = int(v["text_len"]), int(case["text_pos"][r])
        n_trunc += 1 if (tl > cap or int(v["truncated"])) else 0
        out.append(verbose_line(name, int(res[r]["taxon"]), int(case["recs"][r]["best"]), ids, [db_names[q] if q < len(db_names) else None for q in seqs],
                                case["pep"][at: at + min(tl, cap)]))
    return out, n_trunc


def expected(case, db_length, out_cap=None, db_names=None):
    """text: all lines; written: the whole lines that fit out_cap (None: everything fits); info: the fields of
    kaiju_gpu_format_verbose_info; line_off: where every line starts"""
    if db_names is None:
        import format_verbose_inputs
        db_names = format_verbose_inputs.DB_NAMES
    res = format_expect.finalize(format_expect.params_of(case), db_length, case["recs"], case["off"], case["paired"])
    lines, n_trunc = lines_of(case, res, db_names)
    text = b"".join(lines)
    line_off = np.concatenate([[0], np.cumsum([len(l) for l in lines], dtype=np.int64)]).astype(np.int64)
    cap = len(text) if out_cap is None else out_cap
    fit = int(np.searchsorted(line_off, cap, side="right")) - 1
    info = {"text_bytes": len(text), "n_records": len(lines), "n_classified": int(np.count_nonzero(res["classified"])),
            "overflow": 1 if len(text) > cap else 0, "n_inexact": int(np.count_nonzero(case["recs"]["info"] & INEXACT)), "n_truncated": n_trunc,
            "reserved": 0}
    return {"text": text, "written": text[: int(line_off[fit])], "info": info, "line_off": line_off, "res": res}
