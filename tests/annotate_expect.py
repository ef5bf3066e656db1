"""What kaiju-addTaxonNames makes of any text of lines, restated from the rules of kaiju_amd/csrc/kj_annotate.h
(kaiju-addTaxonNames.cpp:133-228 of the reference) over names_expect.Names: the text, where every line's output starts, the
kaiju_gpu_annotate_info and the cut at a capacity.  tests/test_annotate_expect_golden.py pins this file byte for byte to the
reference tool's own outputs; every other test of the annotator compares with it."""
import numpy as np

DIGITS = b"0123456789"
INFO_FIELDS = ("text_bytes", "n_lines", "n_c_lines", "n_annotated", "n_bad_id", "n_unknown_taxon", "n_unnamed_taxon", "n_dropped", "n_empty", "overflow")


def split_lines(text):
    """the lines without their newline; a trailing newline opens no line"""
    if not text:
        return []
    lines = text.split(b"\n")
    return lines[:-1] if text.endswith(b"\n") else lines


def read_id(line):
    """the id of a 'C' line, or None: fewer than two tabs, no digit behind the second, a value above 2^64 - 1"""
    t1 = line.find(b"\t")
    t2 = line.find(b"\t", t1 + 1) if t1 >= 0 else -1
    if t2 < 0:
        return None
    end = t2 + 1
    while end < len(line) and line[end] in DIGITS:
        end += 1
    if end == t2 + 1 or int(line[t2 + 1:end]) >= 2 ** 64:
        return None
    return int(line[t2 + 1:end])


def one_line(names, line, drop):
    """(output bytes, why): why one of annotated, bad_id, unknown, unnamed, dropped, empty, other"""
    if not line:
        return b"", "empty"
    if line[:1] != b"C":
        return (b"", "dropped") if drop else (line + b"\n", "other")
    tid = read_id(line)
    if tid is None:
        return line + b"\n", "bad_id"
    why = names.why_unchanged(tid)
    if why is not None:
        return line + b"\n", why
    return line + b"\t" + names.annotation(tid) + b"\n", "annotated"


def expected(names, text, drop_unclassified=False, out_cap=None):
    """a dict: text (everything), written (the lines that end at or in front of out_cap), line_off (int64, one more than
    lines), info"""
    outs, count = [], {}
    for line in split_lines(text):
        out, why = one_line(names, line, drop_unclassified)
        outs.append(out)
        count[why] = count.get(why, 0) + 1
    full = b"".join(outs)
    line_off = np.concatenate([[0], np.cumsum([len(o) for o in outs], dtype=np.int64)]).astype(np.int64)
    cap = len(full) if out_cap is None else out_cap
    fit = int(np.searchsorted(line_off, cap, side="right")) - 1
    c = lambda k: count.get(k, 0)
    info = {"text_bytes": len(full), "n_lines": len(outs), "n_c_lines": c("annotated") + c("bad_id") + c("unknown") + c("unnamed"),
            "n_annotated": c("annotated"), "n_bad_id": c("bad_id"), "n_unknown_taxon": c("unknown"), "n_unnamed_taxon": c("unnamed"),
            "n_dropped": c("dropped"), "n_empty": c("empty"), "overflow": 1 if len(full) > cap else 0}
    return {"text": full, "written": full[: int(line_off[fit])], "line_off": line_off, "info": info}
