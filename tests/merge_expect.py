"""What kaiju-mergeOutputs makes of any two texts of lines, restated from the rules of kaiju_amd/csrc/kj_merge.h
(kaiju-mergeOutputs.cpp:110-295, :355-399 and util.cpp:42-77 of the reference) with Python's own strings, dicts and Decimal:
the text, the kaiju_gpu_merge_info, the summary of -v and the cut at a capacity.  tests/test_merge_expect_golden.py pins this
file byte for byte to the reference tool's own outputs; every other test of the merger compares with it."""
import re
from decimal import Decimal

MODES = ("1", "2", "lca", "lowest")
MODE_CODE = {"1": 0, "2": 1, "lca": 2, "lowest": 3}
STOP = {"none": 0, "1_class": 1, "1_tabs": 2, "1_column": 3, "2_short": 4, "2_class": 5, "2_tabs": 6, "2_column": 7, "names": 8, "score_wide": 9}
INFO_FIELDS = ("text_bytes", "used1", "used2", "n_pairs", "count", "count_c1", "count_c2", "count_c12", "count_c3", "count_c1_not_c2",
               "count_c2_not_c1", "stop_pair", "stop_why", "more_in_2", "overflow")
NO_PAIR = 2 ** 64 - 1
DIGITS = b"0123456789"


def split_lines(text, final=True):
    """the lines without their newline; a trailing newline opens no line; without `final` only lines a newline ends"""
    lines = text.split(b"\n")
    return lines[:-1] if text.endswith(b"\n") or not text or not final else lines


def parse_nodes(data):
    """node -> parent as parseNodesDmp reads it: the first two numbers of a line that starts with a digit; the first line of an id wins"""
    parent = {}
    for line in data.split(b"\n"):
        m = re.match(rb"([0-9]+)[^0-9]+([0-9]+)", line)
        if m and int(m.group(1)) < 2 ** 64 and int(m.group(2)) < 2 ** 64:
            parent.setdefault(int(m.group(1)), int(m.group(2)))
    return parent


def stoul(s):
    """the number of an id, or None"""
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?)([0-9]+)", s)
    if not m or int(m.group(2)) >= 2 ** 64:
        return None
    return (-int(m.group(2))) % 2 ** 64 if m.group(1) == b"-" else int(m.group(2))


def lineage(parent, n):
    out = [n]
    while parent[n] != n:
        n = parent[n]
        out.append(n)
    return out


def mlca(parent, id1, id2):
    n1, n2 = stoul(id1), stoul(id2)
    if n1 is None or n2 is None or (n1 not in parent and n2 not in parent):
        return 0
    if n1 not in parent:
        return n2
    if n2 not in parent:
        return n1
    mine = set(lineage(parent, n1))
    x = parent[n2]
    while x not in mine and x != parent[x]:
        x = parent[x]
    return x


def anc(parent, ida, idb):
    a, b = stoul(ida), stoul(idb)
    return a is not None and b is not None and a in parent and b in parent and a in lineage(parent, b)


class ScoreWide(Exception):
    pass


def score_value(s):
    """the Decimal a score text stands for, 0 where stod gives up (no digit, above the largest double); ScoreWide outside the
    domain the device compares exactly"""
    m = re.match(rb"[0-9]+\.?[0-9]*|\.[0-9]+", s)
    if not m:
        return Decimal(0)
    d = Decimal(m.group(0).decode())
    if d == 0:
        return Decimal(0)
    exp = d.adjusted()
    if exp >= 309:
        return Decimal(0)
    significant = "".join(map(str, d.as_tuple().digits)).strip("0")
    if len(significant) > 15 or exp >= 300 or exp < -300:
        raise ScoreWide(s)
    return d


def parse(line, use_score):
    """(why, classified, name, id, score): why one of None, "class", "tabs", "column"; score None without the column"""
    if line[:1] not in (b"C", b"U"):
        return "class", None, None, None, None
    t1 = line.find(b"\t")
    t2 = line.find(b"\t", t1 + 1) if t1 >= 0 else -1
    if t2 < 0:
        return "tabs", None, None, None, None
    c = line[:1] == b"C"
    if use_score and c:
        t3 = line.find(b"\t", t2 + 1)
        if t3 < 0 or t3 == len(line) - 1:
            return "column", None, None, None, None
        return None, c, line[t1 + 1:t2], line[t2 + 1:t3], re.match(rb"[.0-9]*", line[t3 + 1:]).group(0)
    if t2 == len(line) - 1:
        return "column", None, None, None, None
    return None, c, line[t1 + 1:t2], re.match(rb"[0-9]*", line[t2 + 1:]).group(0), None


def one_pair(parent, l1, l2, mode, use_score):
    """(output, kind) or (None, why)"""
    why, c1, name1, id1, s1 = parse(l1, use_score)
    if why:
        return None, "1_" + why
    if l2 is None:
        return None, "2_short"
    why, c2, name2, id2, s2 = parse(l2, use_score)
    if why:
        return None, "2_" + why
    if name1 != name2:
        return None, "names"
    tail = lambda i, s: i + (b"\t" + s if s is not None else b"") + b"\n"
    head = b"C\t" + name1 + b"\t"
    if not c1 and not c2:
        return b"U\t" + name1 + b"\t0\n", "u"
    if not c2:
        return head + tail(id1, s1), "c1"
    if not c1:
        return head + tail(id2, s2), "c2"
    try:
        d1, d2 = (score_value(s1), score_value(s2)) if use_score else (0, 0)
    except ScoreWide:
        return None, "score_wide"
    if id1 == id2:
        return head + tail(id1, s2 if d2 > d1 else s1), "c12"
    if d1 != d2:
        return head + (tail(id1, s1) if d1 > d2 else tail(id2, s2)), "c12"
    if mode == "1":
        pick = id1
    elif mode == "2":
        pick = id2
    elif mode == "lowest" and anc(parent, id1, id2):
        pick = id2
    elif mode == "lowest" and anc(parent, id2, id1):
        pick = id1
    else:
        L = mlca(parent, id1, id2)
        pick = b"%d" % L if L else id1
    return head + tail(pick, s1), "c12"


def summary(info):
    """the seven lines of -v"""
    n = info["count"]
    rows = (("         classified in file1:", "count_c1"), ("            but not in file2:", "count_c1_not_c2"), ("         classified in file2:", "count_c2"),
            ("            but not in file1:", "count_c2_not_c1"), ("          classified in both:", "count_c12"), ("         combined classified:", "count_c3"))
    out = ["Number of all reads in input:\t%10u\n" % n]
    for label, f in rows:
        k = info[f]
        out.append("%s\t%10u  %s\n" % (label, k, "%6.2f%%" % (k / n * 100.0) if n else "  -nan%"))
    return "".join(out)


def expected(parent, text1, text2, mode="lca", use_score=False, final=True, out_cap=None):
    """a dict: text (every line in front of the stop), written (those that end at or in front of out_cap), info"""
    L1, L2 = split_lines(text1, final), split_lines(text2, final)
    n_pairs = min(len(L1), len(L2))
    outs, kinds, stop, why = [], {}, NO_PAIR, "none"
    for k in range(len(L1) if final else n_pairs):
        out, kind = one_pair(parent, L1[k], L2[k] if k < len(L2) else None, mode, use_score)
        if out is None:
            stop, why = k, kind
            break
        outs.append(out)
        kinds[kind] = kinds.get(kind, 0) + 1
    full = b"".join(outs)
    cap = len(full) if out_cap is None else out_cap
    fit, size = 0, 0
    for o in outs:
        if size + len(o) > cap:
            break
        size += len(o)
        fit += 1
    c = lambda k: kinds.get(k, 0)
    used = lambda L, text: len(text) if final else sum(len(l) + 1 for l in L[:n_pairs])
    info = {"text_bytes": len(full), "used1": used(L1, text1), "used2": used(L2, text2), "n_pairs": n_pairs,
            "count": len(outs) + (stop != NO_PAIR), "count_c1": c("c1") + c("c12"), "count_c2": c("c2") + c("c12"), "count_c12": c("c12"),
            "count_c3": c("c1") + c("c2") + c("c12"), "count_c1_not_c2": c("c1"), "count_c2_not_c1": c("c2"), "stop_pair": stop,
            "stop_why": STOP[why], "more_in_2": 1 if final and stop == NO_PAIR and len(L2) > len(L1) and L2[len(L1)] != b"" else 0,
            "overflow": 1 if len(full) > cap else 0}
    return {"text": full, "written": full[:size], "info": info}
