"""Golden files of the merger:  python tests/golden/make_golden_merge.py

The unmodified reference tool is compiled by the pattern rules of oracle/Makefile (its object, util.o and those of bwt/) and
linked into oracle/_ref/kaiju-mergeOutputs (git-ignored), as tests/golden/make_golden_names.py builds its tool.  Only data is
written, under tests/golden/merge/: inputs, the tool's outputs gzip'ed, and the seven summary lines of -v as text.

  odd/      nodes.dmp (a forest with two self-parent roots), in1.tsv, in2.tsv: every kind of pair the tool's loop tells apart.
            out_<mode>[_s].tsv.gz / sum_<mode>[_s].txt for -c 1, 2, lca, lowest, each without and with -s;
            out_lowest_notree[_s]: -c lowest without -t
  stops/    <case>.1.tsv, <case>.2.tsv, <case>.out.tsv.gz, <case>.sum.txt: one pair of files per reason the loop breaks for,
            text 1 longer, text 2 longer, text 2 longer by one empty line.  A case whose name ends in _s is run with -s;
            all with -c 1
  real/     tests/golden/ref_mem_1.tsv against ref_greedy_1.tsv (the reference's kaiju -v on the committed reads) over
            tests/golden/nodes.dmp: out_<mode>[_s].tsv.gz / sum_<mode>[_s].txt"""
import gzip
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
TOOL = os.path.join(REF, "kaiju-mergeOutputs")
OUT = os.path.join(HERE, "merge")
MODES = ("1", "2", "lca", "lowest")
BWT = ["_ref/obj/bwt/%s.o" % f for f in ("bwt", "compactfmi", "sequence", "suffixArray")]


def build_tool():
    objs = ["_ref/obj/kaiju-mergeOutputs.o", "_ref/obj/util.o"] + BWT
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")] + objs, check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["g++", "-o", TOOL] + [os.path.join(ROOT, "oracle", o) for o in objs] + ["-lpthread", "-lz"], check=True)


def tool(in1, in2, out, summary, *args):
    """runs the tool with -v; keeps its output gzip'ed and the summary lines of its stderr"""
    r = subprocess.run([TOOL, "-i", in1, "-j", in2, "-o", out, "-v"] + list(args), check=True, stderr=subprocess.PIPE)
    with open(out, "rb") as f, open(out + ".gz", "wb") as g, gzip.GzipFile(fileobj=g, mode="wb", mtime=0, filename="") as z:
        z.write(f.read())                              # (byte for byte what the tool wrote)
    os.remove(out)
    err = r.stderr.decode("latin-1")
    with open(summary, "w") as f:
        f.write(err[err.rindex("Number of all reads in input:"):])
    print(out + ".gz", os.path.getsize(out + ".gz"))


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)


ODD_NODES = b"".join(b"%d\t|\t%d\t|\tno rank\t|\n" % p for p in (
    (1, 1), (2, 1), (3, 2), (4, 3), (5, 3), (6, 2), (7, 1), (100, 100), (101, 100), (102, 101), (18446744073709551614, 7), (1234567890, 6),
    (1234567890123456789, 1234567890), (9999999999999999999, 1234567890)))


def odd_pairs():
    """(line of text 1, line of text 2); 'C' lines carry a score column, so the same files run without and with -s"""
    c = lambda name, tid, score=b"10", rest=b"": b"C\t" + name + b"\t" + tid + b"\t" + score + rest
    u = lambda name, rest=b"": b"U\t" + name + b"\t0" + rest
    P = [(u(b"uu"), u(b"uu")), (c(b"cu", b"4"), u(b"cu")), (u(b"uc"), c(b"uc", b"5", b"7.5")),
         (c(b"same", b"4", b"10"), c(b"same", b"4", b"10")), (c(b"same_hi2", b"4", b"10"), c(b"same_hi2", b"4", b"11")),
         (c(b"same_hi1", b"4", b"12"), c(b"same_hi1", b"4", b"11")),
         (c(b"diff_hi1", b"4", b"12"), c(b"diff_hi1", b"5", b"11")), (c(b"diff_hi2", b"4", b"9"), c(b"diff_hi2", b"5", b"11.5"))]
    # equal scores: the conflict modes
    ids = [(b"4", b"5"), (b"3", b"4"), (b"4", b"3"), (b"04", b"4"), (b"4", b"04"), (b"4", b"102"), (b"102", b"4"), (b"1", b"100"), (b"100", b"1"),
           (b"1", b"7"), (b"7", b"1"), (b"6", b"4"), (b"2", b"2 "), (b"999", b"4"), (b"4", b"999"), (b"998", b"999"), (b"-3", b"4"), (b"4", b"-3"),
           (b" +4", b"5"), (b"5", b" +4"), (b"x", b"4"), (b"4", b"x"), (b"", b"4"), (b"4", b""), (b"12345678901234567890123", b"4"),
           (b"4", b"12345678901234567890123"), (b"-1", b"4"), (b"4", b"-1"), (b"-1", b"-2"), (b"18446744073709551614", b"4"),
           (b"1234567890123456789", b"9999999999999999999"), (b"9999999999999999999", b"4"), (b"4", b"18446744073709551614"),
           (b"7abc", b"7"), (b"\r4", b"5"), (b"0", b"4"), (b"4", b"0"), (b"-18446744073709551612", b"5"), (b"18446744073709551616", b"4")]
    for k, (a, b) in enumerate(ids):
        P.append((c(b"conflict%d" % k, a), c(b"conflict%d" % k, b)))
    # score texts: pairs the tool calls equal, and pairs it does not
    scores = [(b"1.20", b"1.2"), (b"007", b"7"), (b"5.", b"5"), (b".5", b"0.5"), (b".", b"0"), (b"1.2.3", b"1.2"), (b"9" * 400, b"2"), (b"2", b"9" * 400),
              (b"", b"0"), (b"", b"1"), (b"1.21", b"1.2"), (b"1.2", b"1.21"), (b"10", b"9"), (b"0.000", b"."), (b"1" + b"0" * 30, b"1" + b"0" * 29),
              (b"0." + b"0" * 40 + b"1", b"0." + b"0" * 41 + b"9"), (b"100", b"100.000"), (b"123456789012345", b"123456789012346")]
    for k, (a, b) in enumerate(scores):
        rest = b"" if a else b"\tbehind an empty score"
        P.append((c(b"score%d" % k, b"4", a, rest), c(b"score%d" % k, b"5", b)))
        P.append((c(b"score_same_id%d" % k, b"4", a, rest), c(b"score_same_id%d" % k, b"4", b)))
    P += [(c(b"cr", b"4", b"10", b"\r"), c(b"cr", b"5", b"10", b"\r")), (u(b"cr_u", b"\r"), c(b"cr_u", b"5", b"3\r")), (c(b"cr in\rname", b"3"), u(b"cr in\rname")),
          (c(b"nul\0name", b"4"), c(b"nul\0name", b"5")), (c(b"", b"4"), c(b"", b"5")), (c(b"score_tail", b"4", b"10abc"), c(b"score_tail", b"5", b"10.0e7")),
          # kaiju -v: seven columns
          (c(b"verbose", b"4", b"312", b"\t4,3,\tacc1,acc2,\tMKVLA,"), c(b"verbose", b"5", b"312", b"\t5,\tacc3,\tMKV,")),
          (c(b"verbose_u", b"4", b"312", b"\t4,3,\tacc1,acc2,\tMKVLA,"), u(b"verbose_u")),
          (c(b"n" * 5000, b"4"), c(b"n" * 5000, b"5")), (u(b"u" * 40), u(b"u" * 40)),
          (c(b"no newline at the end", b"102", b"3"), c(b"no newline at the end", b"101", b"3"))]
    return P


def odd():
    d = os.path.join(OUT, "odd")
    os.makedirs(d, exist_ok=True)
    P = odd_pairs()
    a = [os.path.join(d, "in1.tsv"), os.path.join(d, "in2.tsv")]
    write(a[0], b"\n".join(p[0] for p in P))
    write(a[1], b"\n".join(p[1] for p in P))
    nodes = os.path.join(d, "nodes.dmp")
    write(nodes, ODD_NODES)
    for mode in MODES:
        for s in ("", "_s"):
            tool(*a, os.path.join(d, "out_%s%s.tsv" % (mode, s)), os.path.join(d, "sum_%s%s.txt" % (mode, s)), "-c", mode, "-t", nodes, *(["-s"] if s else []))
    for s in ("", "_s"):
        tool(*a, os.path.join(d, "out_lowest_notree%s.tsv" % s), os.path.join(d, "sum_lowest_notree%s.txt" % s), "-c", "lowest", *(["-s"] if s else []))


def stop_cases():
    good = [(b"C\tr%d\t4\t10" % k, b"C\tr%d\t5\t10" % k) for k in range(5)]
    g1 = lambda: [p[0] for p in good]
    g2 = lambda: [p[1] for p in good]

    def with_bad(side, line):
        L = [g1(), g2()]
        L[side][3] = line
        return L
    cases = {
        "1_class": with_bad(0, b"X\tr3\t4\t10"), "1_lower_case": with_bad(0, b"c\tr3\t4\t10"), "1_empty": with_bad(0, b""), "1_tabs_none": with_bad(0, b"C"),
        "1_tabs_one": with_bad(0, b"C\tr3"), "1_column": with_bad(0, b"C\tr3\t"), "1_column_u": with_bad(0, b"U\tr3\t"), "1_no_score_s": with_bad(0, b"C\tr3\t4"),
        "1_score_end_s": with_bad(0, b"C\tr3\t4\t"), "2_class": with_bad(1, b"\tC\tr3\t5\t10"), "2_empty": with_bad(1, b""), "2_tabs_one": with_bad(1, b"U\tr3"),
        "2_column": with_bad(1, b"C\tr3\t"), "2_no_score_s": with_bad(1, b"C\tr3\t5"), "2_score_end_s": with_bad(1, b"C\tr3\t5\t"),
        "names": with_bad(1, b"C\tr3 \t5\t10"), "names_case": with_bad(1, b"C\tR3\t5\t10"), "both_bad": [g1()[:3] + [b"C\tr3"] + g1()[4:], g2()[:3] + [b"X"] + g2()[4:]],
        "stop_at_0": [[b""] + g1(), g2()], "stop_at_last": [g1()[:4] + [b"C\tr4"], g2()],
        "text1_longer": [g1(), g2()[:3]], "text1_longer_bad": [g1()[:3] + [b"Z"] + g1()[4:], g2()[:3]],
        "text2_longer": [g1()[:3], g2()], "text2_longer_empty": [g1()[:3], g2()[:3] + [b""]], "text2_longer_empty_more": [g1()[:3], g2()[:3] + [b"", b"x"]],
        "no_stop_no_newline": [g1(), g2()],
    }
    out = {}
    for name, (l1, l2) in cases.items():
        t1, t2 = b"\n".join(l1) + b"\n", b"\n".join(l2) + b"\n"
        if name == "no_stop_no_newline":
            t1 = t1[:-1]
        if name == "text2_longer_empty":
            assert t2.endswith(b"10\n\n")
        out[name] = (t1, t2)
    return out


def stops():
    d = os.path.join(OUT, "stops")
    os.makedirs(d, exist_ok=True)
    for name, (t1, t2) in stop_cases().items():
        a = [os.path.join(d, name + ".1.tsv"), os.path.join(d, name + ".2.tsv")]
        write(a[0], t1)
        write(a[1], t2)
        tool(*a, os.path.join(d, name + ".out.tsv"), os.path.join(d, name + ".sum.txt"), "-c", "1", *(["-s"] if name.endswith("_s") else []))


def real():
    d = os.path.join(OUT, "real")
    os.makedirs(d, exist_ok=True)
    a = [os.path.join(HERE, "ref_mem_1.tsv"), os.path.join(HERE, "ref_greedy_1.tsv")]
    for mode in MODES:
        for s in ("", "_s"):
            tool(*a, os.path.join(d, "out_%s%s.tsv" % (mode, s)), os.path.join(d, "sum_%s%s.txt" % (mode, s)), "-c", mode, "-t", os.path.join(HERE, "nodes.dmp"),
                 *(["-s"] if s else []))


if __name__ == "__main__":
    build_tool()
    odd()
    stops()
    real()
