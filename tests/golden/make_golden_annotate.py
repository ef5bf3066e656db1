"""Golden files of the stand-alone annotator:  python tests/golden/make_golden_annotate.py

The unmodified reference tool is built as tests/golden/make_golden_names.py builds it (oracle/_ref/kaiju-addTaxonNames,
git-ignored).  Only data is written, under tests/golden/annotate/:

  odd/      in.tsv: every kind of line the tool's reading loop tells apart (first byte, tabs, the digit run and what follows it,
            values at and beyond 2^64 - 1, ids that are no node or have no name, '\\r' and NUL bytes, a line of 5000 bytes, a
            last line without newline), run against tests/golden/names/deep/; the tool's outputs, gzip'ed: out_name.tsv.gz,
            out_path.tsv.gz (-p), out_ranks.tsv.gz (-r RANKS_DEEP), out_path_u.tsv.gz (-u -p)
  verbose/  the reference's `kaiju -v` on the committed reads (tests/golden/ref_<mode>_1.tsv, already there) piped through the
            tool with tests/golden/nodes.dmp and names/golden/names.dmp: <mode>.name.tsv.gz, <mode>.path.tsv.gz (-p)"""
import os

from make_golden_names import HERE, RANKS_DEEP, build_tool, tool

OUT = os.path.join(HERE, "annotate")
DEEP = os.path.join(HERE, "names", "deep")


def odd_lines():
    L = [
        b"U\tu1\t0", b"X\tr\t7", b"CC\tr16\t1", b"Cfoo\tr4\t7abc\tz", b"C\tr5\t7 8", b"C\tr6\t7\r", b"C\tr7\t7\tx\ty", b"C\tr8\t007",
        b"C\tlast column\t1039", b"C", b"C\tonly", b"C\tr9\t", b"C\tr10\t+7", b"C\tr11\t-7", b"C\tr12\t 7", b"C\tr13\t99999999999999999999999",
        b"C\tr14\t" + b"0" * 30 + b"7", b"C\tr15\t18446744073709551615", b"C\tr16\t18446744073709551616", b"C\tr17\t18446744073709551614",
        b"C\tr18\t777777", b"C\tr19\t12", b"C\t\t7", b"", b"", b"U\t\t0", b"\tC\tr20\t7", b"c\tr21\t7", b"C\tr22\t10000000000000000000",
        # kaiju -v: seven columns; kaijux: the third column is a name
        b"C\tread_v\t1039\t312\t1039,1038,\tacc1,acc2,\tMKVLA,", b"C\tread_x\tWP_012345.1_1039", b"C\tread_x2\t1039_WP_1",
        b"C\tnul\0in name\t7\0rest", b"\0", b"C\0\tr23\t7", b"C\tr24\t9223372036854775808", b"C\tr25\t4294967296", b"C\tr26\t7\t",
        b"C\t" + b"n" * (5000 - 7) + b"\t1005",
        b"U\t" + b"u" * 40 + b"\t0", b"C\tr27\t1002", b"C\tr28\t1", b"\r", b"C\r\tr29\t7",
        b"C\tno newline at the end\t78",
    ]
    assert len(L[38]) == 5000 and L[38].startswith(b"C\tnnn")
    return L


def odd():
    d = os.path.join(OUT, "odd")
    os.makedirs(d, exist_ok=True)
    inp = os.path.join(d, "in.tsv")
    with open(inp, "wb") as f:
        f.write(b"\n".join(odd_lines()))
    a = [os.path.join(DEEP, "nodes.dmp"), os.path.join(DEEP, "names.dmp"), inp]
    tool(*a, os.path.join(d, "out_name.tsv"))
    tool(*a, os.path.join(d, "out_path.tsv"), "-p")
    tool(*a, os.path.join(d, "out_ranks.tsv"), "-r", RANKS_DEEP)
    tool(*a, os.path.join(d, "out_path_u.tsv"), "-u", "-p")


def verbose():
    d = os.path.join(OUT, "verbose")
    os.makedirs(d, exist_ok=True)
    nodes, names = os.path.join(HERE, "nodes.dmp"), os.path.join(HERE, "names", "golden", "names.dmp")
    for mode in ("mem", "greedy"):
        inp = os.path.join(HERE, "ref_%s_1.tsv" % mode)       # `kaiju -v -z 1` of the reference (make_golden.py)
        tool(nodes, names, inp, os.path.join(d, "%s.name.tsv" % mode))
        tool(nodes, names, inp, os.path.join(d, "%s.path.tsv" % mode), "-p")


if __name__ == "__main__":
    build_tool()
    odd()
    verbose()
