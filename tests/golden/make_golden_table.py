"""Golden files of the taxon table:  python tests/golden/make_golden_table.py

The unmodified reference tool is compiled by the pattern rules of oracle/Makefile (its object, util.o and those of bwt/) and
linked into oracle/_ref/kaiju2table (git-ignored), as tests/golden/make_golden_merge.py builds its tool.  Only data is
written, under tests/golden/table/:

  nodes.dmp, names.dmp   a root; a cellular branch with superkingdom .. species; 10239 with family / genus / species below
            it; a species under a species; a genus whose parent is no node; a clade without a rank; a family without a name
  odd/in.tsv             every kind of line the tool's loop tells apart, a line of more than 4096 bytes, no final newline
  empty.tsv, allu.tsv    no byte at all; nothing but 'U' lines
  out_<set>.tsv          the tool on "odd/in.tsv empty.tsv allu.tsv", run inside the directory so that the file column holds
            these names, for every option set of SETS
  real/out_<set>.tsv     the same on ../../ref_mem_1.tsv ../../ref_greedy_1.tsv (the reference's kaiju -v on the committed
            reads) over tests/golden/nodes.dmp and tests/golden/names/golden/names.dmp, run inside real/"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
TOOL = os.path.join(REF, "kaiju2table")
OUT = os.path.join(HERE, "table")
BWT = ["_ref/obj/bwt/%s.o" % f for f in ("bwt", "compactfmi", "sequence", "suffixArray")]

# name of the set -> the options behind -t / -n / -o
SETS = {
    "species": ["-r", "species"],
    "species_u": ["-r", "species", "-u"],
    "genus_e": ["-r", "genus", "-e"],
    "species_c3": ["-r", "species", "-c", "3"],
    "species_m10": ["-r", "species", "-m", "10"],
    "species_p": ["-r", "species", "-p"],
    "genus_l": ["-r", "genus", "-l", "superkingdom,genus,,phylum"],
    "species_eup": ["-r", "species", "-e", "-u", "-p"],
}
FILES = ["odd/in.tsv", "empty.tsv", "allu.tsv"]
REAL_FILES = ["../../ref_mem_1.tsv", "../../ref_greedy_1.tsv"]
REAL_TREE = ["../../nodes.dmp", "../../names/golden/names.dmp"]

# (id, parent, rank, name or None)
TREE = [
    (1, 1, "no rank", "root"), (2, 1, "superkingdom", "Name 2"), (20, 2, "phylum", "Name 20"), (21, 20, "class", "Name 21"),
    (22, 21, "order", "Name 22"), (23, 22, "family", None), (24, 23, "genus", "Genus A"), (25, 24, "species", "Species A1"),
    (26, 25, "species", "Species A1 below A1"), (27, 24, "species", "Species A2"), (28, 23, "genus", "Genus B"),
    (29, 28, "species", "Species B1"), (30, 20, "genus", "Genus C"), (31, 30, "species", "Species C1"), (40, 2, "no rank", "a clade"),
    (41, 40, "species", "Species of the clade"), (10239, 1, "superkingdom", "Viruses"), (10240, 10239, "family", "Virus family"),
    (10241, 10240, "genus", "Virus genus"), (10242, 10241, "species", "Virus species 1"), (10243, 10241, "species", None),
    (500, 499, "genus", "Orphan genus"), (501, 500, "species", "Orphan species"),
]


def build_tool():
    objs = ["_ref/obj/kaiju2table.o", "_ref/obj/util.o"] + BWT
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")] + objs, check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["g++", "-o", TOOL] + [os.path.join(ROOT, "oracle", o) for o in objs] + ["-lpthread", "-lz"], check=True)


def write(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def odd_lines():
    c = lambda name, tid, rest=b"": b"C\t" + name + b"\t" + tid + rest
    L = []
    k = 0
    for tid, n in ((25, 3), (26, 2), (27, 1), (29, 4), (31, 2), (24, 2), (20, 1), (2, 1), (1, 2), (41, 1), (40, 1), (501, 2), (500, 1), (23, 1),
                   (10239, 1), (10240, 1), (10242, 3), (10243, 1)):
        for _ in range(n):
            L.append(c(b"r%d" % k, b"%d" % tid))
            k += 1
    L += [c(b"tail", b"22abc"), c(b"zeros_cr", b"0022\r"), c(b"blank", b" 22"), c(b"plus", b"+22"), c(b"minus", b"-3"), b"C\tone_tab", b"C",
          b"c\tlower\t25", b"X", b"U\tu0\t0", b"U\tu1\t0", b"", c(b"digits23", b"12345678901234567890123"), c(b"unknown", b"999"),
          c(b"thirty_zeros", b"0" * 30 + b"25"), c(b"max64", b"18446744073709551615"), c(b"over64", b"18446744073709551616"),
          c(b"verbose", b"25", b"\t38\t25,\tWP000000287.1,\tFISLVVQSAHLKEV,"), c(b"verbose_virus", b"10242", b"\t50\t10242,10243,\tacc1,acc2,\tGLLEQ,"),
          c(b"nul\0name", b"27"), c(b"\rcr", b"29\r"), c(b"", b"31"), b"U\tverbose_u\t0", b"", b"", c(b"n" * 5000, b"29"),
          b"\tC\ttab_first\t25", c(b"orphan_parent", b"499"), c(b"no newline at the end", b"26")]
    return L


def run(cwd, tree, files, name, args):
    out = "out_%s.tsv" % name
    subprocess.run([TOOL, "-t", tree[0], "-n", tree[1], "-o", out] + args + files, check=True, cwd=cwd, stderr=subprocess.DEVNULL)
    print(os.path.join(cwd, out), os.path.getsize(os.path.join(cwd, out)))


if __name__ == "__main__":
    build_tool()
    write(os.path.join(OUT, "nodes.dmp"), b"".join(b"%d\t|\t%d\t|\t%s\t|\n" % (t, p, r.encode()) for t, p, r, _ in TREE))
    write(os.path.join(OUT, "names.dmp"), b"".join(b"%d\t|\t%s\t|\t\t|\tscientific name\t|\n" % (t, n.encode()) for t, _, _, n in TREE if n))
    write(os.path.join(OUT, "odd", "in.tsv"), b"\n".join(odd_lines()))
    write(os.path.join(OUT, "empty.tsv"), b"")
    write(os.path.join(OUT, "allu.tsv"), b"".join(b"U\tread%d\t0\n" % k for k in range(7)))
    os.makedirs(os.path.join(OUT, "real"), exist_ok=True)
    for name, args in SETS.items():
        run(OUT, ["nodes.dmp", "names.dmp"], FILES, name, args)
        run(os.path.join(OUT, "real"), REAL_TREE, REAL_FILES, name, args)
