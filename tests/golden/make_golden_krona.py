"""Golden files of the Krona text:  python tests/golden/make_golden_krona.py

The unmodified reference tool is compiled by the pattern rules of oracle/Makefile (its object, util.o and those of bwt/) and
linked into oracle/_ref/kaiju2krona (git-ignored), exactly as tests/golden/make_golden_table.py builds its tool.  Only data is
written, under tests/golden/krona/:

  nodes.dmp, names.dmp   the tree of tests/golden/table/ and a name for 499, the parent of genus 500 that is no node
  out_<file>_<set>.txt   the tool on ../table/odd/in.tsv, ../table/empty.tsv and ../table/allu.tsv for every option set of SETS
  real/out_<set>.txt     the same on ../../ref_mem_1.tsv (the reference's kaiju -v on the committed reads) over
            tests/golden/nodes.dmp and tests/golden/names/golden/names.dmp

The order of the tool's lines is that of its unordered_map: the tests compare sorted lines."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
TOOL = os.path.join(REF, "kaiju2krona")
OUT = os.path.join(HERE, "krona")
BWT = ["_ref/obj/bwt/%s.o" % f for f in ("bwt", "compactfmi", "sequence", "suffixArray")]

# name of the set -> the options behind -t / -n / -i / -o
SETS = {
    "none": [],
    "u": ["-u"],
    "l4": ["-l", "superkingdom,phylum,genus,species"],
    "lnorank": ["-l", "superkingdom,genus,,no rank"],
    "tribe": ["-l", "tribe"],
}
FILES = {"odd": "../table/odd/in.tsv", "empty": "../table/empty.tsv", "allu": "../table/allu.tsv"}
REAL_FILE = "../../ref_mem_1.tsv"
REAL_TREE = ["../../nodes.dmp", "../../names/golden/names.dmp"]
DANGLING = b"499\t|\tDangling parent\t|\t\t|\tscientific name\t|\n"


def build_tool():
    objs = ["_ref/obj/kaiju2krona.o", "_ref/obj/util.o"] + BWT
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")] + objs, check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["g++", "-o", TOOL] + [os.path.join(ROOT, "oracle", o) for o in objs] + ["-lpthread", "-lz"], check=True)


def run(cwd, tree, file, out, args):
    subprocess.run([TOOL, "-t", tree[0], "-n", tree[1], "-i", file, "-o", out] + args, check=True, cwd=cwd, stderr=subprocess.DEVNULL)
    print(os.path.join(cwd, out), os.path.getsize(os.path.join(cwd, out)))


if __name__ == "__main__":
    build_tool()
    os.makedirs(os.path.join(OUT, "real"), exist_ok=True)
    shutil.copyfile(os.path.join(HERE, "table", "nodes.dmp"), os.path.join(OUT, "nodes.dmp"))
    with open(os.path.join(HERE, "table", "names.dmp"), "rb") as f:
        names = f.read()
    with open(os.path.join(OUT, "names.dmp"), "wb") as f:
        f.write(names + DANGLING)
    for name, args in SETS.items():
        for label, file in FILES.items():
            run(OUT, ["nodes.dmp", "names.dmp"], file, "out_%s_%s.txt" % (label, name), args)
        run(os.path.join(OUT, "real"), REAL_TREE, REAL_FILE, "out_%s.txt" % name, args)
