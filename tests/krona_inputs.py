"""What the tests of the Krona text share: the fixtures under tests/golden/krona/ (made by tests/golden/make_golden_krona.py),
the option sets the goldens were written with, small trees."""
import os

import table_expect as te
import table_inputs as ti

KRONA = os.path.join(ti.GOLDEN, "krona")
NODES, NAMES = os.path.join(KRONA, "nodes.dmp"), os.path.join(KRONA, "names.dmp")
FILES = {"odd": os.path.join(ti.TABLE, "odd", "in.tsv"), "empty": os.path.join(ti.TABLE, "empty.tsv"), "allu": os.path.join(ti.TABLE, "allu.tsv")}
REAL_FILE = os.path.join(ti.GOLDEN, "ref_mem_1.tsv")

# name of the set -> (unclassified, ranks)
SETS = {
    "none": (False, None),
    "u": (True, None),
    "l4": (False, "superkingdom,phylum,genus,species"),
    "lnorank": (False, "superkingdom,genus,,no rank"),
    "tribe": (False, "tribe"),
}


def argv_of(name):
    u, ranks = SETS[name]
    return (["-u"] if u else []) + (["-l", ranks] if ranks is not None else [])


_trees = {}


def fixture_tree():
    if "fixture" not in _trees:
        _trees["fixture"] = te.Tree(ti.read(NODES), ti.read(NAMES))
    return _trees["fixture"]


def golden(label, name):
    """the tool's file for a fixture file ("odd", "empty", "allu") or for the golden reads ("real")"""
    return ti.read(os.path.join(KRONA, "real", "out_%s.txt" % name) if label == "real" else os.path.join(KRONA, "out_%s_%s.txt" % (label, name)))


def cases():
    """(label, tree, text) of the three fixture files and of the golden reads"""
    return [(label, fixture_tree(), ti.read(path)) for label, path in FILES.items()] + [("real", ti.real_tree(), ti.read(REAL_FILE))]


def chain_tree(depth, long_every=3, long_bytes=200):
    """a root and a chain of `depth` nodes below it, names of 1 byte and - every long_every-th - of about long_bytes bytes, one
    node in the middle without a name: (nodes.dmp, names.dmp) bytes; the nodes are 2 .. depth + 1"""
    nodes = [b"1\t|\t1\t|\tno rank\t|\n"]
    names = [b"1\t|\troot\t|\t\t|\tscientific name\t|\n"]
    for k in range(depth):
        tid = 2 + k
        nodes.append(b"%d\t|\t%d\t|\t%s\t|\n" % (tid, tid - 1, (b"genus", b"species", b"no rank")[k % 3]))
        if k == depth // 2:
            continue
        name = (b"L%d-" % tid + b"x" * long_bytes)[:long_bytes + k % 7] if k % long_every == 0 else b"abcdefghijklmnopqrstuvwxyz"[k % 26:k % 26 + 1]
        names.append(b"%d\t|\t%s\t|\t\t|\tscientific name\t|\n" % (tid, name))
    return b"".join(nodes), b"".join(names)
