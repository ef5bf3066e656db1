"""What the tests of the tally and of the table share: the fixtures under tests/golden/table/, the option sets the goldens were
written with (those of tests/golden/make_golden_table.py), small trees and texts."""
import os

import numpy as np

import table_expect as te

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLE = os.path.join(GOLDEN, "table")
FILES = ["odd/in.tsv", "empty.tsv", "allu.tsv"]
REAL_FILES = ["../../ref_mem_1.tsv", "../../ref_greedy_1.tsv"]
NODES, NAMES = os.path.join(TABLE, "nodes.dmp"), os.path.join(TABLE, "names.dmp")
REAL_NODES, REAL_NAMES = os.path.join(GOLDEN, "nodes.dmp"), os.path.join(GOLDEN, "names", "golden", "names.dmp")

SETS = {
    "species": dict(rank="species"),
    "species_u": dict(rank="species", filter_unclassified=True),
    "genus_e": dict(rank="genus", expand_viruses=True),
    "species_c3": dict(rank="species", min_count=3),
    "species_m10": dict(rank="species", min_percent=10.0),
    "species_p": dict(rank="species", full_path=True),
    "genus_l": dict(rank="genus", ranks="superkingdom,genus,,phylum"),
    "species_eup": dict(rank="species", expand_viruses=True, filter_unclassified=True, full_path=True),
}


def argv_of(opt):
    """the options of a set as the command line takes them"""
    a = ["-r", opt["rank"]]
    if opt.get("ranks"):
        a += ["-l", opt["ranks"]]
    if opt.get("min_count"):
        a += ["-c", str(opt["min_count"])]
    if opt.get("min_percent"):
        a += ["-m", "%g" % opt["min_percent"]]
    for key, flag in (("expand_viruses", "-e"), ("filter_unclassified", "-u"), ("full_path", "-p")):
        if opt.get(key):
            a.append(flag)
    return a


def read(path):
    with open(path, "rb") as f:
        return f.read()


_trees = {}


def fixture_tree():
    if "fixture" not in _trees:
        _trees["fixture"] = te.Tree(read(NODES), read(NAMES))
    return _trees["fixture"]


def real_tree():
    if "real" not in _trees:
        _trees["real"] = te.Tree(read(REAL_NODES), read(REAL_NAMES))
    return _trees["real"]


def fixture_texts():
    """(label, text) of the three fixture files"""
    return [(f, read(os.path.join(TABLE, f))) for f in FILES]


def real_texts():
    return [(f, read(os.path.join(TABLE, "real", f))) for f in REAL_FILES]


def line_of(tid, k=0, kind=b"C"):
    return kind + b"\tr%d\t%d\n" % (k, tid)


def random_text(rng, tree, n_lines, final_newline=True):
    """lines over the nodes of the tree, skewed: half of them one taxon; odd lines in between"""
    ids = sorted(tree.nodes)
    odd = [b"U\tu\t0", b"", b"C\tx\t", b"C\tx\t 7", b"C\tx\t99999", b"C", b"c\tx\t25", b"C\tx\t0025\r", b"C\tv\t25\t12\t25,\tacc,\tPEP,", b"C\t" + b"n" * 300 + b"\t29"]
    lines = []
    for k in range(n_lines):
        u = rng.random()
        if u < 0.5:
            lines.append(b"C\tr%d\t%d" % (k, ids[len(ids) // 2]))
        elif u < 0.85:
            lines.append(b"C\tr%d\t%d" % (k, ids[int(rng.integers(len(ids)))]))
        else:
            lines.append(odd[int(rng.integers(len(odd)))])
    text = b"\n".join(lines)
    return text + b"\n" if final_newline and lines else text


def many_taxa_tree(n):
    """a root with n species below n genera: (nodes.dmp, names.dmp) bytes; the species are 1000 .. 1000 + n - 1"""
    nodes = [b"1\t|\t1\t|\tno rank\t|\n"]
    names = [b"1\t|\troot\t|\t\t|\tscientific name\t|\n"]
    for k in range(n):
        nodes.append(b"%d\t|\t1\t|\tgenus\t|\n" % (100000 + k))
        nodes.append(b"%d\t|\t%d\t|\tspecies\t|\n" % (1000 + k, 100000 + k))
        names.append(b"%d\t|\tSpecies %d\t|\t\t|\tscientific name\t|\n" % (1000 + k, k))
    return b"".join(nodes), b"".join(names)


TABLE_SLOTS, COUNT_SHARE = 2048, 32768     # kj_tally.h: slots of a block's table, bytes of text a block sweeps at least
WIDE_TAXA = 4000                           # species of the wide tree: more than a block's table holds


def table_shapes():
    """texts over many_taxa_tree(WIDE_TAXA) for the table of a block of the count pass: name -> text"""
    short = lambda tid: b"C\t\t%d\n" % tid
    S = {
        # one block (less than COUNT_SHARE bytes) meets more taxa than its table has slots
        "one_block_3600_taxa": b"".join(short(1000 + k) for k in range(3600)),
        # ... twice each, the second time behind all the others: what the table holds and what it does not, both again
        "one_block_1800_taxa_twice": b"".join(short(1000 + k % 1800) for k in range(3600)),
        # four blocks, every one of them sweeps every taxon
        "four_blocks_every_taxon": b"".join(short(1000 + (k * 7) % WIDE_TAXA) for k in range(4 * 3640 - 700)),
        "fits_the_table": b"".join(short(1000 + k % 40) for k in range(3000)),
    }
    assert len(S["one_block_3600_taxa"]) < COUNT_SHARE and 3 * COUNT_SHARE < len(S["four_blocks_every_taxon"]) < 4 * COUNT_SHARE
    return S


def entries_array(entries, dtype):
    a = np.zeros(len(entries), dtype=dtype)
    for k, (t, d, s, v) in enumerate(entries):
        a[k]["taxon"], a[k]["direct"], a[k]["summed"], a[k]["virus"] = t, d, s, v
    return a
