"""tests/names_expect.py against the reference tool's own outputs (tests/golden/names/, made by tests/golden/make_golden_names.py
with the unmodified kaiju-addTaxonNames): byte for byte, every file."""
import os

import pytest

import names_expect
import names_inputs
import util

NAMES = os.path.join(util.ROOT, "tests", "golden", "names")
RANKS_DEEP, RANKS_GOLDEN = "ranks:genus,species,phylum,genus", "ranks:family,genus,species"
DEEP = [("out_name.tsv", "name", False), ("out_path.tsv", "path", False), ("out_ranks.tsv", RANKS_DEEP, False), ("out_path_u.tsv", "path", True)]
GOLDEN_MODES = {"name": "name", "path": "path", "ranks": RANKS_GOLDEN}


def read(*parts):
    return names_inputs.read(os.path.join(NAMES, *parts))


def deep_names(mode):
    return names_expect.Names(read("deep", "nodes.dmp"), read("deep", "names.dmp"), mode)


def golden_names(mode):
    with open(os.path.join(util.ROOT, "tests", "golden", "nodes.dmp"), "rb") as f:
        return names_expect.Names(f.read(), read("golden", "names.dmp"), mode)


def three_columns(text):
    """the input of the tool from one of its outputs: the first three columns of every line"""
    return b"".join(b"\t".join(l.split(b"\t")[:3]) + b"\n" for l in text.split(b"\n") if l)


@pytest.mark.parametrize("out,mode,drop", DEEP)
def test_deep(out, mode, drop):
    assert deep_names(mode).text(read("deep", "in.tsv"), drop) == read("deep", out)


def test_deep_fixture_holds_what_it_is_for():
    """every quirk the fixture was built for is in the files, seen through the reference's outputs alone"""
    nodes, names, inp = read("deep", "nodes.dmp"), read("deep", "names.dmp"), read("deep", "in.tsv")
    N = deep_names("path")
    assert 4000 not in N.nodes and N.nodes[4001][1] == b"embl" and N.nodes[1002][0] == 1001 and 77 in N.nodes and 76 not in N.nodes
    assert N.names[1003] == b"Outer" and N.names[1004].startswith(b"fake scientific name") and N.names[1005] == b"First of two"
    assert len(N.names[1000]) == 1 and len(N.names[1002]) == 300 and any(b > 127 for b in N.names[1001]) and 1006 not in N.names and 12 not in N.names
    assert len(N.emitted(1039)) > 40
    by_read = {l.split(b"\t")[1]: l for l in read("deep", "out_path.tsv").split(b"\n") if l}
    line = lambda taxon: next(l for l in by_read.values() if l.split(b"\t")[2] == b"%d" % taxon)
    assert line(1).endswith(b"\t1\t")                                       # the root: a tab and nothing
    assert line(12).endswith(b"\t12") and line(777777).endswith(b"\t777777") and line(4000).endswith(b"\t4000")       # unchanged
    assert b"taxonid:99999; " in line(999999) and b"taxonid:1006; " in line(1039) and b"taxonid:4294967296; " in line(2 ** 63)
    assert line(78).endswith(b"\tOrphan genus; Orphan species; ")
    assert b"\n\n" in inp and b"\nU\t" in inp and b"\n\n" not in read("deep", "out_name.tsv")
    assert read("deep", "out_path_u.tsv").count(b"\nU\t") == 0
    ranks = {l.split(b"\t")[2]: l.split(b"\t")[3] for l in read("deep", "out_ranks.tsv").split(b"\n") if l.count(b"\t") == 3}
    first, second, third, fourth = ranks[b"1039"].split(b"; ")[:4]
    assert first == fourth == b"Lineage 100" and second == b"Lineage 999" and third == b"Lineage 9"        # the node nearest the root wins
    assert ranks[b"1"] == b"NA; NA; NA; NA; "


@pytest.mark.parametrize("kind", ["name", "path", "ranks"])
@pytest.mark.parametrize("run", ["mem", "mem_pe", "greedy", "greedy_pe"])
def test_golden(run, kind):
    want = read("golden", "%s.%s.tsv" % (run, kind))
    N = golden_names(GOLDEN_MODES[kind])
    assert N.text(three_columns(want)) == want
    assert b"\t100005\n" in want and (kind != "path" or b"taxonid:1003; " in want)      # the two gaps show
