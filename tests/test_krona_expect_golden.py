"""tests/krona_expect.py against the files the unmodified kaiju2krona wrote (tests/golden/krona/, made by
tests/golden/make_golden_krona.py): every option set and file, as sorted lines - the tool's order is that of a hash map.  The
model is what every other test of the Krona text compares with."""
import pytest

import krona_expect as ke
import krona_inputs as ki


@pytest.mark.parametrize("name", sorted(ki.SETS))
def test_model_writes_the_tools_lines(name):
    u, ranks = ki.SETS[name]
    for label, tree, text in ki.cases():
        got = ke.text_of(tree, [text], unclassified=u, ranks=ranks)
        assert ke.sorted_lines(got) == ke.sorted_lines(ki.golden(label, name)), (label, name)


def test_the_fixture_shows_what_it_is_meant_to_show():
    """the lines the tool gave on a tree of this shape"""
    none = ki.golden("odd", "none")
    # genus 24 below the unnamed family 23 prints its ancestors alone, the same bytes as order 22 itself; both are written
    assert none.count(b"2\troot\tName 2\tName 20\tName 21\tName 22\n") == 2
    # a parent that is no node but has a name is printed, and the walk ends behind it
    assert b"2\tDangling parent\tOrphan genus\tOrphan species\n" in none and b"2\troot\n" in none
    # 10243 and 23 have no name: no line
    assert b"taxonid" not in none and len(ke.sorted_lines(none)) == 17
    assert ki.golden("allu", "u") == b"7\tUnclassified\n" and ki.golden("empty", "u") == b"" and ki.golden("allu", "none") == b""
    assert ki.golden("odd", "u").endswith(b"\tUnclassified\n")
    # "no rank" is a rank like any other; a dangling parent is never printed with a list
    lnr = ki.golden("odd", "lnorank")
    assert b"1\troot\tName 2\ta clade\n" in lnr and b"Dangling" not in lnr and b"Dangling" not in ki.golden("odd", "l4")
    # a list that no node satisfies: the counts alone
    assert set(ke.sorted_lines(ki.golden("odd", "tribe"))) <= {b"%d" % k for k in range(1, 10)}


def test_the_models_order_is_that_of_the_loaders_table():
    tree = ki.fixture_tree()
    where = ke.slots_of(tree)
    assert len(set(where.values())) == len(tree.nodes) and max(where.values()) < 64
