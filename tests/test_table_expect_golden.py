"""tests/table_expect.py against the files the unmodified kaiju2table wrote (tests/golden/table/, made by
tests/golden/make_golden_table.py): every option set, byte for byte.  The model is what every other test of the tally and of
the table compares with."""
import os

import pytest

import table_expect as te
import table_inputs as ti


@pytest.mark.parametrize("name", sorted(ti.SETS))
def test_model_writes_the_tools_table_of_the_fixture_files(name):
    tree = ti.fixture_tree()
    got = te.table_of_files(tree, [(f, ti.read(os.path.join(ti.TABLE, f))) for f in ti.FILES], ti.SETS[name])
    assert got == ti.read(os.path.join(ti.TABLE, "out_%s.tsv" % name))


@pytest.mark.parametrize("name", sorted(ti.SETS))
def test_model_writes_the_tools_table_of_the_golden_reads(name):
    tree = ti.real_tree()
    got = te.table_of_files(tree, [(f, ti.read(os.path.join(ti.TABLE, "real", f))) for f in ti.REAL_FILES], ti.SETS[name])
    assert got == ti.read(os.path.join(ti.TABLE, "real", "out_%s.tsv" % name))


def test_the_fixture_shows_what_it_is_meant_to_show():
    """the rows the tool gave on a tree of this shape: -nan for the empty file, taxonid:N, paths with ';', NA fills"""
    species = ti.read(os.path.join(ti.TABLE, "out_species_c3.tsv"))
    assert b"empty.tsv\t-nan\t0\tNA\tbelong to" in species
    assert b"\ttaxonid:10243\n" in ti.read(os.path.join(ti.TABLE, "out_genus_e.tsv")) or b"taxonid:10243" in ti.read(os.path.join(ti.TABLE, "out_species_eup.tsv"))
    assert b"\tName 2;Name 20;Name 21;Name 22;taxonid:23;Genus A;Species A1;\n" in ti.read(os.path.join(ti.TABLE, "out_species_p.tsv"))
    assert b"\tNA;Orphan genus;NA;\n" in ti.read(os.path.join(ti.TABLE, "out_genus_l.tsv"))
    # the species under a species counts twice at the rank, and the remainder stays positive
    totals, entries = te.tally(ti.fixture_tree(), [ti.read(os.path.join(ti.TABLE, "odd/in.tsv"))])
    by = {e[0]: e for e in entries}
    assert by[26][2] > 0 and by[25][2] >= by[25][1] + by[26][2]
    assert totals["n_bad_id"] and totals["n_unknown_taxon"] and totals["n_virus"] and 1 not in by
