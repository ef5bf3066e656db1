"""The host side of kaiju2table that needs no GPU: the rows (kaiju_amd/csrc/host/table_rows.h through api.table_text) given
the entries and totals of tests/table_expect.py must be the tables the unmodified tool wrote, and the command line must
refuse what the tool refuses, with its status."""
import os
import subprocess

import pytest

import table_expect as te
import table_inputs as ti
from kaiju_amd import api, build


@pytest.fixture(scope="module")
def names():
    n = {"fixture": api.TaxonNames(ti.NODES, ti.NAMES), "real": api.TaxonNames(ti.REAL_NODES, ti.REAL_NAMES, "path")}   # (any mode will do)
    yield n
    for v in n.values():
        v.close()


def rows_of(names, tree, files, opt):
    out = te.HEADER
    for label, text in files:
        totals, entries = te.tally(tree, [text])
        out += api.table_text(names, ti.entries_array(entries, api.TALLY_ENTRY_DTYPE), tuple(totals[f] for f in te.INFO_FIELDS), label, **opt)
    return out


@pytest.mark.parametrize("name", sorted(ti.SETS))
def test_rows_of_the_fixture_files_are_the_tools(names, name):
    assert rows_of(names["fixture"], ti.fixture_tree(), ti.fixture_texts(), ti.SETS[name]) == ti.read(os.path.join(ti.TABLE, "out_%s.tsv" % name))


@pytest.mark.parametrize("name", sorted(ti.SETS))
def test_rows_of_the_golden_reads_are_the_tools(names, name):
    assert rows_of(names["real"], ti.real_tree(), ti.real_texts(), ti.SETS[name]) == ti.read(os.path.join(ti.TABLE, "real", "out_%s.tsv" % name))


def test_rows_do_not_depend_on_the_order_of_the_entries(names):
    tree = ti.fixture_tree()
    totals, entries = te.tally(tree, [ti.fixture_texts()[0][1]])
    tot = tuple(totals[f] for f in te.INFO_FIELDS)
    for opt in ti.SETS.values():
        a = api.table_text(names["fixture"], ti.entries_array(entries, api.TALLY_ENTRY_DTYPE), tot, "f", **opt)
        b = api.table_text(names["fixture"], ti.entries_array(entries[::-1], api.TALLY_ENTRY_DTYPE), tot, "f", **opt)
        assert a == b == te.table_rows(tree, entries, totals, opt, "f")


REFUSED = {
    "no rank": [],
    "bad rank": ["-r", "strain"],
    "-p with -l": ["-r", "genus", "-p", "-l", "genus,species"],
    "-m with -c": ["-r", "genus", "-m", "5", "-c", "2"],
    "rank not in -l": ["-r", "genus", "-l", "superkingdom,species"],
    "-m outside [0, 100]": ["-r", "genus", "-m", "101"],
    "-c below 0": ["-r", "genus", "-c", "-1"],
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_the_command_line_refuses_what_the_tool_refuses(tmp_path, why):
    build.build_table_cli()
    out = tmp_path / "out.tsv"
    r = subprocess.run([build.TABLE_CLI, "-t", ti.NODES, "-n", ti.NAMES, "-o", str(out)] + REFUSED[why] + [os.path.join(ti.TABLE, "allu.tsv")],
                       capture_output=True, timeout=60)
    assert r.returncode == 1 and r.stderr.startswith(b"Error: ") and b"usage:" in r.stderr and r.stdout == b""
    assert not out.exists()


def test_the_model_and_the_library_refuse_the_same_options(names):
    tot = (0,) * len(te.INFO_FIELDS)
    empty = ti.entries_array([], api.TALLY_ENTRY_DTYPE)
    for opt in (dict(rank=""), dict(rank="strain"), dict(rank="genus", full_path=True, ranks="genus"), dict(rank="genus", min_percent=5.0, min_count=2),
                dict(rank="genus", ranks="species,,phylum"), dict(rank="genus", min_percent=100.5), dict(rank="genus", min_count=-1)):
        assert te.refusal(opt) is not None
        with pytest.raises(api.KaijuGpuError):
            api.table_text(names["fixture"], empty, tot, "f", **opt)
    for opt in ti.SETS.values():
        assert te.refusal(opt) is None
