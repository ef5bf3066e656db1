"""tests/annotate_expect.py against the reference tool's own outputs: tests/golden/names/deep/ (the tool's input and its four
outputs), tests/golden/annotate/odd/ (every kind of line its reading loop tells apart) and tests/golden/annotate/verbose/ (the
reference's kaiju -v piped through the tool), all made with the unmodified kaiju-addTaxonNames: byte for byte, every file."""
import pytest

import annotate_expect
import annotate_inputs as ai


@pytest.mark.parametrize("fixture", ["deep", "odd"])
@pytest.mark.parametrize("out,mode,drop", ai.FOUR_MODES)
def test_deep_and_odd(fixture, out, mode, drop):
    got = annotate_expect.expected(ai.deep_names(mode), ai.fixture_input(fixture), drop)
    assert got["text"] == ai.fixture_output(fixture, out) and got["written"] == got["text"] and got["info"]["overflow"] == 0


@pytest.mark.parametrize("kind", ["name", "path"])
@pytest.mark.parametrize("run", ["mem", "greedy"])
def test_verbose(run, kind):
    text = ai.verbose_input(run)
    got = annotate_expect.expected(ai.golden_names(kind), text)
    assert got["text"] == ai.verbose_output(run, kind)
    assert got["info"]["n_annotated"] > 100 and got["info"]["n_unnamed_taxon"] > 0 and got["info"]["n_c_lines"] < got["info"]["n_lines"]
    assert any(l.count(b"\t") == 7 for l in got["text"].split(b"\n"))      # seven columns of -v and the eighth


def test_odd_fixture_holds_what_it_is_for():
    inp = ai.fixture_input("odd")
    e = annotate_expect.expected(ai.deep_names("path"), inp)
    i = e["info"]
    assert not inp.endswith(b"\n") and e["text"].endswith(b"Orphan genus; Orphan species; \n")
    assert i["n_empty"] == 2 and i["n_bad_id"] >= 9 and i["n_unknown_taxon"] >= 3 and i["n_unnamed_taxon"] >= 2 and i["n_dropped"] == 0
    assert i["n_lines"] == len(annotate_expect.split_lines(inp)) and max(len(l) for l in annotate_expect.split_lines(inp)) == 5000
    assert b"\0" in inp and b"\r" in inp and b"\nCC\tr16\t1\t\n" in e["text"] and b"\t007\tS; \n" in e["text"]
    name = annotate_expect.expected(ai.deep_names("name"), inp)["text"]
    assert b"\nCC\tr16\t1\troot\n" in name and b"\nC\t\t7\tS\n" in name and b"\nC\tr14\t" + b"0" * 30 + b"7\tS\n" in name
    assert b"\nC\tr6\t7\r\tS\n" in name and b"\nC\tr15\t18446744073709551615\nC\tr16\t18446744073709551616\n" in name
    u = annotate_expect.expected(ai.deep_names("path"), inp, True)
    assert u["info"]["n_dropped"] > 5 and b"\nC\tonly\n" in u["text"] and b"\nX\t" not in u["text"]
