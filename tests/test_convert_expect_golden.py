"""tests/convert_expect.py against the files the unmodified kaiju-convertNR wrote (tests/golden/make_golden_convert.py): the
model the emulation and the GPU tests compare with is pinned on the tool, byte for byte."""
import random

import pytest

import convert_expect as ce


@pytest.fixture(scope="module")
def fx():
    return ce.Fixture()


@pytest.mark.parametrize("name", sorted(ce.SETS))
def test_the_model_writes_the_tools_file(fx, name):
    assert ce.file_of(fx.expected(name)["text"]) == ce.golden("out_%s.txt" % name)


def test_a_file_of_which_nothing_is_kept_is_one_line_end(fx):
    got = fx.expected("default", text=fx.nr_none)
    assert got["text"] == b"" and ce.file_of(got["text"]) == ce.golden("none_default.txt") == b"\n"
    assert got["info"]["n_records"] == 3 and got["info"]["n_kept"] == 0


def test_what_the_fixtures_pin_about_the_map(fx):
    m = fx.model
    want = {b"A1.1": 562, b"A5.1": 562, b"A6.1": 1236, b"A8.1": 10240, b"A9.1": 561, b"B1.1": 2157, b"B2.1": 562, b"561": 561, b"K1": 1386, b"": 1423,
            b"V\x011.1": 10240, b"B5.1": 2, b"B8.1": 564, b"B6.1": 1, b"NP_0123456789012345678901234567890.12": 562}
    for key, taxon in want.items():
        assert m.lookup(key) == taxon, key
    for key in (b"A7.1", b"Y9", b"B7.1", b"accession.version", b"X9", b"1386"):
        assert m.lookup(key) == ce.MISS, key
    assert m.duplicates == 1 and m.no_insert == 6 and m.lines == 27
    assert fx.merged == {666: 562, 777: 4242} and fx.nodes[562] == 561 and fx.listed == [561, 1386, 2759]


def test_the_counts_of_the_fixture(fx):
    info = fx.expected("ale")["info"]
    # (counted by hand in nr.txt: the headers, those with E1.1 or A4.1 in an entry - ">A1.1 first\x01A4.1" has no such entry)
    assert info["dropped_excluded"] == 4 and info["dropped_no_lca"] == 0 and info["n_records"] == 28
    assert sum(info[k] for k in ("n_kept", "dropped_excluded", "dropped_no_taxon", "dropped_not_included", "dropped_no_lca")) == info["n_records"]


def test_the_local_entry_rule_is_the_sequential_one(fx):
    for line in ce.getlines(fx.nr):
        assert ce.entries_local(line) == ce.entries_sequential(line), line
    rng = random.Random(5)
    for _ in range(4000):
        line = b">" + bytes(rng.choice(b"\x01\x01  ab>") for _ in range(rng.randrange(0, 14)))
        assert ce.entries_local(line) == ce.entries_sequential(line), line
    for name in ce.SETS:
        assert fx.expected(name, entries=ce.entries_local) == fx.expected(name)


def test_strtoul_of_the_model():
    for text, want in ((b"562", 562), (b"  +7x", 7), (b"-1", ce.ULONG_MAX), (b"", 0), (b"abc", 0), (b"18446744073709551615", ce.ULONG_MAX),
                       (b"18446744073709551616", ce.ULONG_MAX), (b"-18446744073709551054", 562), (b"\t\r 12\t3", 12), (b"- 5", 0), (b"5\x006", 5)):
        assert ce.strtoul(text) == want, text
