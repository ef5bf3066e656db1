"""tests/refseq_expect.py against the files the unmodified kaiju-convertRefSeq wrote (tests/golden/make_golden_refseq.py): the
model the emulation and the GPU tests compare with is pinned on the tool, byte for byte."""
import pytest

import convert_expect as ce
import refseq_expect as re_


@pytest.fixture(scope="module")
def fx():
    return re_.Fixture()


@pytest.mark.parametrize("name", sorted(re_.SETS))
def test_the_model_writes_the_tools_file(fx, name):
    assert re_.file_of(fx.expected(name)["text"]) == re_.golden("out_%s.txt" % name)


def test_a_file_of_which_nothing_is_kept_is_one_line_end(fx):
    got = fx.expected("default", text=fx.faa_none)
    assert got["text"] == b"" and re_.file_of(got["text"]) == re_.golden("none_default.txt") == b"\n"
    assert got["info"]["n_records"] == 3 and got["info"]["n_kept"] == 0 and got["info"]["n_entries"] == 2 and got["info"]["n_hits"] == 2


def test_what_the_fixtures_pin_about_the_map(fx):
    m = fx.model
    want = {b"WP_1.1": 562, b"WP_": 564, b"WP": 562, b"WP_5.": 562, b"WP_6.1": 1236, b"WP_8.1": 10240, b"WP_9.1": 561, b"WP_B1.1": 2157, b"WP_B8.1": 564,
            b"WP_B5.1": 2, b"WP_12": 562, b"WP_34": 562, b"WP_K 1": 1423, b"WP_H.1": 9606, b"WP_R.1": 28384, b"WP_R1": 1, b"WP_\x011.1": 10240, b"WP_B2.1": 562,
            b"WP_LAST.1": 1386}
    assert m.map == want
    for key in (b"NP_1.1", b"XP_1.1", b"wp_1.1", b"W", b"WP_notab", b"WP_5.1", b"WP_7.1", b"WP_4C", b"WP_4C.1", b"WP_123", b"WP_345", b"accession.version"):
        assert m.lookup(key) == re_.MISS, key
    # 34 non-empty lines behind the header line; the duplicates: WP_1.1 again, WP_123 -> "WP_12", WP_34
    assert m.lines == 34 and m.duplicates == 3 and m.no_insert == 34 - 3 - len(want)
    assert fx.merged == {666: 562, 777: 4242} and fx.listed == [561, 1386, 2759]


def test_the_rules_differ_from_those_of_convert_nr(fx):
    """the same lines under the rules of kaiju-convertNR: a line without a tab is a key there, the taxon is column 2, nothing is truncated"""
    nr = ce.Model(fx.nodes, fx.merged).add_text(re_.golden("map.tsv"))
    assert nr.lookup(b"WP_4C.1") == 562 and fx.model.lookup(b"WP_4C.1") == re_.MISS
    assert nr.lookup(b"WP_5.1") == re_.MISS and nr.lookup(b"WP_5.") == re_.MISS and fx.model.lookup(b"WP_5.") == 562
    text = b">ZZ.1 unknown\x01WP_1.1 known\nFFFF\n>WP_1.1 x\nAAAA\n"
    assert re_.convert(fx.nodes, re_.DEFAULT_INCLUDE, fx.model.map, text)["text"] == b">562\nAAAA\n"
    assert ce.convert(fx.nodes, re_.DEFAULT_INCLUDE, fx.model.map, set(), text)["text"] == b">562\nFFFF\n>562\nAAAA\n"


def test_the_counts_of_the_fixture(fx):
    info = fx.expected("al")["info"]
    headers = [l for l in ce.getlines(fx.faa) if l[:1] == b">"]
    assert info["n_records"] == len(headers) == 35 and info["n_entries"] == sum(1 for l in headers if b" " in l) == 34
    assert info["dropped_excluded"] == 0 and info["dropped_no_lca"] == 0
    assert sum(info[k] for k in ("n_kept", "dropped_no_taxon", "dropped_not_included")) == info["n_records"]
    assert info["n_hits"] == info["n_kept"] + info["dropped_not_included"]
