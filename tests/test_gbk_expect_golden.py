"""tests/gbk_expect.py against the files the unmodified kaiju-gbk2faa.pl wrote (tests/golden/make_golden_gbk.py), and, where
perl and the reference are present, against the script itself on generated lines: the model the emulation and the GPU tests
compare with is pinned on the script, byte for byte."""
import random

import pytest

import gbk_expect as ge


def statuses():
    return dict((line.split()[0], int(line.split()[1])) for line in ge.golden("status.txt").decode().splitlines())


@pytest.mark.parametrize("name", ge.FIXTURES)
def test_the_model_writes_the_scripts_file(name):
    text = ge.golden(name + ".gbk")
    out, status = ge.convert_file(text)
    assert out == ge.golden(name + ".faa") and status == statuses()[name]
    for cuts in ([], ge.cuts_behind_lines(text)):
        got, _, bad = ge.convert_blocks(text, cuts)
        assert got == out and (bad != 0) == (status != 0)


def test_what_the_fixtures_pin():
    out = ge.golden("rules.faa")
    assert out.startswith(b">P1_0010239\nMKVDEacd\n>P2_13\nQ\n")                  # the digits as written, the filter, the leftmost match
    assert b">P2_13\nACD\nEFG\n\nHIKy\n>P3_77\nLMN\nPQR\n>P3_77\nSTV\nWYAtrailingtetacd\n" in out     # inside a translation
    assert b"CCC" not in out and b"NO" not in out and b"X\n" not in out
    for letters, white in ((b"AAV", True), (b"AAF", True), (b"AAG", False), (b"AAH", False), (b"AAT", True), (b"AAR", True), (b"AAS", True)):
        assert (b"\n" + letters + b"\n" in out) == white, letters               # 0x0b and 0x0c are white space, 0x85 and 0xa0 are not
    assert b">P3_77\nACDE\n>P\x004_77\nKK\n>P\x004_1234567890123456789012345\nGG\n>P\x004_5\nHH\n>P5_5\nII\n" in out
    assert out.endswith(b">P5_9\nLL\n>P5_9\nMM\nNN\n\n>P6_8\nSS\n")
    assert ge.golden("nopid.faa") == b">_5\nMKV\n"
    assert ge.golden("crlf.faa") == b">C1_11\nMKV\n>C1_11\nACD\nEFG\nHIK\n"
    assert ge.golden("tail_open.faa") == b">T1_5\nMKV\nACD\nEFG\n" and ge.golden("tail_closed.faa") == b">T1_5\nMKV\nACD\nEFG\n"
    assert ge.golden("notaxon.faa") == b"" == ge.golden("notaxon_late.faa") and statuses()["notaxon"] == 255 == statuses()["notaxon_late"]
    assert ge.golden("record.faa").count(b">") == 2 and ge.golden("record.faa").count(b"\n") == 6


def test_every_kind_and_state_is_in_the_fixture():
    r = ge.convert(ge.golden("rules.gbk"))
    assert all(k > 0 for k in r["kinds"]) and sum(r["kinds"]) == r["info"]["n_lines"]
    assert r["info"]["letters_dropped"] > 0 and r["info"]["n_records"] == r["text"].count(b">")
    late = ge.convert(ge.golden("notaxon_late.gbk"))
    assert late["info"]["no_taxon_line"] == 6 and late["info"]["text_bytes"] == 0 and late["state"] == ge.State()


def test_the_state_does_not_advance_on_overflow():
    text = ge.golden("rules.gbk")
    full = ge.convert(text)
    assert full["state"] != ge.State()
    short = ge.convert(text, out_cap=len(full["text"]) - 1)
    assert short["state"] == ge.State() and short["info"]["overflow"] == 1 and short["written"] == b"".join(full["lines"][:-1])


def test_generated_lines_against_the_script():
    """the cap on skipped cases is zero where perl and the reference are present"""
    if not ge.have_script():
        pytest.skip("perl or the reference's util/kaiju-gbk2faa.pl is not on this machine")
    rng = random.Random(20261020)
    texts = [ge.random_text(rng, 400, taxon_first=True) for _ in range(6)] + [ge.random_text(rng, 30, taxon_first=False) for _ in range(6)]
    texts.append(ge.genbank_text(rng, 3))
    compared = 0
    for text in texts:
        assert ge.convert_file(text) == ge.run_script(text), text[:400]
        compared += 1
    assert compared == len(texts)
    kinds = [sum(k) for k in zip(*(ge.convert(t)["kinds"] for t in texts))]
    assert all(k > 20 for k in kinds), kinds                   # the generator reaches every kind
