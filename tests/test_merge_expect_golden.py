"""tests/merge_expect.py against the reference tool's own outputs under tests/golden/merge/ (odd/: every kind of pair its loop
tells apart; stops/: every reason it breaks for; real/: the reference's kaiju -v in MEM and Greedy mode on the committed reads),
all made with the unmodified kaiju-mergeOutputs: byte for byte, every file and every summary of -v.  And the model's decimal
comparison of scores against the comparison of the doubles the tool makes."""
import random

import pytest

import merge_expect as me
import merge_inputs as mi


@pytest.mark.parametrize("mode,use_score", mi.VARIANTS)
def test_odd(mode, use_score):
    nodes, t1, t2 = mi.odd()
    got = me.expected(me.parse_nodes(nodes), t1, t2, mode, use_score)
    text, summary = mi.odd_output(mode, use_score)
    assert got["text"] == text and me.summary(got["info"]) == summary
    assert got["info"]["stop_pair"] == me.NO_PAIR and got["info"]["count"] == 94 and got["written"] == got["text"]


@pytest.mark.parametrize("use_score", [False, True])
def test_odd_lowest_without_a_tree(use_score):
    _, t1, t2 = mi.odd()
    got = me.expected({}, t1, t2, "lowest", use_score)
    text, summary = mi.odd_output("lowest", use_score, tree=False)
    assert got["text"] == text and me.summary(got["info"]) == summary
    assert text == mi.odd_output("1", use_score)[0]                    # always id1


def test_odd_fixture_holds_what_it_is_for():
    nodes, t1, t2 = mi.odd()
    parent = me.parse_nodes(nodes)
    assert [n for n in parent if parent[n] == n] == [1, 100] and not t1.endswith(b"\n") and not t2.endswith(b"\n")
    assert b"\0" in t1 and b"\r" in t1 and max(len(l) for l in t1.split(b"\n")) > 5000
    outs = {v: me.expected(parent, t1, t2, *v)["text"] for v in mi.VARIANTS}
    assert len(set(outs.values())) == 8                                 # no two variants agree
    lca, low = outs[("lca", True)], outs[("lowest", True)]
    assert b"C\tconflict1\t3\t10\n" in lca and b"C\tconflict2\t2\t10\n" in lca            # 3,4: 3; 4,3: the ancestor's parent
    assert b"C\tconflict1\t4\t10\n" in low and b"C\tconflict2\t4\t10\n" in low
    assert b"C\tconflict3\t3\t10\n" in lca and b"C\tconflict3\t4\t10\n" in low and b"C\tconflict4\t04\t10\n" in low   # 04 and 4
    assert b"C\tconflict5\t100\t10\n" in lca and b"C\tconflict6\t1\t10\n" in lca          # two trees: the root of n2's
    assert b"C\tconflict26\t4\t10\n" in lca and b"C\tconflict27\t4\t10\n" in lca          # -1 is no node
    assert b"C\tconflict22\t\t10\n" in lca and b"C\tconflict20\tx\t10\n" in lca           # a bad number: the text of id1, also the empty one
    assert b"C\tscore6\t5\t2\n" in lca and b"C\tscore7\t4\t2\n" in lca                    # 400 digits are 0
    assert b"C\tscore0\t3\t1.20\n" in lca and b"C\tscore5\t3\t1.2.3\n" in lca and b"C\tscore4\t3\t.\n" in lca
    i = me.expected(parent, t1, t2, "lca", True)["info"]
    assert i["count_c12"] == 87 and i["count_c1_not_c2"] == 3 and i["count_c2_not_c1"] == 2 and i["count_c3"] == 94 - 2


@pytest.mark.parametrize("name", mi.stop_names())
def test_stops(name):
    t1, t2, use_score, text, summary = mi.stop_case(name)
    got = me.expected({}, t1, t2, "1", use_score)
    assert got["text"] == text and me.summary(got["info"]) == summary


def test_stop_reasons():
    why = {n: me.expected({}, *mi.stop_case(n)[:2], "1", mi.stop_case(n)[2])["info"] for n in mi.stop_names()}
    assert len(why) == 26 and {i["stop_why"] for i in why.values()} == set(range(9))       # every reason but SCORE_WIDE, and none
    assert why["both_bad"]["stop_why"] == me.STOP["1_tabs"] and why["text1_longer_bad"]["stop_why"] == me.STOP["1_class"]
    assert why["text1_longer"]["stop_why"] == me.STOP["2_short"] and why["text1_longer"]["stop_pair"] == 3 and why["text1_longer"]["count"] == 4
    assert why["text2_longer"]["more_in_2"] == 1 and why["text2_longer_empty"]["more_in_2"] == 0 and why["text2_longer"]["stop_pair"] == me.NO_PAIR
    assert why["stop_at_0"]["count"] == 1 and why["stop_at_0"]["text_bytes"] == 0 and why["stop_at_last"]["stop_pair"] == 4


@pytest.mark.parametrize("mode,use_score", mi.VARIANTS)
def test_real(mode, use_score):
    nodes, t1, t2 = mi.real()
    got = me.expected(me.parse_nodes(nodes), t1, t2, mode, use_score)
    text, summary = mi.real_output(mode, use_score)
    assert got["text"] == text and me.summary(got["info"]) == summary and got["info"]["count"] == 713
    assert 0 < got["info"]["count_c1_not_c2"] + got["info"]["count_c2_not_c1"] and got["info"]["count_c12"] > 300


def in_domain(rng):
    """a score text inside the domain: at most 15 digits from the first to the last non-zero one, in [1e-300, 1e300), with
    zeros and a point wherever they may stand; or a zero; or an invalid text"""
    k = rng.random()
    if k < 0.08:
        return rng.choice([b"", b".", b"0", b"000", b"0.0", b".000", b"0.", b"..", b".0.5"])
    digits = "".join(rng.choice("0123456789") for _ in range(rng.randrange(1, 16)))
    digits = rng.choice("123456789") + digits[1:]
    exp = rng.randrange(-300, 300) if rng.random() < 0.3 else rng.randrange(-4, 6)        # of the first digit
    if exp >= 0:
        whole = (digits + "0" * max(0, exp + 1 - len(digits)))
        text = whole[:exp + 1] + ("." + whole[exp + 1:] if len(whole) > exp + 1 or rng.random() < 0.3 else "")
    else:
        text = rng.choice(["0", "", "00"]) + "." + "0" * (-exp - 1) + digits
    text = "0" * rng.randrange(0, 3) + text
    if "." in text:
        text += "0" * rng.randrange(0, 4) + rng.choice(["", "", ".7"])
    return text.encode()


def as_double(s):
    """stod of the text, with its two ways to fail giving 0"""
    import re
    m = re.match(rb"[0-9]+\.?[0-9]*|\.[0-9]+", s)
    v = float(m.group(0)) if m else 0.0
    return 0.0 if v == float("inf") else v


def test_decimal_comparison_is_the_comparison_of_the_doubles():
    rng = random.Random(20241020)
    pairs, unequal, near = 0, 0, 0
    for _ in range(20000):
        a = in_domain(rng)
        b = in_domain(rng) if rng.random() < 0.5 else a
        if rng.random() < 0.4 and len(a) > 2:                                             # a neighbour: one digit changed
            k = rng.randrange(len(a))
            if a[k:k + 1].isdigit():
                b = a[:k] + rng.choice(b"0123456789".decode()).encode() + a[k + 1:]
                near += 1
        try:
            da, db = me.score_value(a), me.score_value(b)
        except me.ScoreWide:
            continue
        x, y = as_double(a), as_double(b)
        assert (da > db) == (x > y) and (da == db) == (x == y) and (da < db) == (x < y), (a, b)
        pairs += 1
        unequal += x != y
    assert pairs >= 10000 and unequal > 3000 and pairs - unequal > 2000 and near > 3000


def test_score_domain():
    for s in (b"9007199254740993", b"9007199254740992", b"1234567890.123456", b"1" + b"0" * 300, b"0." + b"0" * 300 + b"1", b"1" + b"0" * 308):
        with pytest.raises(me.ScoreWide):
            me.score_value(s)
    assert float(b"9007199254740993") == float(b"9007199254740992")                      # what the tool sees: equal
    for s in (b"", b".", b"0.000", b"9" * 400, b"1" + b"0" * 309):
        assert me.score_value(s) == 0
    assert me.score_value(b"1.2.3") == me.score_value(b"1.20") and me.score_value(b"007") == 7 and me.score_value(b"999999999999999" + b"0" * 285) > 0
    e = me.expected({}, b"C\tb\t4\t9007199254740993\n", b"C\tb\t5\t9007199254740992\n", "1", True)
    assert e["info"]["stop_why"] == me.STOP["score_wide"] and e["info"]["stop_pair"] == 0 and e["text"] == b""
    assert me.expected({}, b"C\tb\t4\t9007199254740993\n", b"C\tb\t5\t9007199254740992\n", "1", False)["text"] == b"C\tb\t4\n"
