"""Inputs of the merger's tests (tests/test_merge_emu.py on the host, tests/test_gpu_merge.py on the device): the fixtures of
tests/golden/merge/ (tests/golden/make_golden_merge.py) and the smallest texts at which a pass of kaiju_amd/csrc/merge.hip can
go wrong.  A case is (what, nodes.dmp bytes or None, text 1, text 2, mode, use_score, final); expectations come from
tests/merge_expect.py."""
import glob
import gzip
import os

import merge_expect

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MERGE = os.path.join(GOLDEN, "merge")
TILE, CHUNK = 4096, 16
VARIANTS = [(m, s) for m in merge_expect.MODES for s in (False, True)]


def read(path):
    with open(path, "rb") as f:
        return f.read()


def gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def suffix(mode, use_score):
    return "%s%s" % (mode, "_s" if use_score else "")


def odd():
    d = os.path.join(MERGE, "odd")
    return read(os.path.join(d, "nodes.dmp")), read(os.path.join(d, "in1.tsv")), read(os.path.join(d, "in2.tsv"))


def odd_output(mode, use_score, tree=True):
    name = suffix(mode, use_score) if tree else "lowest_notree" + ("_s" if use_score else "")
    d = os.path.join(MERGE, "odd")
    return gunzip(os.path.join(d, "out_%s.tsv.gz" % name)), read(os.path.join(d, "sum_%s.txt" % name)).decode()


def real():
    return read(os.path.join(GOLDEN, "nodes.dmp")), read(os.path.join(GOLDEN, "ref_mem_1.tsv")), read(os.path.join(GOLDEN, "ref_greedy_1.tsv"))


def real_output(mode, use_score):
    d = os.path.join(MERGE, "real")
    return gunzip(os.path.join(d, "out_%s.tsv.gz" % suffix(mode, use_score))), read(os.path.join(d, "sum_%s.txt" % suffix(mode, use_score))).decode()


def stop_names():
    return sorted(os.path.basename(f)[:-len(".1.tsv")] for f in glob.glob(os.path.join(MERGE, "stops", "*.1.tsv")))


def stop_case(name):
    """text 1, text 2, use_score, the tool's output and summary (all with -c 1 and no tree)"""
    d = os.path.join(MERGE, "stops")
    return (read(os.path.join(d, name + ".1.tsv")), read(os.path.join(d, name + ".2.tsv")), name.endswith("_s"),
            gunzip(os.path.join(d, name + ".out.tsv.gz")), read(os.path.join(d, name + ".sum.txt")).decode())


# ---- synthetic ------------------------------------------------------------------------------------------------------------
def nodes(pairs):
    return b"".join(b"%d\t|\t%d\t|\tno rank\t|\n" % p for p in pairs)


SMALL_TREE = nodes([(1, 1), (2, 1), (3, 2), (4, 3), (5, 3), (6, 2), (7, 1), (100, 100), (101, 100)])
BIG = 2 ** 64 - 2
DIGIT_TREE = nodes([(1, 1), (5, 1), (6, 1), (1234567890, 1), (20, 1234567890), (21, 1234567890), (1234567890123456789, 1234567890),
                    (30, 1234567890123456789), (31, 1234567890123456789), (BIG, 1234567890123456789), (BIG - 1, BIG), (BIG - 2, BIG)])
NAME_LENGTHS = (0, 1, 15, 16, 17, 33)
NAME_KINDS = ("first", "last", "length")


def name_of(n, salt=0):
    return bytes(97 + (k * 7 + n + salt) % 26 for k in range(n))


def name_compare_equal(shift):
    """names of every length, equal, the lines of text 2 `shift` bytes behind those of text 1"""
    l1 = [b"U\tpad\t0"] + [b"C\t" + name_of(n) + b"\t4" for n in NAME_LENGTHS]
    l2 = [b"U\tpad\t0\t" + b"x" * (shift - 1) if shift else b"U\tpad\t0"] + [b"C\t" + name_of(n) + b"\t5" for n in NAME_LENGTHS]
    return l1, l2


def name_compare_cases():
    """(what, text 1, text 2): per relative alignment the equal names, then one run per length and way to differ: the pair that
    differs follows the equal ones and is followed by a good one"""
    out = []
    for shift in range(CHUNK):
        l1, l2 = name_compare_equal(shift)
        out.append(("name_equal_shift%d" % shift, b"\n".join(l1) + b"\n", b"\n".join(l2) + b"\n"))
        for n in NAME_LENGTHS:
            for kind in NAME_KINDS:
                a = name_of(n)
                if kind == "length":
                    b = a + b"z"
                elif n == 0 or (kind == "last" and n == 1):
                    continue
                else:
                    k = 0 if kind == "first" else n - 1
                    b = a[:k] + bytes([a[k] ^ 1]) + a[k + 1:]
                t1 = l1 + [b"C\t" + a + b"\t4", b"U\tafter\t0"]
                t2 = l2 + [b"C\t" + b + b"\t5", b"U\tafter\t0"]
                out.append(("name_%s_len%d_shift%d" % (kind, n, shift), b"\n".join(t1) + b"\n", b"\n".join(t2) + b"\n"))
    return out


def counted(n, bad=()):
    """n pairs, text 1 with lines of 15 bytes and text 2 with lines of 5: the pairs in `bad` stop"""
    l1 = [b"U\t\t0\t" + b"%09d" % k for k in range(n)]
    l2 = [b"C\t\t%d" % (k % 9 + 1) for k in range(n)]
    for k in bad:
        l2[k] = b"C\t\t"
    join = lambda L: b"".join(l + b"\n" for l in L)
    return join(l1), join(l2)


def small_cases():
    """(what, nodes, text 1, text 2, mode, use_score, final)"""
    C = []
    for n in (0, 1, 255, 256, 257, 700):
        t1, t2 = counted(n)
        C.append(("pairs_%d" % n, None, t1, t2, "1", False, True))
    t1, t2 = counted(700)
    assert 2 * TILE < len(t1) <= 3 * TILE and len(t2) < TILE                # text 1 spans three tiles, text 2 one
    for what, bad in (("stop_0", (0,)), ("stop_256", (256,)), ("stop_last", (699,)), ("stop_two", (650, 300)), ("stop_two_near", (257, 255))):
        t1, t2 = counted(700, bad)
        C.append((what, None, t1, t2, "2", False, True))
    # the number of an LCA: 1, 10, 19 and 20 digits
    ids = [(5, 6), (20, 21), (30, 31), (BIG - 1, BIG - 2), (BIG - 1, 30), (30, BIG - 1), (BIG, BIG - 1), (BIG - 1, BIG)]
    l1 = [b"C\tread%d\t%d\t7" % (k, a) for k, (a, b) in enumerate(ids)]
    l2 = [b"C\tread%d\t%d\t7" % (k, b) for k, (a, b) in enumerate(ids)]
    for mode in ("lca", "lowest"):
        for s in (False, True):
            C.append(("lca_digits_%s" % suffix(mode, s), DIGIT_TREE, b"\n".join(l1) + b"\n", b"\n".join(l2), mode, s, True))
    # ids that are no number or no node, 2^64 - 1 (the key of an empty slot)
    ids = [(b"-1", b"4"), (b"4", b"-1"), (b"18446744073709551615", b"5"), (b"x", b"4"), (b"", b"4"), (b" 4", b"5"), (b"4", b"3"), (b"3", b"4"), (b"4", b"101"),
           (b"999", b"4"), (b"998", b"999"), (b"04", b"4")]
    l1 = [b"C\tr%d\t%s\t1.5" % (k, a) for k, (a, b) in enumerate(ids)]
    l2 = [b"C\tr%d\t%s\t1.50" % (k, b) for k, (a, b) in enumerate(ids)]
    for mode, s in VARIANTS:
        C.append(("ids_%s" % suffix(mode, s), SMALL_TREE, b"\n".join(l1) + b"\n", b"\n".join(l2) + b"\n", mode, s, True))
        if mode != "lca":
            C.append(("ids_notree_%s" % suffix(mode, s), None, b"\n".join(l1) + b"\n", b"\n".join(l2) + b"\n", mode, s, True))
    # a score outside the domain stops a C,C pair under -s and nothing else
    wide1 = b"C\ta\t4\t1\nC\tb\t4\t9007199254740993\nC\tc\t4\t1\n"
    wide2 = b"C\ta\t5\t1\nC\tb\t5\t9007199254740992\nC\tc\t5\t1\n"
    C.append(("score_wide_s", SMALL_TREE, wide1, wide2, "lca", True, True))
    C.append(("score_wide", SMALL_TREE, wide1, wide2, "lca", False, True))
    C.append(("score_wide_cu_s", SMALL_TREE, wide1, wide2.replace(b"C\tb\t5\t9007199254740992", b"U\tb\t0"), "lca", True, True))
    C.append(("score_1e300_s", SMALL_TREE, b"C\ta\t4\t1" + b"0" * 300 + b"\n", b"C\ta\t5\t1\n", "1", True, True))
    C.append(("score_1e309_s", SMALL_TREE, b"C\ta\t4\t1" + b"0" * 309 + b"\n", b"C\ta\t5\t1\n", "1", True, True))
    # ragged ends
    t1, t2 = b"C\ta\t4\nC\tb\t4\nC\tc\t4\nC\td", b"C\ta\t5\nC\tb\t5\nU\tc"
    for final in (False, True):
        C.append(("ragged_final%d" % final, SMALL_TREE, t1, t2, "lca", False, final))
        C.append(("ragged_swapped_final%d" % final, SMALL_TREE, t2, t1, "lca", False, final))
        C.append(("closed_final%d" % final, SMALL_TREE, t1 + b"\t4\n", t2 + b"\t0\nC\td\t5\n", "lca", False, final))
        C.append(("more_in_2_final%d" % final, SMALL_TREE, b"U\ta\t0\n", b"U\ta\t0\nU\tb\t0\n", "1", False, final))
        C.append(("empty_1_final%d" % final, None, b"", b"U\ta\t0\n", "1", False, final))
        C.append(("empty_2_final%d" % final, None, b"U\ta\t0\n", b"", "1", False, final))
        C.append(("both_empty_final%d" % final, None, b"", b"", "1", False, final))
        C.append(("only_newlines_final%d" % final, None, b"\n\n\n", b"\n\n", "1", False, final))
    # a line that ends at every offset of a chunk; a name that spans tiles
    for k in range(CHUNK + 1):
        C.append(("offset_%d" % k, SMALL_TREE, b"C\t" + b"n" * k + b"\t4\t3\nC\tx\t4\t2\n", b"C\t" + b"n" * k + b"\t5\t3\nC\tx\t3\t2.0\n", "lowest", True, True))
    long_name = name_of(2 * TILE + 5)
    C.append(("long_name", SMALL_TREE, b"U\ta\t0\nC\t" + long_name + b"\t4\nU\tz\t0", b"U\ta\t0\nC\t" + long_name + b"\t5\nC\tz\t7\n", "lca", False, True))
    return C


def capacity_case():
    _, t1, t2 = odd()
    return t1, t2
