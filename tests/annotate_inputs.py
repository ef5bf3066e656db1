"""Inputs of the tests of the stand-alone annotator (tests/test_annotate_emu.py on the host, tests/test_gpu_annotate.py on
the device): the fixtures of tests/golden/names/deep/ and tests/golden/annotate/, the smallest texts at which a pass can go
wrong, and the capacity cases."""
import os

import names_expect
import names_inputs
import util

GOLDEN = os.path.join(util.ROOT, "tests", "golden")
ANNOTATE = os.path.join(GOLDEN, "annotate")
RANKS_DEEP = names_inputs.RANKS_DEEP
FOUR_MODES = [("out_name.tsv", "name", False), ("out_path.tsv", "path", False), ("out_ranks.tsv", RANKS_DEEP, False), ("out_path_u.tsv", "path", True)]
VARIANTS = names_inputs.VARIANTS                                     # {name, path, ranks} x {keep, drop}
TILE, CHUNK = 4096, 16
_memo = {}


def deep_names(mode):
    if ("deep", mode) not in _memo:
        _memo["deep", mode] = names_inputs.deep_expect(mode)
    return _memo["deep", mode]


def golden_names(mode):
    if ("golden", mode) not in _memo:
        _memo["golden", mode] = names_expect.Names(names_inputs.read(os.path.join(GOLDEN, "nodes.dmp")), names_inputs.read(names_inputs.GOLDEN_NAMES), mode)
    return _memo["golden", mode]


def fixture_dir(fixture):
    return os.path.join(names_inputs.NAMES_DIR, "deep") if fixture == "deep" else os.path.join(ANNOTATE, fixture)


def fixture_input(fixture):
    return names_inputs.read(os.path.join(fixture_dir(fixture), "in.tsv"))


def fixture_output(fixture, out):
    return names_inputs.read(os.path.join(fixture_dir(fixture), out))


def verbose_input(run):
    """the reference's `kaiju -v` on the committed reads"""
    return names_inputs.read(os.path.join(GOLDEN, "ref_%s_1.tsv" % run))


def verbose_output(run, kind):
    return names_inputs.read(os.path.join(ANNOTATE, "verbose", "%s.%s.tsv" % (run, kind)))


def sized(n):
    """exactly n bytes of lines over taxa of deep/ (the last line is cut where the size is reached)"""
    taxa = [7, 1039, 0, 12, 777777, 1, 1002, 78]
    out, k = b"", 0
    while len(out) < n:
        t = taxa[k % len(taxa)]
        out += (b"U\tu%d\t0\n" % k) if t == 0 else b"C\tr%d%s\t%d\n" % (k, b"n" * (k * 5 % 23), t)
        k += 1
    return out[:n]


def body_line(n, taxon=1039):
    """a 'C' line whose body has exactly n bytes"""
    tail = b"\t%d" % taxon
    assert n >= 2 + len(tail)
    return b"C\t" + b"b" * (n - 2 - len(tail)) + tail + b"\n"


def small_cases():
    """[(id, text)]"""
    c = [("bytes_%d" % n, sized(n)) for n in (0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1)]
    c.append(("only_newlines", b"\n" * 33))
    c.append(("one_newline", b"\n"))
    c.append(("no_newline", b"C\tabc\t1039"))
    c.append(("no_newline_u", b"U"))
    # bodies of 16 bytes: every line ends one byte further into its chunk than the one before
    c.append(("line_end_every_offset", b"".join(body_line(16, t) for t in [7, 78, 12, 9] * 5)))
    # the second tab and the digit run at every offset of a chunk, in front of and behind the end of a tile
    c.append(("tab_and_run_over_chunks", b"".join(b"U\t" + b"u" * s + b"\t0\n" + b"C\t" + b"n" * 10 + b"\t1039\txx\n" for s in range(20))))
    for k in range(-3, 5):                                          # the second tab at byte TILE - 3 - k
        c.append(("tab_and_run_over_tile_%d" % (k + 3), b"U\t" + b"u" * (TILE - 16 - k - 4) + b"\t0\n" + b"C\t" + b"n" * 10 + b"\t1039\txx\nC\tz\t7\n"))
        assert c[-1][1].index(b"\t1039") == TILE - 3 - k
    # bodies of exactly one and two chunks at offset 0 and 1 of a chunk of the output; with a line of length 0 in front the
    # input lies one byte further than the output
    for pre_id, pre in (("off0", b""), ("off1", b"U" + b"u" * 15 + b"\n"), ("shifted", b"\n"), ("off1_shifted", b"\n\nU" + b"u" * 15 + b"\n")):
        for n in (16, 32):
            c.append(("body_%d_%s" % (n, pre_id), pre + body_line(n) + body_line(n, 12) + b"U\tu\t0\n"))
    c.append(("long_line", b"C\tr\t7\n" + b"C\t" + b"n" * 4990 + b"\t1005\n" + b"X" * 5000 + b"\nC\tq\t1039"))
    c.append(("all_dropped", b"U\ta\t0\n" * 20 + b"\nX\n"))
    return c


def big():
    """names_inputs.BIG_COUNT lines, one more than a step of the block on top of the prefix sum takes; a tenth of length 0"""
    n = names_inputs.BIG_COUNT
    return b"".join(b"\n" if i % 10 == 3 else b"C\tb%d\t%d\n" % (i, i % 10) for i in range(n))


def capacity_text():
    return fixture_input("odd") + b"\n" + fixture_input("deep")


def capacity_caps(e, mode):
    """e: annotate_expect.expected of capacity_text().  0, the exact size, one byte less, one below and one above the end of a
    line in the middle, the middle of the longest body and - in path mode - of a lineage"""
    import numpy as np
    lo, total = e["line_off"], len(e["text"])
    nz = [int(x) for x in lo[1:-1] if 0 < x < total]
    end = nz[len(nz) // 2]
    lens = np.diff(lo)
    r = int(np.argmax(lens))
    assert lens[r] > 5000
    caps = [0, total, total - 1, end - 1, end + 1, int(lo[r]) + 2500]
    if mode == "path":
        want = b"Chain node 39 with spaces; \n"
        at = e["text"].index(want)
        caps.append(at - 300)
    return caps
