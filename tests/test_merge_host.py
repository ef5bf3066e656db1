"""The host side of kaiju-mergeOutputs that needs no GPU (kaiju_amd/csrc/host/merge_blocks.h: the reader that hands two files
out in pieces, the options), as a plain executable of its own under the address and undefined-behaviour sanitizers
(tests/tools/merge_blocks_san.cpp): nothing is loaded into this process."""
import os
import subprocess

import pytest

import merge_inputs as mi
import util


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("merge_host") / "merge_blocks_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", e,
                    os.path.join(util.ROOT, "tests", "tools", "merge_blocks_san.cpp")], check=True)
    return e


def pairs_of_files():
    """name -> (text 1, text 2): the same number of lines unless the name says otherwise"""
    _, o1, o2 = mi.odd()
    _, r1, r2 = mi.real()
    short = b"".join(b"U\t%d\t0\n" % k for k in range(400))
    long = b"".join(b"C\t%d\t7\t%s\n" % (k, b"x" * 50 * 8) for k in range(400))        # lines 50 times as long
    return {"odd": (o1, o2), "real": (r1, r2), "long_1": (long, short), "long_2": (short, long), "empty": (b"", b""), "closed": (b"U\ta\t0\nC\tb\t7\n", b"U\ta\t0\nU\tb\t0\n"),
            "no_newline_1": (b"U\ta\t0\nC\tb\t7", b"U\ta\t0\nU\tb\t0\n"), "no_newline_2": (b"U\ta\t0\nC\tb\t7\n", b"U\ta\t0\nU\tb\t0"),
            "no_newline_both": (b"U\ta\t0\nC\tb\t7", b"U\ta\t0\nU\tb\t0"), "newlines": (b"\n" * 9, b"\n" * 9),
            "more_lines_1": (short, short[:600]), "more_lines_2": (short[:600], short), "more_lines_1_open": (short[:-1], short[:599]),
            "empty_1": (b"", short), "empty_2": (long, b"")}


def run(exe, tmp_path, t1, t2, block):
    p = [str(tmp_path / n) for n in ("in1", "in2", "out1", "out2")]
    for path, text in zip(p, (t1, t2)):
        with open(path, "wb") as f:
            f.write(text)
    r = subprocess.run([exe, "read", p[0], p[1], str(block), p[2], p[3]], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr[-2000:])
    rows = [tuple(int(x) for x in l.split()) for l in r.stdout.split(b"\n") if l]
    return rows, open(p[2], "rb").read(), open(p[3], "rb").read()


@pytest.mark.parametrize("block", [1, 7, 4096])
def test_pieces_are_the_files(exe, tmp_path, block):
    for name, (t1, t2) in pairs_of_files().items():
        rows, u1, u2 = run(exe, tmp_path, t1, t2, block)
        longest = max(len(l) for l in (t1 + b"\n" + t2).split(b"\n")) + 1
        if name.startswith(("more_lines", "empty_")):
            # the longer file is read up to the line the shorter one has no partner for, and that line is in the last piece
            n = min(len(mi.merge_expect.split_lines(t1)), len(mi.merge_expect.split_lines(t2)))
            cut = lambda t: len(b"".join(l + b"\n" for l in t.split(b"\n")[:n + 1])[:len(t)])
            # (or to its end, where the end came with the same piece)
            assert t1.startswith(u1) and t2.startswith(u2) and len(u1) >= cut(t1) and len(u2) >= cut(t2), name
            assert block > 7 or (u1, u2) == (t1[:cut(t1)], t2[:cut(t2)]), name
            assert rows[-1][2] == 1 and (block > 7 or 0 in rows[-1][:2]), (name, rows[-1])
        else:
            assert (u1, u2) == (t1, t2), name
            assert (not rows) == (not t1 and not t2), name
            assert all(not final for _, _, final, _, _ in rows[:-1]) and (rows[-1][2] == 1 or t1.endswith(b"\n") and t2.endswith(b"\n")) if rows else True, name
        # no side piles up: a piece holds a block, or the line that did not fit one and the block behind it
        assert all(b1 <= block + longest and b2 <= block + longest for b1, b2, _, _, _ in rows), (name, max(rows))
        assert all(final or u1 or u2 or b1 + b2 < 2 * (block + longest) for b1, b2, final, u1, u2 in rows), name
        if name in ("long_1", "long_2") and block == 4096:
            assert len(rows) > 30 and sum(1 for r in rows if r[2]) == 1


def test_options(exe):
    def run(*args):
        r = subprocess.run([exe, "opts"] + list(args), capture_output=True, timeout=60)
        assert r.stderr == b"", r.stderr[-2000:]
        return r.returncode, r.stdout
    assert run("-i", "a", "-j", "b", "-t", "n") == (0, b"i=a j=b o= t=n c=lca mode=2 s=0 v=0 d=0 h=0\n")
    assert run("-i", "a", "-j", "b", "-c", "1") == (0, b"i=a j=b o= t= c=1 mode=0 s=0 v=0 d=0 h=0\n")
    assert run("-s", "-v", "-d", "-o", "x", "-c", "lowest", "-j", "b", "-i", "a") == (0, b"i=a j=b o=x t= c=lowest mode=3 s=1 v=1 d=1 h=0\n")
    assert run("-i", "a", "-j", "b", "-c", "2", "-t", "n") == (0, b"i=a j=b o= t=n c=2 mode=1 s=0 v=0 d=0 h=0\n")
    assert run("-h")[1].endswith(b"h=1\n")
    for bad, word in ((("-i", "a", "-j", "b"), b"LCA mode requires"), (("-i", "a", "-j", "b", "-c", "3"), b"-c must be"), (("-j", "b", "-c", "1"), b"-i option"),
                      (("-i", "a", "-c", "1"), b"-j option"), (("-i", "a", "-j"), b"-j"), (("-x",), b"-x"), (("-i", "a", "-j", "b", "-c", "LCA", "-t", "n"), b"-c must be")):
        rc, out = run(*bad)
        assert rc == 1 and out.startswith(b"error: ") and word in out, (bad, out)
