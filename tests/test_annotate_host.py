"""The host side of kaiju-addTaxonNames that needs no GPU (kaiju_amd/csrc/host/annotate_blocks.h: the reader that cuts the
input into blocks, the options), as a plain executable of its own under the address and undefined-behaviour sanitizers
(tests/tools/annotate_blocks_san.cpp): nothing is loaded into this process."""
import os
import subprocess

import pytest

import annotate_inputs as ai
import util


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("annotate_host") / "annotate_blocks_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", e,
                    os.path.join(util.ROOT, "tests", "tools", "annotate_blocks_san.cpp")], check=True)
    return e


def files(tmp_path):
    out = {"deep": ai.fixture_input("deep"), "odd": ai.fixture_input("odd"), "verbose": ai.verbose_input("mem"), "empty": b"", "newlines": b"\n" * 9,
           "no_newline": b"C\tabc\t7", "closed": b"U\ta\t0\nC\tb\t7\n"}
    paths = {}
    for k, v in out.items():
        paths[k] = str(tmp_path / (k + ".in"))
        with open(paths[k], "wb") as f:
            f.write(v)
    return out, paths


@pytest.mark.parametrize("block", [1, 7, 64, 4096])
def test_blocks_are_the_file_and_end_behind_a_newline(exe, tmp_path, block):
    texts, paths = files(tmp_path)
    for k, text in texts.items():
        o = str(tmp_path / "o.bin")
        r = subprocess.run([exe, "cut", paths[k], str(block), o], capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stderr == b"", (k, r.returncode, r.stderr[-2000:])
        with open(o, "rb") as f:
            assert f.read() == text, k
        rows = [tuple(int(x) for x in l.split()) for l in r.stdout.split(b"\n") if l]
        assert sum(n for n, _, _ in rows) == len(text) and sum(nl for _, nl, _ in rows) == text.count(b"\n"), k
        assert all(closed == 1 for _, _, closed in rows[:-1]) and all(n > 0 for n, _, _ in rows), k
        assert (not rows) == (not text) and (not rows or rows[-1][2] == (1 if text.endswith(b"\n") else 0)), k
        # a block is larger than asked for only where it grew: its first `block` bytes hold no newline (a line longer than a block)
        at = 0
        for n, _, _ in rows:
            assert n <= block or b"\n" not in text[at:at + block], (k, at, n)
            at += n
        if k == "odd" and block == 64:
            assert max(n for n, _, _ in rows) >= 5000 and len(rows) > 10


def test_options(exe):
    def run(*args):
        r = subprocess.run([exe, "opts"] + list(args), capture_output=True, timeout=60)
        assert r.stderr == b"", r.stderr[-2000:]
        return r.returncode, r.stdout
    assert run("-t", "a", "-n", "b", "-i", "c") == (0, b"t=a n=b i=c o= r= v=0 u=0 p=0 h=0\n")
    assert run("-v", "-u", "-p", "-o", "d", "-i", "c", "-n", "b", "-t", "a") == (0, b"t=a n=b i=c o=d r= v=1 u=1 p=1 h=0\n")
    assert run("-r", "genus,species", "-t", "a", "-n", "b", "-i", "c") == (0, b"t=a n=b i=c o= r=genus,species v=0 u=0 p=0 h=0\n")
    for bad, word in ((("-p", "-r", "genus", "-t", "a", "-n", "b", "-i", "c"), b"-p and -r"), (("-n", "b", "-i", "c"), b"-t"), (("-t", "a", "-i", "c"), b"-n"),
                      (("-t", "a", "-n", "b"), b"-i"), (("-t", "a", "-n", "b", "-i"), b"-i"), (("-x",), b"-x")):
        rc, out = run(*bad)
        assert rc == 1 and out.startswith(b"error: ") and word in out, (bad, out)
