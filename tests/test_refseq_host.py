"""The one piece of host code kaiju-convertRefSeq has beyond kaiju_amd/csrc/host/convert_blocks.h - its options
(kaiju_amd/csrc/host/refseq_options.h) - as a plain executable of its own under the address and undefined-behaviour sanitizers
(tests/tools/refseq_options_san.cpp): nothing is loaded into this process.  And the cutter of convert_blocks.h
(tests/tools/convert_blocks_san.cpp) on the RefSeq fixture: the records of the blocks are the records of the file."""
import os
import subprocess

import pytest

import refseq_expect as rs
import util

SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("refseq_host")
    out = {}
    for name in ("refseq_options_san", "convert_blocks_san"):
        out[name] = str(d / name)
        subprocess.run(SAN + ["-o", out[name], os.path.join(util.ROOT, "tests", "tools", name + ".cpp")], check=True)
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=120)
    assert r.returncode in (0, 1) and (r.returncode == 1 or r.stderr == b""), (r.returncode, r.stderr[-2000:])
    return r


def test_options_and_the_tools_messages(exes):
    exe = exes["refseq_options_san"]
    ok = ["-t", "n", "-m", "m", "-g", "g", "-o", "o"]
    assert run(exe, *ok).stdout == b"t=n m=m g=g o=o i= l= e= a=0 v=0 d=0\n"
    assert run(exe, "-a", "-v", "-d", "-l", "L", *ok).stdout == b"t=n m=m g=g o=o i= l=L e= a=1 v=1 d=1\n"
    assert run(exe, "-avd", "-lL", *ok).stdout == b"t=n m=m g=g o=o i= l=L e= a=1 v=1 d=1\n"
    for drop, word in ((0, b"nodes.dmp file, using the -t option."), (2, b"merged.dmp file, using the -m option."), (4, b"prot.accession2taxid file, using the -g option."),
                       (6, b"name of the output file, using the -o option.")):
        r = run(exe, *(ok[:drop] + ok[drop + 2:]))
        assert r.returncode == 1 and r.stdout.startswith(b"error: Please specify the ") and r.stdout.rstrip().endswith(word)
    # -i, -e and -r stand in the tool's option string and end in its usage text; so do -h, an unknown option and a missing argument
    for bad in (["-h"], ["-x"], ok + ["-r"], ok + ["-i", "nr"], ok + ["-e", "E"], ["-i", "nr"] + ok, ok + ["-i"], ok + ["-l"], ["-e"]):
        r = run(exe, *bad)
        assert r.returncode == 1 and r.stdout == b"usage\n", bad
    assert run(exe).stdout.startswith(b"error: Please specify the location of the nodes.dmp file")


def blocks_of(out):
    blocks, at = [], 0
    while at < len(out):
        nl = out.index(b"\n", at)
        n = int(out[at:nl])
        blocks.append(out[nl + 1:nl + 1 + n])
        at = nl + 1 + n
    return blocks


@pytest.mark.parametrize("name", ["faa.txt", "faa_none.txt"])
def test_the_records_of_the_blocks_are_the_records_of_the_file(exes, tmp_path, name):
    text = rs.golden(name)
    (tmp_path / "t").write_bytes(text)
    fx = rs.Fixture()
    whole = fx.expected("a", text=text)
    cuts = [0] + [k + 1 for k in range(len(text) - 1) if text[k:k + 2] == b"\n>"] + [len(text)]
    largest = max(b - a for a, b in zip(cuts, cuts[1:]))
    for block in (largest + 1, largest + 2, 2 * largest, 300, len(text) + 5):
        r = run(exes["convert_blocks_san"], "cut", "records", tmp_path / "t", block)
        blocks = blocks_of(r.stdout)
        assert r.returncode == 0 and b"".join(blocks) == text and all(b[:1] == b">" for b in blocks[1:])
        assert b"".join(fx.expected("a", text=b)["text"] for b in blocks) == whole["text"]
    r = run(exes["convert_blocks_san"], "cut", "records", tmp_path / "t", 5)
    assert r.returncode == 1 and r.stderr.startswith(b"error: a record of more than ")
