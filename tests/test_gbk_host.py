"""The host side of kaiju-gbk2faa that needs no GPU (kaiju_amd/csrc/host/gbk_blocks.h: the arguments, the look at the first
bytes of the input, the cutter at line ends), as a plain executable of its own under the address and undefined-behaviour
sanitizers (tests/tools/gbk_blocks_san.cpp): nothing is loaded into this process."""
import gzip
import os
import subprocess

import pytest

import gbk_expect as ge
import util


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("gbk_host") / "gbk_blocks_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", e,
                    os.path.join(util.ROOT, "tests", "tools", "gbk_blocks_san.cpp")], check=True)
    return e


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=120)
    assert r.returncode in (0, 1) and (r.returncode == 1 or r.stderr == b""), (r.returncode, r.stderr[-2000:])
    return r


def blocks_of(out):
    blocks, at = [], 0
    while at < len(out):
        nl = out.index(b"\n", at)
        n = int(out[at:nl])
        blocks.append(out[nl + 1:nl + 1 + n])
        at = nl + 1 + n
    return blocks


@pytest.mark.parametrize("name", ["rules", "crlf", "tail_open"])
def test_lines_at_every_block_size(exe, tmp_path, name):
    """the blocks are the file, every block but the last ends behind a '\\n', the model block by block writes the script's file;
    a block size below the longest line is an error that names a size"""
    text = ge.golden(name + ".gbk")
    (tmp_path / "t").write_bytes(text)
    longest = max(len(l) for l in text.split(b"\n")) + 1
    for block in list(range(1, longest + 4)) + [200, len(text), len(text) + 1]:
        r = run(exe, "cut", tmp_path / "t", block)
        blocks = blocks_of(r.stdout)
        if r.returncode:
            assert block < longest and r.stderr.startswith(b"error: a line of more than ") and b"".join(blocks) == text[:len(b"".join(blocks))]
            continue
        assert b"".join(blocks) == text and all(b.endswith(b"\n") for b in blocks[:-1]) and all(len(b) <= max(block, 2) for b in blocks)
        cuts, at = [], 0
        for b in blocks[:-1]:
            at += len(b)
            cuts.append(at)
        assert ge.convert_blocks(text, cuts)[0] == ge.golden(name + ".faa")
    assert run(exe, "cut", tmp_path / "t", longest).returncode == 0
    for data in (b"", b"\n\n\n", b"no line end"):
        (tmp_path / "d").write_bytes(data)
        assert b"".join(blocks_of(run(exe, "cut", tmp_path / "d", 12).stdout)) == data


def test_the_first_bytes_of_the_input(exe, tmp_path):
    cases = [(ge.golden("record.gbk"), b"plain\n"), (gzip.compress(b"LOCUS\n"), b"gzip\n"), (b"", b"plain\n"), (b"\x1f", b"plain\n"), (b"BZh91AY&SY", b"refused bzip2\n"),
             (b"\xfd7zXZ\x00\x00\x04", b"refused xz\n"), (b"\x28\xb5\x2f\xfd\x04", b"refused zstd\n"), (b"PK\x03\x04\x14", b"refused zip\n"), (b"LZIP\x01", b"refused lzip\n"),
             (b"\x89LZO\x00", b"refused lzop\n"), (b"\x5d\x00\x00\x80\x00", b"refused lzma\n"), (b"\x1f\x9d\x90", b"refused compress (.Z)\n"), (b"BZ", b"plain\n")]
    for data, want in cases:
        (tmp_path / "f").write_bytes(data)
        assert run(exe, "sniff", tmp_path / "f").stdout == want, data


def test_the_arguments(exe):
    assert run(exe, "opts", "a.gbff.gz", "b.faa").stdout == b"in=a.gbff.gz out=b.faa v=0\n"
    assert run(exe, "opts", "-v", "a", "b").stdout == b"in=a out=b v=1\n" == run(exe, "opts", "a", "b", "-v").stdout
    assert run(exe, "opts", "a", "b", "ignored").stdout == b"in=a out=b v=0\n"               # (the script looks at two)
    assert run(exe, "opts", "--", "-a", "-b").stdout == b"in=-a out=-b v=0\n" and run(exe, "opts", "-", "b").stdout == b"in=- out=b v=0\n"
    for bad in ([], ["a"], ["-v", "a"], ["-v"]):
        r = run(exe, "opts", *bad)
        assert r.returncode == 1 and r.stdout == b"usage\n", bad
    for bad in (["-x", "a", "b"], ["a", "-h", "b"], ["--help"]):
        r = run(exe, "opts", *bad)
        assert r.returncode == 1 and r.stdout.startswith(b"error: unknown option "), bad
