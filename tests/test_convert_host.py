"""The host side of kaiju-convertNR that needs no GPU (kaiju_amd/csrc/host/convert_blocks.h: the options, the readers of
merged.dmp and of the list of taxa, the cutter), as a plain executable of its own under the address and undefined-behaviour
sanitizers (tests/tools/convert_blocks_san.cpp): nothing is loaded into this process."""
import os
import subprocess

import pytest

import convert_expect as ce
import util


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("convert_host") / "convert_blocks_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", e,
                    os.path.join(util.ROOT, "tests", "tools", "convert_blocks_san.cpp")], check=True)
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


def test_merged_dmp_by_the_tools_rules(exe, tmp_path):
    text = ce.golden("merged.dmp") + b"12\n\nx 5 | 6\n7|8 junk 9\n  3 | 4\n18446744073709551616 | 1\n18446744073709551615\t|\t2\n9 | 18446744073709551616\n44 abc"
    (tmp_path / "m").write_bytes(text)
    got = [tuple(int(x) for x in l.split()) for l in run(exe, "pairs", tmp_path / "m").stdout.split(b"\n") if l]
    assert got == ce.merged_pairs(text) == [(666, 562), (777, 4242), (666, 9606), (7, 8), (18446744073709551615, 2)]
    first = {}
    for a, b in got:
        first.setdefault(a, b)
    assert first == ce.parse_pairs(text)


def test_the_list_of_taxa_by_the_tools_rules(exe, tmp_path):
    text = ce.golden("list.txt") + b"x\n\n 12 13\n99999999999999999999999\nlast 7"
    (tmp_path / "l").write_bytes(text)
    got = [int(l) for l in run(exe, "list", tmp_path / "l").stdout.split(b"\n") if l]
    assert got == [561, 1386, 99999, 2759, 12, 7]
    nodes = ce.parse_pairs(ce.golden("nodes.dmp"))
    assert [t for t in got if t in nodes] == ce.parse_list(text, nodes) == [561, 1386, 2759]


@pytest.mark.parametrize("name", ["nr.txt", "nr_none.txt"])
def test_records_at_every_block_size(exe, tmp_path, name):
    """every block starts at a header line (the first: at the start of the file), the blocks are the file, and the records of the
    blocks are the records of the file; a block size below the largest record is an error that names a size"""
    text = ce.golden(name)
    (tmp_path / "t").write_bytes(text)
    fx = ce.Fixture()
    whole = fx.expected("a", text=text)
    cuts = [0] + [k + 1 for k in range(len(text) - 1) if text[k:k + 2] == b"\n>"] + [len(text)]
    largest = max(b - a for a, b in zip(cuts, cuts[1:]))
    for block in range(1, len(text) + 3):
        r = run(exe, "cut", "records", tmp_path / "t", block)
        blocks = blocks_of(r.stdout)
        assert all(b[:1] == b">" for b in blocks[1:]) and all(b for b in blocks)
        if r.returncode:
            # (the last record needs no cut behind it: a block may be smaller than it by what the block before took)
            assert block < largest + 1 and r.stderr.startswith(b"error: a record of more than ") and b"".join(blocks) == text[:len(b"".join(blocks))]
            continue
        assert b"".join(blocks) == text and all(len(b) <= max(block, 2) for b in blocks)
        assert b"".join(fx.expected("a", text=b)["text"] for b in blocks) == whole["text"]
        if block >= largest + 1:
            assert r.returncode == 0
    assert run(exe, "cut", "records", tmp_path / "t", len(text) + 5).returncode == 0


def test_lines_at_every_block_size(exe, tmp_path):
    text = ce.golden("map.tsv")
    (tmp_path / "t").write_bytes(text)
    longest = max(len(l) for l in text.split(b"\n")) + 1
    for block in list(range(1, longest + 4)) + [len(text), len(text) + 1]:
        r = run(exe, "cut", "lines", tmp_path / "t", block)
        blocks = blocks_of(r.stdout)
        if r.returncode:
            assert block < longest and r.stderr.startswith(b"error: a line of more than ")
            continue
        assert b"".join(blocks) == text and all(b.endswith(b"\n") for b in blocks[:-1])
    for name, data in (("empty", b""), ("nl", b"\n\n\n"), ("open", b"a\tb\t1")):
        (tmp_path / name).write_bytes(data)
        assert b"".join(blocks_of(run(exe, "cut", "lines", tmp_path / name, 6).stdout)) == data


def test_options_and_the_tools_messages(exe):
    ok = ["-t", "n", "-m", "m", "-g", "g", "-o", "o"]
    assert run(exe, "opts", *ok).stdout == b"t=n m=m g=g o=o i= l= e= a=0 v=0 d=0\n"
    assert run(exe, "opts", "-a", "-v", "-d", "-i", "nr", "-l", "L", "-e", "E", *ok).stdout == b"t=n m=m g=g o=o i=nr l=L e=E a=1 v=1 d=1\n"
    for drop, word in ((0, b"nodes.dmp file, using the -t option."), (2, b"merged.dmp file, using the -m option."), (4, b"prot.accession2taxid file, using the -g option."),
                       (6, b"name of the output file, using the -o option.")):
        r = run(exe, "opts", *(ok[:drop] + ok[drop + 2:]))
        assert r.returncode == 1 and r.stdout.startswith(b"error: Please specify the ") and r.stdout.rstrip().endswith(word)
    for bad in (["-h"], ["-x"], ["-r"], ok + ["-i"]):
        r = run(exe, "opts", *bad)
        assert r.returncode == 1 and r.stdout == b"usage\n"
