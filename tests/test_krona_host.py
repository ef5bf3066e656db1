"""The host side of kaiju2krona that needs no GPU: the loader's names of parents that are no nodes and the splitting of -l,
with the loader and the per-lane functions as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/tools/krona_san.cpp), and the command line's refusals."""
import os
import subprocess

import pytest

import krona_expect as ke
import krona_inputs as ki
import table_inputs as ti
import util
from kaiju_amd import api, build

LISTS = [None, "superkingdom,phylum,genus,species", "superkingdom,genus,,no rank", "tribe", "", ",,,"]       # those of krona_san.cpp


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    """a plain executable of its own: nothing is loaded into this process"""
    tmp = tmp_path_factory.mktemp("krona_san")
    exe = str(tmp / "krona_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(util.ROOT, "tests", "tools", "krona_san.cpp"), os.path.join(util.ROOT, "tests", "emu", "krona_emu.cpp"),
                    os.path.join(util.ROOT, "kaiju_amd", "csrc", "taxon_names.cpp")], check=True)
    r = subprocess.run([exe, ki.NODES, ki.NAMES, ki.NODES, ti.NAMES, ti.REAL_NODES, ti.REAL_NAMES], env=dict(os.environ, TMPDIR=str(tmp)), capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout.rstrip().endswith(b" ok"), (r.returncode, r.stdout[-300:], r.stderr[-2000:])
    return r.stdout


def test_the_loader_keeps_dangling_parent_names_in_every_mode(san):
    lines = [l for l in san.split(b"\n") if l.startswith(b"dangling ")]
    # the only parent that is no node is 499, above genus 500; only the first pair's names.dmp names it
    assert sorted(lines) == [b"dangling %d 500 Dangling parent" % m for m in range(3)]


def test_the_lists_are_split_as_the_tool_splits_them(san):
    """the text of "every node holds 3 reads, 4 lines unclassified" for every list, byte for byte the model's"""
    trees = [ki.fixture_tree(), ti.fixture_tree(), ti.real_tree()]
    at, seen = 0, 0
    while True:
        at = san.find(b"text ", at)
        if at < 0:
            break
        end = san.index(b"\n", at)
        pair, lst, size = (int(x) for x in san[at + 5:end].split())
        text = san[end + 1:end + 1 + size]
        tree = trees[pair]
        assert text == ke.expected(tree, {t: 3 for t in tree.nodes}, 4, True, LISTS[lst])["text"], (pair, lst)
        at, seen = end + 1 + size, seen + 1
    assert seen == len(trees) * len(LISTS)
    assert ke.split_ranks("superkingdom,genus,,no rank") == {b"superkingdom", b"genus", b"no rank"} and ke.split_ranks(",,,") == set() and ke.split_ranks(None) is None


def test_no_existing_table_changes_by_the_dangling_names():
    """the annotations of the tree with and without the line for 499 are the same"""
    for mode in ("name", "path", "ranks:genus,species"):
        a, b = api.TaxonNames(ki.NODES, ki.NAMES, mode), api.TaxonNames(ki.NODES, ti.NAMES, mode)
        assert a.count() == b.count() and a.count(named=True) == b.count(named=True)
        for tid in list(ki.fixture_tree().nodes) + [499, 999]:
            assert a.annotation(tid) == b.annotation(tid), (mode, tid)
        a.close()
        b.close()


def test_entry_points_exist():
    L = api.lib()
    for sym in ("kaiju_gpu_krona_create", "kaiju_gpu_krona_free", "kaiju_gpu_krona_text_device", "kaiju_gpu_krona_text", "kaiju_gpu_krona_pass_ms"):
        assert hasattr(L, sym), sym
    assert hasattr(api, "Krona")


def cli(args, **kw):
    build.build_krona_cli()
    return subprocess.run([build.KRONA_CLI] + args, capture_output=True, timeout=60, **kw)


@pytest.mark.parametrize("missing", ["-o", "-n", "-t", "-i"])
def test_the_command_line_refuses_a_missing_option(tmp_path, missing):
    out = tmp_path / "out.txt"
    given = {"-t": ki.NODES, "-n": ki.NAMES, "-i": ki.FILES["allu"], "-o": str(out)}
    del given[missing]
    r = cli([x for kv in given.items() for x in kv])
    assert r.returncode == 1 and r.stderr.startswith(b"Error: ") and b"usage:" in r.stderr and r.stdout == b""
    assert not out.exists()


def test_the_command_line_refuses_an_unknown_option_and_files_it_cannot_open(tmp_path):
    out = tmp_path / "out.txt"
    ok = {"-t": ki.NODES, "-n": ki.NAMES, "-i": ki.FILES["allu"], "-o": str(out)}
    r = cli([x for kv in ok.items() for x in kv] + ["-x"])
    assert r.returncode == 1 and b"usage:" in r.stderr and not out.exists()
    r = cli(["-h"])
    assert r.returncode == 1 and b"usage:" in r.stderr
    for opt in ("-t", "-n", "-i"):
        args = dict(ok, **{opt: str(tmp_path / "none")})
        r = cli([x for kv in args.items() for x in kv])
        assert r.returncode == 1 and b"Could not open file" in r.stderr and b"usage:" not in r.stderr and not out.exists(), opt
    args = dict(ok, **{"-o": str(tmp_path / "no_such_directory" / "out.txt")})
    r = cli([x for kv in args.items() for x in kv])
    assert r.returncode == 1 and b"for writing" in r.stderr
