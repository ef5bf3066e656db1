"""Inputs of the tests of the column of kaiju-addTaxonNames (tests/test_format_names_emu.py on the host,
tests/test_gpu_format_names.py on the device): the trees of tests/golden/names/, the six variants every case runs in, the
capacity cases, and records drawn over every taxon of deep/."""
import gzip
import os

import numpy as np

import format_inputs
import names_expect
import util

NAMES_DIR = os.path.join(util.ROOT, "tests", "golden", "names")
DEEP_NODES, DEEP_NAMES = os.path.join(NAMES_DIR, "deep", "nodes.dmp"), os.path.join(NAMES_DIR, "deep", "names.dmp")
GOLDEN_NAMES = os.path.join(NAMES_DIR, "golden", "names.dmp")
RANKS_DEEP, RANKS_GOLDEN = "ranks:genus,species,phylum,genus", "ranks:family,genus,species"
MODES = ("name", "path", RANKS_DEEP)
VARIANTS = [(m, d) for m in MODES for d in (False, True)]          # mode, drop_unclassified
BIG_COUNT = 256 * 256 + 1             # more records than one step of the block on top of the prefix sum takes


def read(path):
    """the bytes of a file; the tool's recorded outputs under tests/golden/names/ are kept gzip'ed (<path>.gz)"""
    if not os.path.exists(path) and os.path.exists(path + ".gz"):
        with gzip.open(path + ".gz", "rb") as f:
            return f.read()
    with open(path, "rb") as f:
        return f.read()


def deep_expect(mode):
    return names_expect.Names(read(DEEP_NODES), read(DEEP_NAMES), mode)


def deep_taxa():
    """every node of deep/, and taxa that are none"""
    return sorted(names_expect.parse_nodes(read(DEEP_NODES))) + [4000, 61, 777777, 2, 2 ** 64 - 1]


def drawn(n, seed=7):
    """n records over every taxon of deep/ (each at least once when n allows), a fifth of them unclassified, names of 0 to 40
    bytes: a case like those of format_inputs"""
    rng = np.random.default_rng(seed)
    taxa = deep_taxa()
    pick = [taxa[i % len(taxa)] for i in rng.permutation(max(n, len(taxa)))[:n]] if n >= len(taxa) else [taxa[i] for i in rng.choice(len(taxa), n)]
    recs = [(0, 5, 1) if rng.random() < 0.2 else (t, 5, 1) for t in pick]
    names = [b"d%d" % i + b"n" * int(rng.integers(0, 38)) for i in range(n)]
    return format_inputs.make("drawn_%d" % n, names, recs)


def big():
    """BIG_COUNT records with short names and a one-digit taxon each (0: not classified; 1, 7 and 9 are nodes of deep/, the others
    are unknown there)"""
    n = BIG_COUNT
    return format_inputs.make("big_%d" % n, [b"b%d" % i for i in range(n)], [(i % 10, 5, 1) for i in range(n)])


def capacity_jobs(cases, expect):
    """(case, mode, drop, out_cap): 0, the exact size, one byte less, one below and one above the end of a line in the middle,
    and - in path mode - the middle of a lineage.  expect(case, mode, drop) -> dict of names_expect.expected"""
    out = []
    for case in cases:
        if case["id"] not in ("n_17", "n_257", "taxon_ids", "drawn_300"):
            continue
        for mode, drop in (("path", False), ("path", True), ("name", True), (RANKS_DEEP, False)):
            e = expect(case, mode, drop)
            total, lo = len(e["text"]), e["line_off"]
            end = int(lo[len(lo) // 2])
            assert 1 < end < total - 1
            caps = [0, total, total - 1, end - 1, end + 1]
            if mode == "path":
                lens = np.diff(lo)
                r = int(np.argmax(lens))                            # the longest line: most of it is lineage
                assert lens[r] > 100
                caps.append(int(lo[r + 1]) - int(lens[r]) // 3)
            out += [(case, mode, drop, c) for c in caps]
    return out
