"""k_fragments_team (the default stage 1 of single-read batches of at most 191 nt without SEG trigger detection; pairs keep
k_fragments_fast) against
the one-lane k_fragments_fast (KAIJU_GPU_STAGE1=lane) and the general stage 1 (KAIJU_GPU_STAGE1=old): identical hit records
on the golden short reads, on fuzzed single reads and on fuzzed pairs, SEG on and off.  The CPU twin of this comparison, at
the level of peptide areas and fragment lists, is test_stage1_team.py."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gidx(gpu_lib, golden):
    return gpu_lib.Index(golden.fmi)


def fuzz_from(golden, n, seed, lo=1, hi=191):
    """slices of the golden reads (so that many of them match) of lo..hi nt, with substitutions, N, IUPAC letters, lowercase
    and U in a part of them; every tenth one is random sequence"""
    rng = np.random.default_rng(seed)
    src = [np.frombuffer(r, dtype=np.uint8) for r in golden.reads if len(r) >= 200]
    junk = np.frombuffer(b"NnRYKMSWBDHVacgtuU", dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    lens = rng.integers(lo, hi + 1, size=n)
    out = []
    for i in range(n):
        ln = int(lens[i])
        if i % 10 == 9:
            out.append(rng.choice(acgt, size=ln).tobytes())
            continue
        s = src[int(rng.integers(0, len(src)))]
        a = int(rng.integers(0, len(s) - ln + 1))
        r = s[a:a + ln].copy()
        if i % 3 == 1 and ln:
            k = int(rng.integers(1, 4))
            r[rng.integers(0, ln, size=k)] = rng.choice(junk, size=k)
        out.append(r.tobytes())
    return out


def classify_all(api, gidx, mode, seg, seqs, off, paired, monkeypatch):
    got = {}
    for v in ("team", "lane", "old"):
        if v == "team":
            monkeypatch.delenv("KAIJU_GPU_STAGE1", raising=False)
        else:
            monkeypatch.setenv("KAIJU_GPU_STAGE1", v)
        clf = api.Classifier(gidx, api.default_params(mode, seg=seg))
        got[v] = clf.classify(seqs, off, paired=paired)
        assert clf.stats().error_flags == 0, v
        clf.close()
    monkeypatch.delenv("KAIJU_GPU_STAGE1", raising=False)
    return got


CASES = [("mem", 1), ("mem", 0), ("greedy", 0)]


@pytest.mark.parametrize("mode,seg", CASES)
def test_golden_short(gpu_lib, golden, gidx, mode, seg, monkeypatch):
    _, seqs, off = golden.short()
    got = classify_all(gpu_lib, gidx, mode, seg, seqs, off, False, monkeypatch)
    assert (got["team"] == got["lane"]).all() and (got["team"] == got["old"]).all()


@pytest.mark.parametrize("mode,seg", CASES)
def test_fuzzed_reads_and_pairs(gpu_lib, golden, gidx, mode, seg, monkeypatch):
    n1, n2 = (200_000, 100_000) if mode == "mem" else (50_000, 25_000)
    seqs, off = util.pack(fuzz_from(golden, n1, 31))
    got = classify_all(gpu_lib, gidx, mode, seg, seqs, off, False, monkeypatch)
    assert (got["team"]["best"] > 0).sum() > n1 // 4
    for v in ("lane", "old"):
        bad = np.nonzero(got["team"] != got[v])[0]
        assert not len(bad), (v, bad[:5])
    a, b = fuzz_from(golden, n2, 32, lo=0), fuzz_from(golden, n2, 33, lo=0)
    for i in range(0, n2, 13):
        b[i] = b""
    seqs, off = util.pack(a, b)
    got = classify_all(gpu_lib, gidx, mode, seg, seqs, off, True, monkeypatch)
    for v in ("lane", "old"):
        bad = np.nonzero(got["team"] != got[v])[0]
        assert not len(bad), (v, "pairs", bad[:5])
