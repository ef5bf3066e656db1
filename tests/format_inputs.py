"""Inputs of the format tests (tests/test_format_emu.py on the host, tests/test_gpu_format.py on the device): synthetic 16-byte
records, off[], name spans and the text the names lie in; nothing is classified.  Every case is the smallest shape that can
break one pass of kaiju_amd/csrc/format.hip.  cases(B, S, K, golden_db) wants the bytes of output per block, the records per
scan block and the entries of the E-value table as the implementation exports them (format_emu_constants), and db_length of
the golden index.

A case is a dict: id, mode ("mem" / "greedy"), protein, min_evalue, db ("golden" or a number: contexts on a device can only
have the golden index's db_length), paired, recs (COMPACT_DTYPE), off (uint64, 2n + 1), names (NAME_SPAN_DTYPE), text1.

    python tests/format_inputs.py CASES      writes every case with its expected output, the capacity cases included, for
                                             the stand-alone build of tests/emu/format_emu.cpp (-DFORMAT_EMU_MAIN)"""
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
from kaiju_amd import api

TAXA = [1, 9, 10, 99, 100] + [10 ** k - 1 for k in range(3, 20)] + [10 ** k for k in range(3, 20)] + [2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1]
NAME_LENGTHS = (0, 1, 15, 16, 17, 255, 256, 257, 4099)
RECORD_COUNTS = (0, 1, 15, 16, 17, 255, 256, 257)
GATE_LEN1, GATE_LEN2, GATE_PROTEIN_LEN1 = (33, 100, 150, 151, 300), (0, 149, 150), (11, 50, 1000)
INEXACT = 0x80000000


def make(cid, names, recs, mode="mem", lens=None, paired=False, protein=False, min_evalue=0.01, db="golden", gap=b"\n@", tail=b""):
    """names: list of bytes; they are laid into text1 one behind the other, each behind `gap` (bytes, or a list of one per name)"""
    n = len(names)
    parts, spans, at = [], np.zeros(n, dtype=api.NAME_SPAN_DTYPE), 0
    for r, nm in enumerate(names):
        g = gap[r] if isinstance(gap, list) else gap
        parts += [g, nm]
        spans[r] = (at + len(g), len(nm))
        at += len(g) + len(nm)
    text1 = b"".join(parts) + tail
    lens = lens if lens is not None else [(150, 0)] * n
    off = np.zeros(2 * n + 1, dtype=np.uint64)
    if n:
        off[1:] = np.cumsum(np.asarray(lens, dtype=np.uint64).reshape(-1))
    rec = np.zeros(n, dtype=api.COMPACT_DTYPE)
    for r, (lca, best, info) in enumerate(recs):
        rec[r] = (lca, best, info)
    return {"id": cid, "mode": mode, "protein": protein, "min_evalue": min_evalue, "db": db, "paired": paired, "recs": rec, "off": off,
            "names": spans, "text1": text1}


def _counts(n, seed):
    rng = np.random.default_rng(seed)
    names = [b"r%d" % i for i in range(n)]
    tax = rng.choice(np.asarray([0] + TAXA[:12], dtype=np.uint64), n) if n else []
    return names, [(int(t), 7, 1) for t in tax]


def _grid():
    """every alignment of a name in the text (0 .. 15) against every alignment of its place in the output (0 .. 15): for each
    pair a filler record steers the output, a gap steers the text.  All lines are 'C' lines with a one-digit taxon"""
    names, gaps, o, at = [], [], 0, 0
    want = []
    for s in range(16):
        for d in range(16):
            fl = (d - (o + 5 + 2)) % 16                      # the filler's line: 5 + fl bytes, then "C\t" of the next line
            for nm, target in ((b"f" * fl, None), (bytes([65 + s, 97 + d, 0x80 + s, 9, 13, 48 + d % 10])[: 1 + (s + d) % 6], s)):
                g = b"\n@" if target is None else b"\n" + b"@" * (1 + (target - (at + 2)) % 16)
                gaps.append(g); names.append(nm)
                if target is not None:
                    want.append((s, d, at + len(g), o + 2))
                at += len(g) + len(nm)
                o += 5 + len(nm)
    for s, d, src, dst in want:
        assert src % 16 == s and dst % 16 == d
    return names, gaps, [(7, 20, 1)] * len(names)


def _flip(fin, params, db_length, len1, len2, paired, K):
    """the smallest score the gate lets pass, by the host function alone (the gate is monotone in the score)"""
    n = K + 2
    recs = np.zeros(n, dtype=api.COMPACT_DTYPE)
    recs["lca"], recs["best"], recs["info"] = 5, np.arange(n), 1
    off = np.zeros(2 * n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.tile(np.asarray([len1, len2], dtype=np.uint64), n))
    ok = fin(params, db_length, recs, off, paired)["classified"]
    first = int(np.argmax(ok))
    assert ok[first] and not ok[1:first].any() and ok[first:].all()
    return first


def cases(B, S, K, golden_db):
    from format_expect import finalize, params_of
    c = []
    # record counts: one block, one more, the block on top of the scan in its second step
    for n in RECORD_COUNTS + (S * S + 1,):
        names, recs = _counts(n, 100 + n)
        c.append(make("n_%d" % n, names, recs))
    # names: lengths, bytes that are not letters, the last one ending at the last byte of a text that is no multiple of 16
    rng = np.random.default_rng(5)
    alphabet = np.asarray([b for b in range(256) if b != 10], dtype=np.uint8)
    names = [bytes(rng.choice(alphabet, l).tolist()) for l in NAME_LENGTHS] + [b"tab\there", b"cr\r", b"\xff\x80\xfe", b"0123456789", b"last"]
    k = make("name_lengths", names, [(TAXA[i % len(TAXA)], 3, 2) for i in range(len(names))])
    if len(k["text1"]) % 16 == 0:
        k = make("name_lengths", names, [(TAXA[i % len(TAXA)], 3, 2) for i in range(len(names))], gap=b"\n@@")
    assert len(k["text1"]) % 16 != 0 and int(k["names"][-1]["pos"]) + int(k["names"][-1]["len"]) == len(k["text1"])
    c.append(k)
    names, gaps, recs = _grid()
    c.append(make("alignment_grid", names, recs, gap=gaps))
    # taxon ids, and the three kinds of record that stay undecided; two records flagged inexact
    recs = [(t, 9, 3) for t in TAXA] + [(77, 9, 0), (77, 0, 2), (0, 9, 2), (0, 0, 0), (12, 9, 1 | INEXACT), (0, 9, 1 | INEXACT)]
    c.append(make("taxon_ids", [b"t%d" % i for i in range(len(recs))], recs))
    assert B > 64 and S > 2
    # the E-value gate: per group every pair of lengths with the scores around the flip and at the ends of the table
    groups = [(pe, False, db, me) for pe in (False, True) for db in ("golden", 1e12) for me in (0.01, 1e-30)]
    groups += [(False, True, db, me) for db in ("golden", 1e12) for me in (0.01, 1e-30)]
    for pe, prot, db, me in groups:
        lens = [(l1, 0) for l1 in GATE_PROTEIN_LEN1] if prot else [(l1, l2) for l1 in GATE_LEN1 for l2 in GATE_LEN2]
        proto = {"mode": "greedy", "protein": prot, "min_evalue": me}
        dbl = golden_db if db == "golden" else db
        recs, rl = [], []
        for l1, l2 in lens:
            f = _flip(finalize, params_of(proto), dbl, l1, l2, pe, K)
            assert 2 <= f < K - 2
            for best in (f - 1, f, f + 1, 1, K - 1, K, K + 1, 2 ** 32 - 1):
                recs.append((1000 + best % 997, best, 1)); rl.append((l1, l2))
        names = [b"g%d" % i for i in range(len(recs))]
        gid = "%s_%s_db_%s_E_%g" % ("pairs" if pe else "single", "protein" if prot else "nt", db, me)
        c.append(make("gate_" + gid, names, recs, mode="greedy", lens=rl, paired=pe, protein=prot, min_evalue=me, db=db))
        c.append(make("nogate_" + gid, names, recs, mode="mem", lens=rl, paired=pe, protein=prot, min_evalue=me, db=db))
    return c


def capacity_cases(all_cases, expect):
    """(case, out_cap) for the exact length, one byte less, the offset of a line in the middle and 0; expect(case) -> dict of
    format_expect.expected"""
    out = []
    for case in all_cases:
        if case["id"] not in ("n_17", "n_257", "name_lengths", "alignment_grid", "taxon_ids"):
            continue
        e = expect(case)
        total, mid = len(e["text"]), int(e["line_off"][len(e["line_off"]) // 2])
        assert 0 < mid < total - 1
        out += [(case, total), (case, total - 1), (case, mid), (case, 0)]
    return out


def main(path):
    import struct

    import format_expect
    import util
    with open(util.Golden().fmi, "rb") as f:
        hdr = np.frombuffer(f.read(12), dtype=np.uint8)
    golden_db = float(int(hdr[:8].view("<i8")[0]) - int(hdr[8:12].view("<i4")[0]))
    all_cases = cases(4096, 256, 4096, golden_db)
    dbl = lambda case: golden_db if case["db"] == "golden" else case["db"]
    jobs = [(k, None) for k in all_cases] + capacity_cases(all_cases, lambda k: format_expect.expected(k, dbl(k)))
    pw = np.zeros(4096)
    assert api.lib().kaiju_gpu_format_evalue_table(pw.ctypes.data, len(pw)) == 0
    with open(path, "wb") as f:
        f.write(pw.tobytes())
        for case, cap in jobs:
            e = format_expect.expected(case, dbl(case), cap)
            cap = len(e["text"]) + 5 if cap is None else cap
            n = len(case["recs"])
            f.write(struct.pack("<7Q2d", n, int(case["paired"]), len(case["text1"]), 1 if case["mode"] == "greedy" else 0, int(case["protein"]),
                                cap, len(e["written"]), dbl(case), case["min_evalue"]))
            info = np.zeros(1, dtype=format_expect.FORMAT_INFO_DTYPE)
            for k, v in e["info"].items():
                info[0][k] = v
            f.write(info.tobytes() + case["recs"].tobytes() + case["names"].tobytes() + case["off"].tobytes() + case["text1"] + e["written"])
    print("%d cases written to %s" % (len(jobs), path))


if __name__ == "__main__":
    main(sys.argv[1])
