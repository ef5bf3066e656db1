"""What the merger (kaiju_amd/csrc/merge.hip) costs, with HIP events, beside the reference tool on the same files (needs a GPU;
the reference binary is oracle/_ref/kaiju-mergeOutputs, built by tests/golden/make_golden_merge.py - without it only the device
side is timed):

    python tests/tools/merge_timing.py [--work DIR] [--lines 10000000] [--reps 5]

Two synthetic texts of `lines` lines each over the benchmark's tree (kaiju_amd/synth.py), sorted alike: about half of the pairs
classified alike, 30 % classified with two different taxa (a conflict: siblings, cousins or taxa of two families), the rest
classified in one file only or in neither.  Once with three columns and once with a score column (equal scores on most of the
conflicts, so that -c decides them).  Timed, -c lca, on device-resident buffers:

    total       kaiju_gpu_merge_text_device, all passes, between two events on the stream (median, lowest, highest of `reps`)
    passes      the events a merger created with KAIJU_GPU_MERGE_TIMES=1 records between its passes (kaiju_gpu_merge_pass_ms;
                medians)
    reference   the wall time of the reference tool from the files to a file, page cache warm

The device's text must equal the reference's file byte for byte.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools")]
from kaiju_amd import api, synth  # noqa: E402
from format_names_timing import Events  # noqa: E402
from test_gpu_parity import Hip  # noqa: E402

PASSES = ("lines_and_plan", "pair", "count", "offsets", "write", "finish")
REF = os.path.join(ROOT, "oracle", "_ref", "kaiju-mergeOutputs")


def make_texts(n, leaves, with_score, seed=4711):
    """the two texts: bytes"""
    rng = np.random.default_rng(seed)
    kind = rng.random(n)
    a = leaves[rng.integers(0, len(leaves), n)]
    step = rng.choice(np.array([1, 3, 10, 100, 1000]), n)                    # siblings ... taxa of other families
    b = np.where(kind < 0.5, a, leaves[(np.searchsorted(leaves, a) + step) % len(leaves)])
    c1 = kind < 0.9                                                          # 0.8 - 0.9: only in file 1; 0.9 - 0.95: only in file 2; behind: in neither
    c2 = (kind < 0.8) | ((kind >= 0.9) & (kind < 0.95))
    s1 = rng.integers(60, 400, n)
    s2 = np.where(rng.random(n) < 0.7, s1, rng.integers(60, 400, n))
    out = []
    for cls, tax, score in ((c1, a, s1), (c2, b, s2)):
        if with_score:
            lines = ["C\tr%d\t%d\t%d" % (i, t, s) if c else "U\tr%d\t0" % i for i, (c, t, s) in enumerate(zip(cls.tolist(), tax.tolist(), score.tolist()))]
        else:
            lines = ["C\tr%d\t%d" % (i, t) if c else "U\tr%d\t0" % i for i, (c, t) in enumerate(zip(cls.tolist(), tax.tolist()))]
        out.append(("\n".join(lines) + "\n").encode())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/kaiju_amd_bench")
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    W, n = args.work, args.lines
    os.makedirs(W, exist_ok=True)
    lines, leaves = synth.make_taxonomy()
    nodes = f"{W}/nodes.dmp"
    synth.write_nodes_dmp(nodes, lines)
    leaves = np.sort(np.asarray(leaves, dtype=np.int64))

    os.environ["KAIJU_GPU_MERGE_TIMES"] = "1"
    hip = Hip()
    ev = Events(hip)
    tax = api.Taxonomy(nodes)
    dtax = api.DeviceTaxonomy(tax, 0)
    stream = hip.stream()
    L = api.lib()
    L.kaiju_gpu_merge_pass_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    res = {"lines": n, "reps": args.reps, "conflict": "lca"}
    ok = True
    for with_score in (False, True):
        key = "score" if with_score else "three_column"
        t0 = time.time()
        t1, t2 = make_texts(n, leaves, with_score)
        print(f"{key}: {len(t1)} + {len(t2)} bytes made in {time.time() - t0:.1f}s", file=sys.stderr)
        merger = api.Merger(dtax, "lca", with_score)
        cap = merger.bound(t1, t2)
        d1, d2, d_out, d_info = hip.malloc(len(t1) + 64), hip.malloc(len(t2) + 64), hip.malloc(cap + 64), hip.malloc(128)
        hip.h2d(d1, np.frombuffer(t1, dtype=np.uint8))
        hip.h2d(d2, np.frombuffer(t2, dtype=np.uint8))
        run = lambda: merger.merge_device(d1, len(t1), d2, len(t2), d_out, cap, d_info, final=True, stream=stream)
        run()                                                                 # warm-up: scratch allocation, code load
        assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        info = hip.d2h(d_info, 112).view(api.MERGE_INFO_DTYPE)[0]
        nb = int(info["text_bytes"])
        assert int(info["overflow"]) == 0 and int(info["stop_pair"]) == 2 ** 64 - 1 and int(info["count"]) == n
        total, passes = [], []
        for _ in range(args.reps):
            total.append(ev.timed(stream, run))
            ms = (C.c_float * len(PASSES))()
            assert L.kaiju_gpu_merge_pass_ms(merger._h, ms, len(PASSES)) == 0
            passes.append(list(ms))
        total.sort()
        med = total[len(total) // 2]
        r = {"bytes_in": len(t1) + len(t2), "bytes_out": nb, "classified_in_both": int(info["count_c12"]), "total_ms": {"median": med, "min": total[0], "max": total[-1]},
             "gb_per_s_in_and_out": (len(t1) + len(t2) + nb) / med / 1e6, "passes_ms": {p: float(np.median([x[k] for x in passes])) for k, p in enumerate(PASSES)}}
        text = hip.d2h(d_out, nb).tobytes()
        for d in (d1, d2, d_out, d_info):
            hip.free(d)
        merger.close()
        if os.path.exists(REF):
            f1, f2, fo = f"{W}/merge_in1.tsv", f"{W}/merge_in2.tsv", f"{W}/merge_ref.tsv"
            for path, t in ((f1, t1), (f2, t2)):
                with open(path, "wb") as f:
                    f.write(t)
            t0 = time.time()
            subprocess.run([REF, "-i", f1, "-j", f2, "-o", fo, "-c", "lca", "-t", nodes] + (["-s"] if with_score else []), check=True, stderr=subprocess.DEVNULL)
            r["reference_wall_s"] = time.time() - t0
            with open(fo, "rb") as f:
                r["equals_the_reference"] = f.read() == text
            ok = ok and r["equals_the_reference"]
            for path in (f1, f2, fo):
                os.remove(path)
        res[key] = r
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
