"""What the tally (kaiju_amd/csrc/tally.hip) costs (needs a GPU; tests/tools/tally_timing.sh runs the three steps):

    python tests/tools/tally_timing.py passes  [--work DIR] [--mib 1024] [--reps 5]
    python tests/tools/tally_timing.py kernels [--work DIR] [--mib 1024]           (under a kernel trace)
    python tests/tools/tally_timing.py cli     [--work DIR] [--mib 1024]

A synthetic three-column text of about `mib` MiB over a tree of 50 000 species (kaiju_amd/synth.py), every line 22 bytes
("C\\tr<9 digits>\\t<8 digits>\\n", the id zero-padded: the tool and the device read it by value; one line in ten "U"), in two
distributions of the ids: uniform over the species, and one species holding 90 % of the classified lines.

    passes   the events a tally created with KAIJU_GPU_TALLY_TIMES=1 records between its passes (lines, count, finish), on a
             device-resident text, for the three ways of counting (KAIJU_GPU_TALLY_COUNT unset, =wave, =lane): median, lowest
             and highest of `reps`.  Every way must give the entries of the first
    kernels  one annotator call (name mode) and one tally call per distribution on the same text, three times, for a kernel
             trace around the process: k_an_lines_count / k_an_top / k_an_lines_fill / k_an_len beside k_tl_*
    cli      kaiju_amd/bin/kaiju2table against oracle/_ref/kaiju2table (built by tests/golden/make_golden_table.py) on the
             skewed text as a file, -r species: wall seconds of three runs each, alternating; the two tables must be equal

Prints one JSON line."""
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
from kaiju_amd import api, build, synth  # noqa: E402
from test_gpu_parity import Hip  # noqa: E402

PASSES = ("lines", "count", "finish")
REF = os.path.join(ROOT, "oracle", "_ref", "kaiju2table")
LINE = 22


def make_text(n, leaves, skewed, seed=4711):
    """n lines of LINE bytes: a uint8 array"""
    rng = np.random.default_rng(seed)
    ids = leaves[rng.integers(0, len(leaves), n)]
    if skewed:
        ids = np.where(rng.random(n) < 0.9, leaves[len(leaves) // 3], ids)
    classified = rng.random(n) >= 0.1
    ids = np.where(classified, ids, 0)
    out = np.empty((n, LINE), dtype=np.uint8)
    out[:, 0] = np.where(classified, ord("C"), ord("U"))
    out[:, 1], out[:, 2], out[:, 12], out[:, 21] = 9, ord("r"), 9, 10
    k = np.arange(n, dtype=np.int64)
    for d in range(9):
        out[:, 11 - d] = 48 + (k // 10 ** d) % 10
    for d in range(8):
        out[:, 20 - d] = 48 + (ids // 10 ** d) % 10
    return out.reshape(-1)


def setup(args):
    os.makedirs(args.work, exist_ok=True)
    lines, leaves = synth.make_taxonomy(n_families=500)
    nodes, names = f"{args.work}/tally_nodes.dmp", f"{args.work}/tally_names.dmp"
    synth.write_nodes_dmp(nodes, lines)
    with open(names, "w") as f:
        for l in lines:
            tid, _, rank = [x.strip() for x in l.split("|")[:3]]
            f.write(f"{tid}\t|\tSynthetic {rank} {tid}\t|\t\t|\tscientific name\t|\n")
    return nodes, names, np.asarray(leaves, dtype=np.int64), args.mib * (1 << 20) // LINE


def entries_key(ent):
    return ent.tobytes()


def passes(args):
    nodes, names, leaves, n = setup(args)
    os.environ["KAIJU_GPU_TALLY_TIMES"] = "1"
    hip = Hip()
    host = api.TaxonNames(nodes, names)
    dev = api.DeviceTaxonNames(host, 0)
    stream = hip.stream()
    res = {"lines": n, "bytes": n * LINE, "reps": args.reps}
    ok = True
    for dist in ("uniform", "skewed"):
        t0 = time.time()
        text = make_text(n, leaves, dist == "skewed")
        print(f"{dist}: {text.nbytes} bytes made in {time.time() - t0:.1f}s", file=sys.stderr)
        d_text, d_info = hip.malloc(text.nbytes + 64), hip.malloc(64)
        hip.h2d(d_text, text)
        first = None
        r = {}
        for way in ("table", "wave", "lane"):
            os.environ.pop("KAIJU_GPU_TALLY_COUNT", None)
            if way != "table":
                os.environ["KAIJU_GPU_TALLY_COUNT"] = way
            t = api.Tally(dev)
            ms = []
            for rep in range(args.reps + 1):                         # the first one is the warm-up: scratch allocation, code load
                t.reset()
                t.add_device(d_text, text.nbytes, d_info, final=True, stream=stream)
                assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
                if rep:
                    ms.append(t.pass_ms())
            ent, tot = t.result()
            assert int(tot["n_total"]) == n and int(tot["n_bad_id"]) == 0 and int(tot["n_unknown_taxon"]) == 0
            first = entries_key(ent) if first is None else first
            ok = ok and entries_key(ent) == first
            ms = np.array(ms)
            r[way] = {p: {"median": float(np.median(ms[:, k])), "min": float(ms[:, k].min()), "max": float(ms[:, k].max())} for k, p in enumerate(PASSES)}
            r[way]["lines_and_count_gb_per_s"] = text.nbytes / float(np.median(ms[:, 0] + ms[:, 1])) / 1e6
            t.close()
        r["entries"] = len(ent)
        r["all_ways_agree"] = ok
        res[dist] = r
        hip.free(d_text)
        hip.free(d_info)
    print(json.dumps(res))
    return 0 if ok else 1


def kernels(args):
    nodes, names, leaves, n = setup(args)
    hip = Hip()
    host = api.TaxonNames(nodes, names)
    dev = api.DeviceTaxonNames(host, 0)
    an, t = api.Annotator(dev), api.Tally(dev)
    stream = hip.stream()
    for dist in ("uniform", "skewed"):
        text = make_text(n, leaves, dist == "skewed")
        cap = int(api.lib().kaiju_gpu_annotate_bound(text.nbytes, n + 1, dev._h))
        d_text, d_out, d_info = hip.malloc(text.nbytes + 64), hip.malloc(cap + 64), hip.malloc(64)
        hip.h2d(d_text, text)
        for _ in range(3):
            an.annotate_device(d_text, text.nbytes, d_out, cap, d_info, stream=stream)
            t.reset()
            t.add_device(d_text, text.nbytes, d_info, final=True, stream=stream)
            assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        for d in (d_text, d_out, d_info):
            hip.free(d)
    print(json.dumps({"lines": n, "bytes": n * LINE, "calls_per_distribution": 3}))
    return 0


def cli(args):
    nodes, names, leaves, n = setup(args)
    path, ours, theirs = f"{args.work}/tally_in.tsv", f"{args.work}/tally_ours.tsv", f"{args.work}/tally_ref.tsv"
    make_text(n, leaves, True).tofile(path)
    exe = build.build_table_cli()
    opts = ["-t", nodes, "-n", names, "-r", "species"]
    res = {"lines": n, "bytes": n * LINE, "ours_s": [], "reference_s": []}
    for _ in range(3):
        t0 = time.time()
        subprocess.run([exe] + opts + ["-o", ours, path], check=True, timeout=600)
        res["ours_s"].append(time.time() - t0)
        if os.path.exists(REF):
            t0 = time.time()
            subprocess.run([REF] + opts + ["-o", theirs, path], check=True, timeout=600, stderr=subprocess.DEVNULL)
            res["reference_s"].append(time.time() - t0)
    if os.path.exists(REF):
        with open(ours, "rb") as a, open(theirs, "rb") as b:
            res["equals_the_reference"] = a.read() == b.read()
    for p in (path, ours, theirs):
        if os.path.exists(p):
            os.remove(p)
    for k in ("ours_s", "reference_s"):
        if res[k]:
            res[k[:-2] + "_median_s"] = sorted(res[k])[1]
    print(json.dumps(res))
    return 0 if res.get("equals_the_reference", True) else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["passes", "kernels", "cli"])
    ap.add_argument("--work", default="/tmp/kaiju_amd_bench")
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.exit({"passes": passes, "kernels": kernels, "cli": cli}[a.step](a))
