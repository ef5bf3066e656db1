"""What the Krona text (kaiju_amd/csrc/krona.hip) costs (needs a GPU; tests/tools/krona_timing.sh runs the two steps):

    python tests/tools/krona_timing.py passes [--work DIR] [--mib 1024] [--reps 5]
    python tests/tools/krona_timing.py cli    [--work DIR] [--mib 1024]

The text and the tree are those of tests/tools/tally_timing.py: about `mib` MiB of 22-byte lines over a tree of 50 000
species, one species holding 90 % of the classified lines, one line in ten "U".

    passes   the text is counted once by a tally (device-resident); then the events a Krona object created with
             KAIJU_GPU_KRONA_TIMES=1 records between its passes (select, compact, len and offsets, write, finish), without a
             list and with -l superkingdom,phylum,genus,species: median, lowest and highest of `reps` calls of
             kaiju_gpu_krona_text_device, and the same for the whole call from event to event.  Every call must give the
             bytes of the first
    cli      kaiju_amd/bin/kaiju2krona -u against oracle/_ref/kaiju2krona -u (built by tests/golden/make_golden_krona.py) on the
             text as a file: wall seconds of three runs each, alternating, the page cache warm; the sorted lines must be equal

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
from kaiju_amd import api, build  # noqa: E402
from tally_timing import LINE, make_text, setup  # noqa: E402
from test_gpu_parity import Hip  # noqa: E402

PASSES = ("select", "compact", "len_offsets", "write", "finish")
REF = os.path.join(ROOT, "oracle", "_ref", "kaiju2krona")
LISTS = {"no_list": None, "four_ranks": "superkingdom,phylum,genus,species"}


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def passes(args):
    nodes, names, leaves, n = setup(args)
    os.environ["KAIJU_GPU_KRONA_TIMES"] = "1"
    hip = Hip()
    host = api.TaxonNames(nodes, names)
    dev = api.DeviceTaxonNames(host, 0)
    stream = hip.stream()
    text = make_text(n, leaves, True)
    d_text, d_info = hip.malloc(text.nbytes + 64), hip.malloc(64)
    hip.h2d(d_text, text)
    tally = api.Tally(dev)
    tally.add_device(d_text, text.nbytes, d_info, final=True, stream=stream)
    assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
    ent, tot = tally.result()
    res = {"lines": n, "bytes": n * LINE, "reps": args.reps, "nodes": host.count(), "taxa_with_reads": int(np.count_nonzero(ent["direct"]))}
    ok = True
    for label, ranks in LISTS.items():
        k = api.Krona(dev, ranks)
        size = int(k.text(tally, unclassified=True, out_cap=0)[1]["text_bytes"])
        d_out = hip.malloc(size + 64)
        first, ms = None, []
        for rep in range(args.reps + 1):                             # the first one is the warm-up: code load
            hip.ck(hip.L.hipMemset(C.c_void_p(d_out), 0, C.c_size_t(size + 64)))
            k.text_device(tally, d_out, size, d_info, unclassified=True, stream=stream)
            assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
            out = bytes(hip.d2h(d_out, size))
            first = out if first is None else first
            ok = ok and out == first and out.endswith(b"\tUnclassified\n")
            if rep:
                ms.append(k.pass_ms())
        ms = np.array(ms)
        r = {p: spread(ms[:, i]) for i, p in enumerate(PASSES)}
        r["all_passes"] = spread(ms.sum(axis=1))
        r["text_bytes"], r["text_lines"] = size, first.count(b"\n")
        res[label] = r
        hip.free(d_out)
        k.close()
    res["every_call_gave_the_same_bytes"] = ok
    print(json.dumps(res))
    return 0 if ok else 1


def cli(args):
    nodes, names, leaves, n = setup(args)
    path, ours, theirs = f"{args.work}/krona_in.tsv", f"{args.work}/krona_ours.txt", f"{args.work}/krona_ref.txt"
    make_text(n, leaves, True).tofile(path)
    exe = build.build_krona_cli()
    opts = ["-t", nodes, "-n", names, "-u", "-i", path]
    res = {"lines": n, "bytes": n * LINE, "ours_s": [], "reference_s": []}
    with open(path, "rb") as f:                                       # the page cache warm for both
        while f.read(1 << 24):
            pass
    for _ in range(3):
        t0 = time.time()
        subprocess.run([exe] + opts + ["-o", ours], check=True, timeout=600)
        res["ours_s"].append(time.time() - t0)
        if os.path.exists(REF):
            t0 = time.time()
            subprocess.run([REF] + opts + ["-o", theirs], check=True, timeout=600, stderr=subprocess.DEVNULL)
            res["reference_s"].append(time.time() - t0)
    if os.path.exists(REF):
        with open(ours, "rb") as a, open(theirs, "rb") as b:
            x, y = a.read(), b.read()
            res["sorted_lines_equal_the_reference"] = sorted(x.split(b"\n")) == sorted(y.split(b"\n"))
            res["text_bytes"] = len(x)
    for p in (path, ours, theirs):
        if os.path.exists(p):
            os.remove(p)
    for key in ("ours_s", "reference_s"):
        if res[key]:
            res[key[:-2] + "_median_s"] = sorted(res[key])[1]
    print(json.dumps(res))
    return 0 if res.get("sorted_lines_equal_the_reference", True) else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["passes", "cli"])
    ap.add_argument("--work", default="/tmp/kaiju_amd_bench")
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.exit({"passes": passes, "cli": cli}[a.step](a))
