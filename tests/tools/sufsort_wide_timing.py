"""The wide (64-bit) device suffix sort against the narrow one and against the host sort.  Whole builds with
KAIJU_GPU_LOAD_TIMES=1 and 16 host threads, a fresh process per build under a time limit of its own; a step that fails ends the
script, nothing more is started on the GPU.  The builder's marks go to <out>/<name>.err as they are written, the figures of
every run to <out>/<what>.json.

    python tests/tools/sufsort_wide_timing.py overhead [--out DIR] [--host-lib LIB] [--trace]
    python tests/tools/sufsort_wide_timing.py full [--out DIR] [--work DIR] [--nseq N]

overhead: the benchmark database (synth.make_db, 680 001 proteins), three runs each, alternating: the narrow sort - --host-lib,
another build of libkaiju_mkfmi_gpu.so (the parent commit's, say), default this tree's - against this tree's wide sort
(KAIJU_MKFMI_FORCE64=1 KAIJU_MKFMI_DEVICE_WIDE=1); every pair of files is compared.
full: the database of `bench.py --nseq 15500001` (tests/tools/gen_db.c, about 4.34 G letters), once the host build and once the
device build with the host stages, one after the other; the two files are compared."""
import argparse
import ctypes as C
import filecmp
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from kaiju_amd import build as kbuild, mkfmi, synth  # noqa: E402

WIDE_ENV = {"KAIJU_MKFMI_FORCE64": "1", "KAIJU_MKFMI_DEVICE_WIDE": "1"}


def child(lib, mode, faa, out):
    """one build in this process: one JSON line on stdout, the marks on stderr.  mode: host, or anything else for device 0"""
    L = C.CDLL(lib)
    L.kaiju_build_fmi_error.restype = C.c_char_p
    res = {"mode": mode}
    t0 = time.perf_counter()
    if mode == "host":
        L.kaiju_build_fmi.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        rc = L.kaiju_build_fmi(faa.encode(), out.encode(), 16, 3)
    else:
        L.kaiju_build_fmi_device.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        rc = L.kaiju_build_fmi_device(faa.encode(), out.encode(), 16, 3, 0)
    res["wall_s"], res["rc"] = time.perf_counter() - t0, rc
    if rc != 0:
        res["error"] = L.kaiju_build_fmi_error().decode()
    print(json.dumps(res))
    return 0 if rc == 0 else 1


def one_build(args, name, lib, mode, faa, out, limit, env=None, prefix=()):
    """a fresh process for one build (prefix: a profiler's command line in front of it); None if it failed"""
    if os.path.exists(out):
        os.remove(out)
    errfile = os.path.join(args.out, name + ".err")
    with open(errfile, "w") as ef:
        r = subprocess.run(["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), args.what, "--child", lib, mode, faa, out],
                           cwd=ROOT, env=dict(os.environ, KAIJU_GPU_LOAD_TIMES="1", **(env or {})), stdout=subprocess.PIPE, stderr=ef, text=True)
    err = open(errfile).read()
    if r.returncode != 0:
        print(name, "failed with", r.returncode, r.stdout[-500:], err[-2000:], flush=True)
        return None
    res = json.loads(r.stdout.strip().splitlines()[-1])
    res["name"] = name
    res["marks"] = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[kaiju mkfmi\] (.{34}) +([0-9.]+) s", err)}
    m = re.search(r"on device \d+: ([0-9.]+) ms, (\d+) rounds, active((?: \d+)*)", err)
    if m:
        res["ms_sort"], res["rounds"], res["active"] = float(m.group(1)), int(m.group(2)), [int(a) for a in m.group(3).split()]
    m = re.search(r"wide suffix sort: needs (\d+) bytes of device memory \(([0-9.]+) per symbol, (\d+) of them temporary storage\), (\d+) are free", err)
    if m:
        res["wide"] = {"need_bytes": int(m.group(1)), "bytes_per_symbol": float(m.group(2)), "temp_bytes": int(m.group(3)), "free_bytes": int(m.group(4))}
    print(name, "suffix sort", res["marks"].get("suffix sort"), "s", {k: res[k] for k in ("ms_sort", "rounds", "wide") if k in res}, flush=True)
    return res


def med(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:.3f} ({v[0]:.3f} .. {v[-1]:.3f})"


def overhead(args, W):
    own = kbuild.build_mkfmi_gpu()
    _, leaves = synth.make_taxonomy()
    db = synth.make_db(nseq=680001, seed=12345, leaves=leaves)
    faa = os.path.join(W, "db.faa")
    synth.write_fasta(db, faa)
    print("database bench", db.nseq, "sequences", db.total_aa, "letters", flush=True)
    runs = []
    for i in range(3):
        for mode, lib, env in (("narrow", args.host_lib or own, None), ("wide", own, WIDE_ENV)):
            res = one_build(args, f"overhead_{mode}_{i}", lib, mode, faa, os.path.join(W, mode + ".fmi"), 150, env)
            if res is None:
                return 1
            res["run"] = i
            runs.append(res)
        if not filecmp.cmp(os.path.join(W, "narrow.fmi"), os.path.join(W, "wide.fmi"), shallow=False):
            print("run", i, ": the two files differ")
            return 2
    if any("wide" not in r for r in runs if r["mode"] == "wide") or any("wide" in r for r in runs if r["mode"] == "narrow"):
        print("the wide sort did not run where it was asked for, or ran where it was not")
        return 3
    with open(os.path.join(args.out, "overhead.json"), "w") as f:
        json.dump({"database": "bench", "nseq": int(db.nseq), "letters": int(db.total_aa), "runs": runs}, f, indent=1)
    nar, wid = [r for r in runs if r["mode"] == "narrow"], [r for r in runs if r["mode"] == "wide"]
    print("narrow, the mark \"suffix sort\", s:", med([r["marks"]["suffix sort"] for r in nar]))
    print("wide,   the mark \"suffix sort\", s:", med([r["marks"]["suffix sort"] for r in wid]))
    print("narrow, HIP events, ms:           ", med([r["ms_sort"] for r in nar]))
    print("wide,   HIP events, ms:           ", med([r["ms_sort"] for r in wid]))
    print("wide / narrow, medians of the HIP events: %.2f" % (sorted(r["ms_sort"] for r in wid)[1] / sorted(r["ms_sort"] for r in nar)[1]))
    print("wide: bytes per symbol", wid[0]["wide"]["bytes_per_symbol"], "rounds", wid[0]["rounds"], "active", wid[0]["active"])
    if args.trace:                                         # one more wide build under a kernel trace: which pass takes the time
        tdir = os.path.join(args.out, "overhead_wide_trace")
        prefix = ("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "-o", "wide", "--")
        if one_build(args, "overhead_wide_trace", own, "wide", faa, os.path.join(W, "wide.fmi"), 300, WIDE_ENV, prefix) is None:
            return 1
    return 0


def full(args, W):
    host_lib, own = kbuild.build_mkfmi(), kbuild.build_mkfmi_gpu()
    base = os.path.join(W, f"db_{args.nseq}")
    exe = os.path.join(tempfile.gettempdir(), f"kaiju_gen_db_{os.getpid()}")
    subprocess.run(["gcc", "-O2", "-fopenmp", "-o", exe, os.path.join(ROOT, "tests", "tools", "gen_db.c"), "-lm"], check=True)
    t0 = time.perf_counter()
    subprocess.run(["timeout", "-k", "10", "180", exe, str(args.nseq), "20260926", base + ".faa", base + ".codes", base + ".offsets", base + ".taxids"], check=True)
    os.remove(exe)
    for ext in (".codes", ".offsets", ".taxids"):          # (what bench.py reads its reads from: not needed here)
        os.remove(base + ext)
    print("database", args.nseq, "sequences,", os.path.getsize(base + ".faa"), "bytes of FASTA, %.1f s" % (time.perf_counter() - t0), flush=True)
    # the host sort of 4.35 G suffixes took 4.5 minutes on 14 cores; reading, the host stages and writing about
    # two more: nine minutes for the host build, six for the device build, whose sort is the smaller part
    runs = []
    for mode, lib, limit in (("host", host_lib, 540), ("device", own, 360)):
        res = one_build(args, f"full_{mode}", lib, mode, base + ".faa", os.path.join(W, mode + ".fmi"), limit)
        if res is None:
            return 1
        runs.append(res)
    same = subprocess.run(["cmp", os.path.join(W, "host.fmi"), os.path.join(W, "device.fmi")]).returncode == 0
    with open(os.path.join(args.out, "full.json"), "w") as f:
        json.dump({"nseq": args.nseq, "faa_bytes": os.path.getsize(base + ".faa"), "fmi_bytes": os.path.getsize(os.path.join(W, "host.fmi")),
                   "files_equal": same, "runs": runs}, f, indent=1)
    print("files equal:", same)
    if not same:
        return 2
    host, dev = runs
    print("host:   bucket counts + bucket fill + suffix sort, s: %.2f" % sum(host["marks"].get(k, 0.0) for k in ("bucket counts", "bucket fill", "suffix sort")))
    print("device: the mark \"suffix sort\", s: %.2f; HIP events %.1f ms; rounds %d; active %s" % (dev["marks"]["suffix sort"], dev["ms_sort"], dev["rounds"], dev["active"]))
    print("device: the size check compared", dev.get("wide"))
    return 0 if "wide" in dev else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("overhead", "full"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sufsort_wide"))
    ap.add_argument("--host-lib", default=None)
    ap.add_argument("--work", default=None, help="where the database and the indexes are written (full: about 25 GB); default a temporary directory")
    ap.add_argument("--nseq", type=int, default=15500001)
    ap.add_argument("--trace", action="store_true", help="overhead: one more wide build under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    args.out = os.path.abspath(args.out)
    args.host_lib = os.path.abspath(args.host_lib) if args.host_lib else None
    os.makedirs(args.out, exist_ok=True)
    W = tempfile.mkdtemp(prefix="sufsort_wide_timing_", dir=args.work)
    try:
        return overhead(args, W) if args.what == "overhead" else full(args, W)
    finally:
        shutil.rmtree(W, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
