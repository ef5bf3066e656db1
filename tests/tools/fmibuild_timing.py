"""The stages behind the suffix sort, host against device: whole builds of the benchmark database or the hard one
with stages = host and stages = device alternating, three runs each, a fresh process per build, KAIJU_GPU_LOAD_TIMES=1, 16 host
threads; every pair of files is compared.  The builder's marks go to <out>/<database>_<mode>_<run>.err, the figures of every run
(marks, HIP events) to <out>/<database>.json.

    python tests/tools/fmibuild_timing.py {bench|hard} [--out DIR] [--host-lib LIB]

--host-lib: another build of libkaiju_mkfmi_gpu.so (an earlier commit's, say) whose kaiju_build_fmi_device stands for the host
stages; the default is this tree's library with stages = host."""
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

POST = ("BWT of the file", "sequence ranks", "BWT", "suffix array samples", "FMI checkpoints", "recode")
EVENTS = ("ms_bwt", "ms_ranks", "ms_samples", "ms_checkpoints", "ms_recode", "ms_download")


def child(lib, mode, faa, out):
    """one build in this process: one JSON line on stdout, the marks on stderr"""
    L = C.CDLL(lib)
    L.kaiju_build_fmi_error.restype = C.c_char_p
    res = {"mode": mode}
    t0 = time.perf_counter()
    if not hasattr(L, "kaiju_build_fmi_device_ex"):
        L.kaiju_build_fmi_device.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        rc = L.kaiju_build_fmi_device(faa.encode(), out.encode(), 16, 3, 0)
    else:
        st = mkfmi.FmiBuildStats()
        L.kaiju_build_fmi_device_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_int,
                                                C.POINTER(mkfmi.FmiBuildStats)]
        rc = L.kaiju_build_fmi_device_ex(faa.encode(), out.encode(), 16, 3, 1, None, 0, 0, mkfmi.STAGES[mode], C.byref(st))
        res["stats"] = mkfmi._stats_dict(st)
    res["wall_s"], res["rc"] = time.perf_counter() - t0, rc
    if rc != 0:
        res["error"] = L.kaiju_build_fmi_error().decode()
    print(json.dumps(res))
    return 0 if rc == 0 else 1


def med(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:.3f} ({v[0]:.3f} .. {v[-1]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("database", choices=("bench", "hard"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmibuild_stages"))
    ap.add_argument("--host-lib", default=None)
    ap.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    os.makedirs(args.out, exist_ok=True)
    own = kbuild.build_mkfmi_gpu()
    libs = {"host": args.host_lib or own, "device": own}
    W = tempfile.mkdtemp(prefix="fmibuild_timing_")
    try:
        _, leaves = synth.make_taxonomy()
        db = synth.make_db_hard(nseq=200001, seed=4321, leaves=leaves) if args.database == "hard" else synth.make_db(nseq=680001, seed=12345, leaves=leaves)
        faa = os.path.join(W, "db.faa")
        synth.write_fasta(db, faa)
        print("database", args.database, db.nseq, "sequences", db.total_aa, "letters", flush=True)
        runs = []
        for i in range(3):
            for mode in ("host", "device"):
                out = os.path.join(W, f"{mode}.fmi")
                if os.path.exists(out):
                    os.remove(out)
                r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), args.database, "--child", libs[mode], mode, faa, out],
                                   cwd=ROOT, env=dict(os.environ, KAIJU_GPU_LOAD_TIMES="1"), capture_output=True, text=True)
                with open(os.path.join(args.out, f"{args.database}_{mode}_{i}.err"), "w") as f:
                    f.write(r.stderr)
                if r.returncode != 0:                  # nothing more is started on the GPU
                    print(mode, i, "failed with", r.returncode, r.stdout[-500:], r.stderr[-2000:])
                    return 1
                res = json.loads(r.stdout.strip().splitlines()[-1])
                res["marks"] = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[kaiju mkfmi\] (.{34}) +([0-9.]+) s", r.stderr)}
                res["run"] = i
                runs.append(res)
            if not filecmp.cmp(os.path.join(W, "host.fmi"), os.path.join(W, "device.fmi"), shallow=False):
                print("run", i, ": the two files differ")
                return 2
        with open(os.path.join(args.out, f"{args.database}.json"), "w") as f:
            json.dump({"database": args.database, "nseq": int(db.nseq), "letters": int(db.total_aa), "runs": runs}, f, indent=1)
        host, dev = [r for r in runs if r["mode"] == "host"], [r for r in runs if r["mode"] == "device"]
        print("stages on the host, sum of the marks, s:    ", med([sum(r["marks"][k] for k in POST) for r in host]))
        print("stages on the device, the mark, s:          ", med([r["marks"]["device stages + download"] for r in dev]))
        print("stages on the device, HIP events, ms:       ", med([sum(r["stats"][k] for k in EVENTS) for r in dev]))
        for k in EVENTS:
            print(f"  {k:<16}", med([r["stats"][k] for r in dev]))
        print("whole build, host stages, sum of marks, s:  ", med([sum(r["marks"].values()) for r in host]))
        print("whole build, device stages, sum of marks, s:", med([sum(r["marks"].values()) for r in dev]))
        return 0
    finally:
        shutil.rmtree(W, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
