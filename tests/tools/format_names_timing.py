"""What the column of kaiju-addTaxonNames costs on the benchmark workload, with HIP events (needs a GPU):

    python tests/tools/format_names_timing.py [--work DIR] [--reads 2000000] [--mode path] [--reps 7]

The database, index, taxonomy and reads are bench.py's (synth.make_db(680 001 proteins, seed 12345), synth.make_reads(seed 777),
150-bp single reads; --work is its work directory, an index found there is used).  Every node of the synthetic tree gets a
name.  One MEM step (kaiju_gpu_classify_batch_device_compact) is timed, then on its records the three-column passes
(kaiju_gpu_format_compact_device) and the passes with the column (kaiju_gpu_format_names_device), each `reps` times on
device-resident buffers; the outputs are compared on the host (every line: the three-column line, and for a classified read
the annotation of kaiju_taxon_names_annotation behind it).
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from kaiju_amd import api, mkfmi, synth  # noqa: E402
from test_gpu_parity import Hip  # noqa: E402


class Events:
    def __init__(self, hip):
        self.L = hip.L
        self.L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def timed(self, stream, launch):
        a, b = C.c_void_p(), C.c_void_p()
        assert self.L.hipEventCreate(C.byref(a)) == 0 and self.L.hipEventCreate(C.byref(b)) == 0
        assert self.L.hipEventRecord(a, C.c_void_p(stream)) == 0
        launch()
        assert self.L.hipEventRecord(b, C.c_void_p(stream)) == 0 and self.L.hipEventSynchronize(b) == 0
        ms = C.c_float()
        assert self.L.hipEventElapsedTime(C.byref(ms), a, b) == 0
        self.L.hipEventDestroy(a)
        self.L.hipEventDestroy(b)
        return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/kaiju_amd_bench")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--nseq", type=int, default=680_001)
    ap.add_argument("--mode", default="path")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    W, n, Lm = args.work, args.reads, 150
    os.makedirs(W, exist_ok=True)
    threads = min(16, os.cpu_count() or 1)
    lines, leaves = synth.make_taxonomy()
    db = synth.make_db(nseq=args.nseq, seed=12345, leaves=leaves)
    fmi, nodes, names_dmp = f"{W}/db_{args.nseq}.fmi", f"{W}/nodes.dmp", f"{W}/names.dmp"
    synth.write_nodes_dmp(nodes, lines)
    with open(names_dmp, "w") as f:
        for l in lines:
            tid, _, rank = [x.strip() for x in l.split("|")[:3]]
            f.write(f"{tid}\t|\tSynthetic {rank} {tid} of the benchmark tree\t|\t\t|\tscientific name\t|\n")
    if not os.path.exists(fmi):
        synth.write_fasta(db, f"{W}/db_{args.nseq}.faa")
        mkfmi.build_fmi(f"{W}/db_{args.nseq}.faa", fmi + ".tmp", threads=threads, exponent=3)
        os.replace(fmi + ".tmp", fmi)
    reads = synth.make_reads(db, n, seed=777, threads=threads)
    assert reads.shape == (n, Lm)
    off = np.arange(2 * n + 1, dtype=np.uint64) // 2 * np.uint64(Lm)
    off[1::2] = off[2::2]
    # the names of the reads as they lie in a FASTQ block: "@r<i>\n" one behind the other
    t0 = time.time()
    name_list = [b"@r%d\n" % i for i in range(n)]
    lens = np.fromiter((len(x) for x in name_list), dtype=np.int64, count=n)
    text1 = b"".join(name_list)
    spans = np.zeros(n, dtype=api.NAME_SPAN_DTYPE)
    spans["pos"] = np.concatenate([[0], np.cumsum(lens)[:-1]]) + 1
    spans["len"] = lens - 2
    print(f"workload ready ({time.time() - t0:.1f}s for the names)", file=sys.stderr)

    hip, index = Hip(), api.Index(fmi, device=0)
    ev = Events(hip)
    dtax = api.DeviceTaxonomy(api.Taxonomy(nodes), 0)
    tnames = api.TaxonNames(nodes, names_dmp, args.mode)
    dnames = api.DeviceTaxonNames(tnames, 0)
    clf = api.Classifier(index, api.default_params("mem"))
    clf.set_max_read_length(Lm)
    stream = clf.stream_handle()
    bound3 = int(api.lib().kaiju_gpu_format_bound(len(text1), n))
    bound4 = int(api.lib().kaiju_gpu_format_names_bound(len(text1), n, dnames._h))
    text_arr = np.frombuffer(text1 + b"\0" * 16, dtype=np.uint8)
    sizes = {"seqs": reads.nbytes, "off": off.nbytes, "hits": n * api.HIT_DTYPE.itemsize, "compact": 16 * n + 16, "text": len(text_arr), "spans": spans.nbytes + 8,
             "out3": bound3 + 64, "out4": bound4 + 64, "info": 64}
    d = {k: hip.malloc(v) for k, v in sizes.items()}
    for k, a in (("seqs", reads.reshape(-1)), ("off", off), ("text", text_arr), ("spans", spans)):
        hip.h2d(d[k], a)
    hip.memset(d["hits"], sizes["hits"])

    def mem_step():
        clf.classify_device_compact(dtax, d["seqs"], reads.nbytes, d["off"], n, d["hits"], d["compact"], paired=False, stream=0)

    def three():
        clf.format_compact_device(d["compact"], d["off"], n, d["text"], len(text1), d["spans"], d["out3"], bound3, d["info"], stream=0)

    def four():
        clf.format_names_device(d["compact"], d["off"], n, d["text"], len(text1), d["spans"], dnames, d["out4"], bound4, d["info"], stream=0)

    res = {"reads": n, "nseq": args.nseq, "mode": args.mode, "max_annotation": dnames.max_annotation}
    for key, fn in (("mem_step_ms", mem_step), ("three_column_ms", three), ("with_names_ms", four)):
        fn()                                            # warm-up (scratch allocation, code load)
        assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        ms = sorted(ev.timed(stream, fn) for _ in range(args.reps))
        res[key] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}
        info = hip.d2h(d["info"], 40)
        if key == "three_column_ms":
            fi = info[:24].view(api.FORMAT_INFO_DTYPE)[0]
            res["three_column_bytes"] = int(fi["text_bytes"])
            text3 = hip.d2h(d["out3"], int(fi["text_bytes"])).tobytes()
        if key == "with_names_ms":
            fi = info.view(api.FORMAT_NAMES_INFO_DTYPE)[0]
            res["with_names_bytes"] = int(fi["text_bytes"])
            res["n_classified"] = int(fi["n_classified"])
            res["n_unknown_taxon"], res["n_unnamed_taxon"] = int(fi["n_unknown_taxon"]), int(fi["n_unnamed_taxon"])
            text4 = hip.d2h(d["out4"], int(fi["text_bytes"])).tobytes()
    # every line with names is its three-column line, for a classified read followed by a tab and the annotation the host's
    # walk of the tree gives for its taxon
    l3, l4 = text3.split(b"\n"), text4.split(b"\n")
    assert len(l3) == len(l4) == n + 1
    memo, bad = {}, 0
    for a, b in zip(l3, l4):
        if a[:1] != b"C":
            bad += a != b
            continue
        t = a[a.rindex(b"\t") + 1:]
        if t not in memo:
            ann = tnames.annotation(int(t))
            memo[t] = b"" if ann is None else b"\t" + ann
        bad += b != a + memo[t]
    res["lines_that_differ_from_the_host_walk"] = bad
    res["distinct_taxa"] = len(memo)
    step = res["mem_step_ms"]["median"]
    res["share_of_mem_step"] = {"three_column": res["three_column_ms"]["median"] / step, "with_names": res["with_names_ms"]["median"] / step}
    print(json.dumps(res))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
