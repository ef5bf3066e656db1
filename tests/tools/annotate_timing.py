"""What the stand-alone annotator (kaiju_amd/csrc/annotate.hip) costs on the benchmark workload, with HIP events (needs a GPU):

    python tests/tools/annotate_timing.py [--work DIR] [--reads 2000000] [--mode path] [--reps 7]

The workload is that of tests/tools/format_names_timing.py (bench.py's database, index, taxonomy and 2 M single 150-bp reads,
every node of the synthetic tree named).  One MEM step gives the records; the three-column passes write their text on the
device and kaiju_gpu_classify_batch_verbose_text gives the lines of kaiju -v of the same reads.  Timed on device-resident
buffers, alternating within every repetition so that none of them has the card to itself at another time than the others:

    column      the passes with the column on the records (kaiju_gpu_format_names_device)
    annotate    kaiju_gpu_annotate_text_device on the three-column text
    annotate_v  kaiju_gpu_annotate_text_device on the -v text

--variant LIB adds the same two legs through a second build of the library loaded into the same process (other kernels, the
same buffers): how a change of the write pass is measured against the library as built (DESIGN.md 3.12 has one such table).

The annotated three-column text must equal the text of the passes with the column byte for byte, a variant the library, and
every line of the annotated -v text its input line, for a classified read followed by a tab and the annotation of the
loader's own walk.  Prints one JSON line: per leg the median, the lowest and the highest of `reps` in ms, and GB/s of text written."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools")]
from kaiju_amd import api, mkfmi, synth  # noqa: E402
from format_names_timing import Events  # noqa: E402
from test_gpu_parity import Hip  # noqa: E402

class Ann:
    """an annotator of library L (raw C-ABI: a variant library is not the one kaiju_amd.api holds)"""

    def __init__(self, L, nodes, names_dmp, mode):
        self.L = L
        m = {"name": 0, "path": 1}[mode]
        L.kaiju_taxon_names_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_void_p]
        L.kaiju_gpu_taxon_names_upload.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.kaiju_gpu_annotator_create.argtypes = [C.c_void_p, C.c_void_p]
        L.kaiju_gpu_annotate_text_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.kaiju_gpu_annotate_bound.restype = C.c_uint64
        L.kaiju_gpu_annotate_bound.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
        self.host, self.dev, self.an = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert L.kaiju_taxon_names_load(nodes.encode(), names_dmp.encode(), m, None, C.byref(self.host)) == 0
        assert L.kaiju_gpu_taxon_names_upload(self.host, 0, C.byref(self.dev)) == 0
        assert L.kaiju_gpu_annotator_create(self.dev, C.byref(self.an)) == 0

    def bound(self, nbytes, n_lines):
        return int(self.L.kaiju_gpu_annotate_bound(nbytes, n_lines, self.dev))

    def run(self, d_text, nbytes, d_out, cap, d_info, stream):
        assert self.L.kaiju_gpu_annotate_text_device(self.an, d_text, nbytes, 0, d_out, cap, d_info, stream) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/kaiju_amd_bench")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--nseq", type=int, default=680_001)
    ap.add_argument("--mode", default="path")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--variant", default=None, help="a second libkaiju_gpu.so to time beside the one in use")
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
    name_list = [b"@r%d\n" % i for i in range(n)]
    lens = np.fromiter((len(x) for x in name_list), dtype=np.int64, count=n)
    text1 = b"".join(name_list)
    spans = np.zeros(n, dtype=api.NAME_SPAN_DTYPE)
    spans["pos"] = np.concatenate([[0], np.cumsum(lens)[:-1]]) + 1
    spans["len"] = lens - 2

    hip, index = Hip(), api.Index(fmi, device=0)
    ev = Events(hip)
    tax = api.Taxonomy(nodes)
    dtax = api.DeviceTaxonomy(tax, 0)
    tnames = api.TaxonNames(nodes, names_dmp, args.mode)
    dnames = api.DeviceTaxonNames(tnames, 0)
    clf = api.Classifier(index, api.default_params("mem"))
    clf.set_max_read_length(Lm)
    stream = clf.stream_handle()
    t0 = time.time()
    index.upload_accessions()
    vtext, vinfo = clf.classify_verbose_text(dtax, reads.reshape(-1), off, text1, spans)
    print(f"-v text: {len(vtext)} bytes in {time.time() - t0:.1f}s", file=sys.stderr)
    assert vtext.count(b"\n") == n

    ann = Ann(api.lib(), nodes, names_dmp, args.mode)
    other = Ann(C.CDLL(os.path.abspath(args.variant)), nodes, names_dmp, args.mode) if args.variant else None
    bound3 = int(api.lib().kaiju_gpu_format_bound(len(text1), n))
    bound4 = int(api.lib().kaiju_gpu_format_names_bound(len(text1), n, dnames._h))
    boundv = ann.bound(len(vtext), n + 1)
    text_arr = np.frombuffer(text1 + b"\0" * 16, dtype=np.uint8)
    sizes = {"seqs": reads.nbytes, "off": off.nbytes, "hits": n * api.HIT_DTYPE.itemsize, "compact": 16 * n + 16, "text": len(text_arr), "spans": spans.nbytes + 8,
             "out3": bound3 + 64, "out4": bound4 + 64, "ann3": bound4 + 64, "vtext": len(vtext) + 64, "annv": boundv + 64, "info": 64}
    d = {k: hip.malloc(v) for k, v in sizes.items()}
    for k, a in (("seqs", reads.reshape(-1)), ("off", off), ("text", text_arr), ("spans", spans), ("vtext", np.frombuffer(vtext, dtype=np.uint8))):
        hip.h2d(d[k], a)
    hip.memset(d["hits"], sizes["hits"])
    clf.classify_device_compact(dtax, d["seqs"], reads.nbytes, d["off"], n, d["hits"], d["compact"], paired=False, stream=0)
    clf.format_compact_device(d["compact"], d["off"], n, d["text"], len(text1), d["spans"], d["out3"], bound3, d["info"], stream=0)
    assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
    bytes3 = int(hip.d2h(d["info"], 24).view(api.FORMAT_INFO_DTYPE)[0]["text_bytes"])

    legs = {
        "column": lambda: clf.format_names_device(d["compact"], d["off"], n, d["text"], len(text1), d["spans"], dnames, d["out4"], bound4, d["info"], stream=0),
        "annotate": lambda: ann.run(d["out3"], bytes3, d["ann3"], bound4, d["info"], stream),
        "annotate_v": lambda: ann.run(d["vtext"], len(vtext), d["annv"], boundv, d["info"], stream),
    }
    if other:
        legs["variant"] = lambda: other.run(d["out3"], bytes3, d["ann3"], bound4, d["info"], stream)
        legs["variant_v"] = lambda: other.run(d["vtext"], len(vtext), d["annv"], boundv, d["info"], stream)
    res = {"reads": n, "nseq": args.nseq, "mode": args.mode, "max_annotation": dnames.max_annotation, "three_column_bytes": bytes3, "verbose_bytes": len(vtext)}
    texts, ms = {}, {k: [] for k in legs}
    for k, fn in legs.items():                                  # warm-up (scratch allocation, code load), and the outputs
        fn()
        assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        info = hip.d2h(d["info"], 48)
        nb = int(info[:8].view("<u8")[0])
        res[k + "_bytes"] = nb
        texts[k] = hip.d2h(d["out4" if k == "column" else "annv" if k.endswith("_v") else "ann3"], nb).tobytes()
    for _ in range(args.reps):
        for k, fn in legs.items():
            ms[k].append(ev.timed(stream, fn))
    for k, v in ms.items():
        v = sorted(v)
        res[k + "_ms"] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "gb_per_s": res[k + "_bytes"] / v[len(v) // 2] / 1e6}
    res["annotated_three_column_equals_the_passes_with_the_column"] = texts["annotate"] == texts["column"]
    res["variants_agree"] = not other or (texts["annotate"] == texts["variant"] and texts["annotate_v"] == texts["variant_v"])
    memo, bad = {}, 0
    lv, la = vtext.split(b"\n"), texts["annotate_v"].split(b"\n")
    bad += len(lv) != len(la)
    for a, b in zip(lv, la):
        if a[:1] != b"C":
            bad += a != b
            continue
        t = a.split(b"\t")[2]
        if t not in memo:
            ann = tnames.annotation(int(t))
            memo[t] = b"" if ann is None else b"\t" + ann
        bad += b != a + memo[t]
    res["verbose_lines_that_differ_from_the_host_walk"] = bad
    print(json.dumps(res))
    return 0 if res["variants_agree"] and res["annotated_three_column_equals_the_passes_with_the_column"] and not bad else 1


if __name__ == "__main__":
    sys.exit(main())
