"""Per-pass times of the accession map and the converter on a synthetic input:  python tests/tools/convert_timing.py [--out FILE]

The input is made here (seeded): a heap-shaped tree of 2^17 - 1 nodes (the parent of id is id // 2), a map file of --keys
lines (default 1 000 000, about 33 MB: "ACC<n>\\tACC<n>.1\\t<taxon>\\t<n>", one line in 16 a duplicate, one in 16 a taxon that is
no node) and an nr-style text of --records records (default 200 000, about 75 MB: 1 to 8 entries a header, one header in 500
with 2000, sequences of 60 to 600 letters in lines of 60).  That runs in well under a minute on the device.  Reported: the
milliseconds per pass summed over the blocks (KAIJU_GPU_CONVERT_TIMES=1), GB/s of text over those sums and over the wall
time of the calls (uploads and downloads included), the load factor of the table and its probe-length histogram.

--dump DIR writes the input files instead, and --reference TOOL times the unmodified tool on them (on the host, one thread):
context for the device numbers, taken on whatever machine this runs on."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N_NODES = (1 << 17) - 1
BLOCK = 16 << 20


def make_inputs(keys, records, seed=7):
    rng = np.random.RandomState(seed)
    nodes = b"".join(b"%d\t|\t%d\t|\tno rank\t|\n" % (i, max(1, i // 2)) for i in range(1, N_NODES + 1))
    merged = b"".join(b"%d\t|\t%d\t|\n" % (N_NODES + 1 + i, 1 + i) for i in range(1000))
    acc = rng.randint(0, max(1, keys - keys // 16), size=keys)
    acc[:keys - keys // 16] = np.arange(keys - keys // 16)
    rng.shuffle(acc)
    taxa = rng.randint(2, N_NODES + 1, size=keys)
    taxa[rng.randint(0, keys, size=keys // 16)] = N_NODES + 5000
    amap = b"accession\taccession.version\ttaxid\tgi\n" + b"".join(b"ACC%d\tACC%d.1\t%d\t%d\n" % (a, a, t, k) for k, (a, t) in enumerate(zip(acc.tolist(), taxa.tolist())))
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    pool = letters[rng.randint(0, 20, size=1 << 20)].tobytes()
    out = []
    n_ent = rng.randint(1, 9, size=records)
    n_ent[rng.randint(0, records, size=max(1, records // 500))] = 2000
    lens = rng.randint(60, 601, size=records)
    starts = rng.randint(0, (1 << 20) - 700, size=records)
    ids = rng.randint(0, keys + keys // 8, size=int(n_ent.sum()))
    at = 0
    for r in range(records):
        k = int(n_ent[r])
        out.append(b">" + b"\x01".join(b"ACC%d.1 hypothetical protein [Some organism]" % i for i in ids[at:at + k].tolist()) + b"\n")
        at += k
        s = pool[int(starts[r]):int(starts[r]) + int(lens[r])]
        out.append(b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n")
    return nodes, merged, amap, b"".join(out)


def blocks(text, lines_only):
    at = 0
    while at < len(text):
        end = len(text)
        if end - at > BLOCK:
            end = (text.rfind(b"\n", at, at + BLOCK) if lines_only else text.rfind(b"\n>", at, at + BLOCK)) + 1
        yield text[at:end]
        at = end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1000000)
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--out")
    ap.add_argument("--dump")
    ap.add_argument("--reference")
    a = ap.parse_args()
    nodes, merged, amap, nr = make_inputs(a.keys, a.records)
    result = {"keys": a.keys, "records": a.records, "map_bytes": len(amap), "nr_bytes": len(nr), "block_bytes": BLOCK}
    d = a.dump or "/tmp/convert_timing_%d" % os.getpid()
    os.makedirs(d, exist_ok=True)
    for name, data in (("nodes.dmp", nodes), ("merged.dmp", merged), ("map.tsv", amap), ("nr.txt", nr)):
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    if a.reference:
        t0 = time.time()
        subprocess.run([os.path.abspath(a.reference), "-t", "nodes.dmp", "-m", "merged.dmp", "-g", "map.tsv", "-i", "nr.txt", "-o", "ref.faa"], cwd=d, check=True, stderr=subprocess.DEVNULL)
        result["reference_wall_s"] = round(time.time() - t0, 2)
        result["reference_out_bytes"] = os.path.getsize(os.path.join(d, "ref.faa"))
        with open(os.path.join(d, "ref.faa"), "rb") as f:
            result["reference_out_sha256"] = hashlib.sha256(f.read()).hexdigest()
    if not a.dump and not a.reference:
        device_run(os.path.join(d, "nodes.dmp"), amap, nr, result)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


def device_run(nodes_path, amap, nr, result):
    os.environ["KAIJU_GPU_CONVERT_TIMES"] = "1"
    from kaiju_amd import api
    host = api.Taxonomy(nodes_path)
    dtax = api.DeviceTaxonomy(host, 0)
    pairs = [(N_NODES + 1 + i, 1 + i) for i in range(1000)]
    m = api.AccMap(dtax, pairs)
    ms, t0 = np.zeros(api.ACCMAP_PASSES), time.time()
    for k, b in enumerate(blocks(amap, True)):
        m.add_text(b, first_block=k == 0)
        ms += m.pass_ms()
    wall = time.time() - t0
    st = m.info()
    result["map"] = {"pass_ms": dict(zip(("lines", "parse", "grow", "insert", "resolve"), (round(float(x), 3) for x in ms))), "wall_s": round(wall, 3),
                     "GBps_passes": round(len(amap) / 1e6 / max(ms.sum(), 1e-9), 2), "GBps_wall": round(len(amap) / 1e9 / wall, 2), "entries": int(st["entries"]),
                     "slots": int(st["slots"]), "load": round(int(st["entries"]) / int(st["slots"]), 3), "arena_bytes": int(st["arena_bytes"]),
                     "bytes_per_entry": round((int(st["arena_bytes"]) + 8 * int(st["slots"])) / max(1, int(st["entries"])), 1), "rehashes": int(st["rehashes"]),
                     "duplicates": int(st["duplicates"]), "lines_no_insert": int(st["lines_no_insert"]), "probe_hist": [int(x) for x in st["probe_hist"]]}
    conv = api.Converter(dtax, m)
    ms, t0, out_bytes, kept, entries, sha = np.zeros(api.CONVERT_PASSES), time.time(), 0, 0, 0, hashlib.sha256()
    for b in blocks(nr, False):
        text, info = conv.convert(b, out_cap=len(b) + len(b) // 4 + 4096)
        assert not int(info["overflow"])
        ms += conv.pass_ms()
        sha.update(text)
        out_bytes, kept, entries = out_bytes + len(text), kept + int(info["n_kept"]), entries + int(info["n_entries"])
    wall = time.time() - t0
    result["convert"] = {"pass_ms": dict(zip(("lines", "kinds", "entries", "decide", "lengths", "write", "finish"), (round(float(x), 3) for x in ms))), "wall_s": round(wall, 3),
                         "GBps_passes": round(len(nr) / 1e6 / max(ms.sum(), 1e-9), 2), "GBps_wall": round(len(nr) / 1e9 / wall, 2), "out_bytes": out_bytes, "kept": kept,
                         "entries": entries, "out_sha256": sha.hexdigest()}          # (equal to reference_out_sha256 of --reference: the same bytes)
    for x in (conv, m, dtax):
        x.close()


if __name__ == "__main__":
    main()
