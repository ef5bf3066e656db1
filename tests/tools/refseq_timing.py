"""Per-pass times of the accession map and the converter under the rules of kaiju-convertRefSeq, on a synthetic input:
    python tests/tools/refseq_timing.py [--out FILE]

The sibling of tests/tools/convert_timing.py, whose tree, block size and block cutter it uses.  The input is made here
(seeded): a two-column map file of --keys lines (default 1 000 000: "WP_<n>.1\\t<taxon>", one line in 16 an NP_ or XP_ line, one in
16 a taxon that merged.dmp maps to a node - its key loses a byte -, one in 16 a taxon that is no node, one in 16 a duplicate)
and a RefSeq-shaped text of --records records (default 200 000: one accession a header, "MULTISPECIES: ..." descriptions, one
accession in 9 not in the map, sequences of 60 to 600 letters in lines of 60, so that about 85 % of the bytes are sequence
lines).  Reported: the milliseconds per pass summed over the 16 MiB blocks (KAIJU_GPU_CONVERT_TIMES=1) for the map and for
--reps conversions (the first is the warm-up), the SHA-256 of the output, and the `entries` pass - k_cv_first - beside that of
an NR-rules converter - k_cv_entries - over the same text with a four-column map of the same accessions: the outputs differ,
the pass is comparable.

--dump DIR writes the input files instead, and --reference TOOL times the unmodified tool on them (on the host, one thread)
and prints the SHA-256 of its file: context for the device numbers, taken on whatever machine this runs on."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convert_timing as ct                                   # noqa: E402  (puts the repository root on sys.path)

N_NODES, N_MERGED = ct.N_NODES, 1000


def make_inputs(keys, records, seed=11):
    rng = np.random.RandomState(seed)
    nodes = b"".join(b"%d\t|\t%d\t|\tno rank\t|\n" % (i, max(1, i // 2)) for i in range(1, N_NODES + 1))
    merged = b"".join(b"%d\t|\t%d\t|\n" % (N_NODES + 1 + i, 2 + i) for i in range(N_MERGED))
    acc = rng.randint(0, max(1, keys - keys // 16), size=keys)
    acc[:keys - keys // 16] = np.arange(keys - keys // 16)
    rng.shuffle(acc)
    taxa = rng.randint(2, N_NODES + 1, size=keys)
    taxa[rng.randint(0, keys, size=keys // 16)] = N_NODES + 5000                                   # no node, not merged
    where = rng.randint(0, keys, size=keys // 16)
    taxa[where] = N_NODES + 1 + rng.randint(0, N_MERGED, size=len(where))                          # merged to a node
    prefix = np.zeros(keys, dtype=np.int64)
    prefix[rng.randint(0, keys, size=keys // 16)] = rng.randint(1, 3, size=keys // 16)
    names = (b"WP_", b"NP_", b"XP_")
    rows = list(zip(prefix.tolist(), acc.tolist(), taxa.tolist()))
    amap = b"accession.version\ttaxid\n" + b"".join(b"%s%09d.1\t%d\n" % (names[p], a, t) for p, a, t in rows)
    amap4 = b"accession\taccession.version\ttaxid\tgi\n" + b"".join(b"%s%09d\t%s%09d.1\t%d\t%d\n" % (names[p], a, names[p], a, t, k) for k, (p, a, t) in enumerate(rows))
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    pool = letters[rng.randint(0, 20, size=1 << 20)].tobytes()
    lens = rng.randint(60, 601, size=records)
    starts = rng.randint(0, (1 << 20) - 700, size=records)
    ids = rng.randint(0, keys + keys // 8, size=records)
    out = []
    for r in range(records):
        out.append(b">WP_%09d.1 MULTISPECIES: hypothetical protein [Some organism]\n" % int(ids[r]))
        s = pool[int(starts[r]):int(starts[r]) + int(lens[r])]
        out.append(b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n")
    return nodes, merged, amap, amap4, b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1000000)
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--dump")
    ap.add_argument("--reference")
    a = ap.parse_args()
    nodes, merged, amap, amap4, faa = make_inputs(a.keys, a.records)
    headers = faa.count(b"\n>") + 1
    result = {"keys": a.keys, "records": a.records, "map_bytes": len(amap), "text_bytes": len(faa), "block_bytes": ct.BLOCK,
              "header_share": round((len(faa) - sum(len(l) + 1 for l in faa.split(b"\n") if l[:1] != b">")) / len(faa), 3), "headers": headers}
    d = a.dump or "/tmp/refseq_timing_%d" % os.getpid()
    os.makedirs(d, exist_ok=True)
    for name, data in (("nodes.dmp", nodes), ("merged.dmp", merged), ("map.tsv", amap), ("faa.txt", faa)):
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    if a.reference:
        t0 = time.time()
        with open(os.path.join(d, "faa.txt"), "rb") as f:
            subprocess.run([os.path.abspath(a.reference), "-t", "nodes.dmp", "-m", "merged.dmp", "-g", "map.tsv", "-o", "ref.faa"], cwd=d, check=True, stdin=f, stderr=subprocess.DEVNULL)
        result["reference_wall_s"] = round(time.time() - t0, 2)
        result["reference_out_bytes"] = os.path.getsize(os.path.join(d, "ref.faa"))
        with open(os.path.join(d, "ref.faa"), "rb") as f:
            result["reference_out_sha256"] = hashlib.sha256(f.read()).hexdigest()
    if not a.dump and not a.reference:
        device_run(os.path.join(d, "nodes.dmp"), amap, amap4, faa, a.reps, result)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


def convert_all(conv, api, faa):
    """one conversion of the whole text: (milliseconds per pass, wall seconds, sha256, info sums)"""
    ms, t0, sha, sums = np.zeros(api.CONVERT_PASSES), time.time(), hashlib.sha256(), {"out_bytes": 0, "kept": 0, "entries": 0, "hits": 0}
    for b in ct.blocks(faa, False):
        text, info = conv.convert(b, out_cap=len(b) + len(b) // 4 + 4096)
        assert not int(info["overflow"])
        ms += conv.pass_ms()
        sha.update(text)
        for key, field in (("kept", "n_kept"), ("entries", "n_entries"), ("hits", "n_hits")):
            sums[key] += int(info[field])
        sums["out_bytes"] += len(text)
    return ms, time.time() - t0, sha.hexdigest(), sums


def device_run(nodes_path, amap, amap4, faa, reps, result):
    os.environ["KAIJU_GPU_CONVERT_TIMES"] = "1"
    from kaiju_amd import api
    host = api.Taxonomy(nodes_path)
    dtax = api.DeviceTaxonomy(host, 0)
    pairs = [(N_NODES + 1 + i, 2 + i) for i in range(N_MERGED)]
    passes = ("lines", "kinds", "entries", "decide", "lengths", "write", "finish")
    maps = {}
    for rules, text in (("refseq", amap), ("nr", amap4)):
        m = api.AccMap(dtax, pairs, rules=rules)
        ms, t0 = np.zeros(api.ACCMAP_PASSES), time.time()
        for k, b in enumerate(ct.blocks(text, True)):
            m.add_text(b, first_block=k == 0)
            ms += m.pass_ms()
        wall = time.time() - t0
        st = m.info()
        maps[rules] = m
        result["map_" + rules] = {"pass_ms": dict(zip(("lines", "parse", "grow", "insert", "resolve"), (round(float(x), 3) for x in ms))), "wall_s": round(wall, 3),
                                  "bytes": len(text), "GBps_passes": round(len(text) / 1e6 / max(ms.sum(), 1e-9), 2), "entries": int(st["entries"]), "slots": int(st["slots"]),
                                  "duplicates": int(st["duplicates"]), "lines_no_insert": int(st["lines_no_insert"]), "rehashes": int(st["rehashes"])}
    convs = {rules: api.Converter(dtax, maps[rules], rules=rules) for rules in ("refseq", "nr")}
    runs = {"refseq": [], "nr": []}
    for rep in range(reps):                                   # alternating, so that both see the same state of the machine
        for rules in ("refseq", "nr"):
            ms, wall, sha, sums = convert_all(convs[rules], api, faa)
            runs[rules].append({"pass_ms": dict(zip(passes, (round(float(x), 3) for x in ms))), "wall_s": round(wall, 3), "out_sha256": sha, **sums})
    for rules in ("refseq", "nr"):
        timed = runs[rules][1:] if reps > 1 else runs[rules]
        assert len({r["out_sha256"] for r in runs[rules]}) == 1
        entries = sorted(r["pass_ms"]["entries"] for r in timed)
        total = sorted(sum(r["pass_ms"].values()) for r in timed)
        result["convert_" + rules] = {"kernel_of_entries": "k_cv_first" if rules == "refseq" else "k_cv_entries", "runs": runs[rules],
                                      "entries_ms_median": entries[len(entries) // 2], "entries_ms_min": entries[0], "entries_ms_max": entries[-1],
                                      "passes_ms_median": round(total[len(total) // 2], 3), "GBps_passes": round(len(faa) / 1e6 / max(total[len(total) // 2], 1e-9), 2),
                                      "out_sha256": runs[rules][0]["out_sha256"]}      # (refseq: equal to reference_out_sha256 of --reference)
    for x in list(convs.values()) + list(maps.values()) + [dtax]:
        x.close()


if __name__ == "__main__":
    main()
