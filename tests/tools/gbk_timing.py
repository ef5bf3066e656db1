"""Per-pass times of the GenBank converter on a synthetic input:  python tests/tools/gbk_timing.py [--records N] [--out FILE]

The input is made here (seeded): --records records (default 1300, about 150 MB) in the shape of a RefSeq .gbff file.  A record
is a genome of 50 000 bases: LOCUS and source lines, 45 genes - a `gene` and a `CDS` feature of 13 qualifier lines and a
/translation of 60 to 600 letters in lines of 58 - and an ORIGIN block of 834 lines.  By bytes that is 56 % ORIGIN lines, 19 %
translation lines and 25 % other feature lines (the result holds the measured mix); about one line in four holds a `"` and is
looked at byte by byte.  One letter in 300 of a translation is X, B, Z or U.

Reported, over --repeat passes through the file behind one warm-up pass: the milliseconds per pass summed over the blocks of
16 MiB (KAIJU_GPU_CONVERT_TIMES=1; median and range over the repeats), GB/s of text over those sums and over the wall time of
the calls (uploads and downloads included), and the SHA-256 of the output - compared with REFERENCE, what the unmodified
kaiju-gbk2faa.pl wrote from the same input.

--dump DIR writes the input instead, and --reference SCRIPT runs the unmodified script on it with perl (on the host, one
thread) and prints the hash to put into REFERENCE: context for the device numbers, taken on whatever machine this runs on."""
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

BLOCK = 16 << 20
GENOME, GENES, SEED = 50000, 45, 11
# records -> (bytes of the input, bytes and SHA-256 of the file the unmodified script wrote from it)
REFERENCE = {1300: (146795222, 21020926, "e611c2dbbed64d108d288ef9bae7c0a5c0fa8fe2a617b01374cab58d12ad2b0f")}


def make_input(records, seed=SEED):
    rng = np.random.RandomState(seed)
    bases = np.frombuffer(b"acgt", dtype=np.uint8)
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    pool = letters[rng.randint(0, 20, size=1 << 20)].copy()
    odd = rng.randint(0, len(pool), size=len(pool) // 300)
    pool[odd] = np.frombuffer(b"XBZU", dtype=np.uint8)[rng.randint(0, 4, size=len(odd))]
    pool = pool.tobytes()
    origins = []
    for _ in range(16):                                         # sixteen ORIGIN blocks to draw from
        seq = bases[rng.randint(0, 4, size=GENOME)].tobytes()
        lines = []
        for at in range(0, GENOME, 60):
            row = seq[at:at + 60]
            lines.append(b"%9d " % (at + 1) + b" ".join(row[k:k + 10] for k in range(0, len(row), 10)) + b"\n")
        origins.append(b"ORIGIN      \n" + b"".join(lines) + b"//\n")
    lens = rng.randint(60, 601, size=records * GENES)
    starts = rng.randint(0, (1 << 20) - 700, size=records * GENES)
    taxa = rng.randint(2, 3000000, size=records)
    which = rng.randint(0, 16, size=records)
    out, g = [], 0
    for r in range(records):
        out.append(b"LOCUS       NZ_SYN%07d          %d bp    DNA     linear   CON 01-JAN-2024\n"
                   b"DEFINITION  Synthetic organism strain %d chromosome, whole genome shotgun sequence.\n"
                   b"ACCESSION   NZ_SYN%07d\nVERSION     NZ_SYN%07d.1\nDBLINK      BioProject: PRJNA000000\nKEYWORDS    WGS; RefSeq.\n"
                   b"SOURCE      Synthetic organism\n  ORGANISM  Synthetic organism\n            Bacteria; Synthetica.\n"
                   b"FEATURES             Location/Qualifiers\n     source          1..%d\n"
                   b'                     /organism="Synthetic organism"\n                     /mol_type="genomic DNA"\n'
                   b'                     /strain="%d"\n                     /db_xref="taxon:%d"\n' % (r, GENOME, r, r, r, GENOME, r, int(taxa[r])))
        for k in range(GENES):
            a, b = 1 + k * 1100, 1 + k * 1100 + 3 * int(lens[g]) + 2
            tag = b"SYN%07d_%05d" % (r, k)
            out.append(b"     gene            %d..%d\n"
                       b'                     /locus_tag="%s"\n'
                       b"     CDS             %d..%d\n"
                       b'                     /locus_tag="%s"\n'
                       b'                     /inference="COORDINATES: similar to AA\n'
                       b'                     sequence:RefSeq:WP_%09d.1"\n'
                       b'                     /note="Derived by automated computational analysis using\n'
                       b'                     gene prediction method: Protein Homology."\n'
                       b"                     /codon_start=1\n                     /transl_table=11\n"
                       b'                     /product="hypothetical protein"\n'
                       b'                     /protein_id="WP_%09d.1"\n' % (a, b, tag, a, b, tag, g % 999999937, g % 999999937))
            body = b'/translation="' + pool[int(starts[g]):int(starts[g]) + int(lens[g])] + b'"'
            out.append(b"".join(b"                     " + body[j:j + 58] + b"\n" for j in range(0, len(body), 58)))
            g += 1
        out.append(origins[int(which[r])])
    return b"".join(out)


def mix_of(text):
    """bytes of the ORIGIN blocks, of the translation lines and of the rest; lines, and lines that hold a `"`"""
    origin = translation = quoted = 0
    state = 0
    lines = text.split(b"\n")
    for l in lines:
        n = len(l) + 1
        if b'"' in l:
            quoted += 1
        if l.startswith(b"ORIGIN"):
            state = 1
        if state == 1:
            origin += n
            if l == b"//":
                state = 0
        elif state == 2 or b"/translation=" in l:
            translation += n
            state = 0 if l.endswith(b'"') else 2
    return {"origin": origin, "translation": translation, "other": len(text) - origin - translation, "lines": len(lines) - 1, "lines_with_quote": quoted}


def blocks(text):
    at = 0
    while at < len(text):
        end = len(text)
        if end - at > BLOCK:
            end = text.rfind(b"\n", at, at + BLOCK) + 1
        yield text[at:end]
        at = end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1300)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--dump")
    ap.add_argument("--reference")
    a = ap.parse_args()
    text = make_input(a.records)
    mix = mix_of(text)
    result = {"records": a.records, "text_bytes": len(text), "block_bytes": BLOCK, "mix_bytes": mix,
              "mix_percent": {k: round(100.0 * mix[k] / len(text), 1) for k in ("origin", "translation", "other")}}
    if a.dump or a.reference:
        d = a.dump or "/tmp/gbk_timing_%d" % os.getpid()
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "in.gbff"), "wb") as f:
            f.write(text)
        if a.reference:
            t0 = time.time()
            subprocess.run(["perl", os.path.abspath(a.reference), "in.gbff", "ref.faa"], cwd=d, check=True)
            result["reference_wall_s"] = round(time.time() - t0, 2)
            with open(os.path.join(d, "ref.faa"), "rb") as f:
                ref = f.read()
            result["reference"] = {a.records: (len(text), len(ref), hashlib.sha256(ref).hexdigest())}
    else:
        device_run(text, a.repeat, result)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


def device_run(text, repeat, result):
    os.environ["KAIJU_GPU_CONVERT_TIMES"] = "1"
    from kaiju_amd import api
    names = ("lines", "kinds", "scans", "lengths", "write", "finish")
    g = api.Gbk(0)
    parts = list(blocks(text))
    runs = []
    for rep in range(repeat + 1):                               # the first pass through the file is the warm-up
        g.reset()
        ms, t0, sha, out_bytes, recs, kinds = np.zeros(api.GBK_PASSES), time.time(), hashlib.sha256(), 0, 0, np.zeros(5, dtype=np.uint64)
        wall_calls = 0.0
        for b in parts:
            t1 = time.time()
            out, info = g.convert(b, out_cap=len(b))
            wall_calls += time.time() - t1
            assert not int(info["overflow"]) and not int(info["no_taxon_line"])
            ms += g.pass_ms()
            sha.update(out)
            out_bytes, recs, kinds = out_bytes + len(out), recs + int(info["n_records"]), kinds + info["lines_kind"]
        runs.append({"pass_ms": ms, "wall_calls_s": wall_calls, "sha": sha.hexdigest(), "out_bytes": out_bytes, "records": recs, "kinds": [int(x) for x in kinds]})
    g.close()
    timed = runs[1:]
    assert len({r["sha"] for r in runs}) == 1
    per_pass = np.array([r["pass_ms"] for r in timed])
    sums = per_pass.sum(axis=1)
    walls = np.array([r["wall_calls_s"] for r in timed])
    result["device"] = {
        "blocks": len(parts), "repeats": len(timed),
        "pass_ms_median": dict(zip(names, (round(float(x), 3) for x in np.median(per_pass, axis=0)))),
        "pass_ms_min": dict(zip(names, (round(float(x), 3) for x in per_pass.min(axis=0)))),
        "pass_ms_max": dict(zip(names, (round(float(x), 3) for x in per_pass.max(axis=0)))),
        "passes_ms_median": round(float(np.median(sums)), 3), "passes_ms_range": [round(float(sums.min()), 3), round(float(sums.max()), 3)],
        "GBps_passes_median": round(len(text) / 1e6 / float(np.median(sums)), 2),
        "wall_calls_s_median": round(float(np.median(walls)), 4), "wall_calls_s_range": [round(float(walls.min()), 4), round(float(walls.max()), 4)],
        "GBps_wall_median": round(len(text) / 1e9 / float(np.median(walls)), 2),
        "out_bytes": runs[0]["out_bytes"], "out_records": runs[0]["records"], "lines_kind": runs[0]["kinds"], "out_sha256": runs[0]["sha"]}
    ref = REFERENCE.get(result["records"])
    result["reference_sha256"] = ref[2] if ref else None
    result["matches_reference"] = bool(ref and ref[0] == len(text) and ref[1] == runs[0]["out_bytes"] and ref[2] == runs[0]["sha"]) if ref else None


if __name__ == "__main__":
    main()
