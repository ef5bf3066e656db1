"""The output lines on the device (kaiju_amd/csrc/format.hip): kaiju_gpu_format_compact on every input of
tests/format_inputs.py a context on the golden index can have, against format_expect (the decisions of kaiju_finalize_compact);
the device-pointer form with buffers of the caller's, the capacity cases among them; kaiju_gpu_classify_text_to_text against
kaiju_gpu_classify_batch_compact on host-parsed buffers -> kaiju_finalize_compact -> format_expect; and the command line programs
with KAIJU_GPU_INGEST=device KAIJU_GPU_OUTPUT=device against the same command without either switch."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import format_expect
import format_inputs
import ingest_expect
import ingest_inputs
from kaiju_amd import build
from test_format_emu import build_format_emu, constants
from test_gpu_ingest import as_fasta
from test_gpu_parity import Hip
from test_ingest_emu import build_ingest_emu
from test_ingest_emu import constants as ingest_constants

pytestmark = pytest.mark.gpu

CLI_TIMEOUT = 120       # seconds per run of a command line program
MAX_READ = 3000         # texts of ingest_inputs with longer reads are left to the ingest tests (they test no formatting)


class Ctx:
    def __init__(self, api, golden):
        self.api = api
        self.index = api.Index(golden.fmi, device=0)
        self.tax = api.Taxonomy(golden.nodes)
        self.dtax = api.DeviceTaxonomy(self.tax, 0)
        self.clf = {}

    def of(self, mode, protein=False, min_evalue=0.01):
        key = (mode, bool(protein), min_evalue)
        if key not in self.clf:
            self.clf[key] = self.api.Classifier(self.index, self.api.default_params(mode, min_evalue=min_evalue, input_is_protein=1 if protein else 0))
        return self.clf[key]

    def for_case(self, case):
        return self.of(case["mode"], case["protein"], case["min_evalue"])


@pytest.fixture(scope="module")
def ctx(gpu_lib, golden):
    c = Ctx(gpu_lib, golden)
    yield c
    for k in c.clf.values():
        k.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, ctx):
    B, S, K = constants(build_format_emu(tmp_path_factory.mktemp("format_emu")))
    return [k for k in format_inputs.cases(B, S, K, ctx.index.db_length) if k["db"] == "golden"]


def compare(out, info, want, what):
    for f in format_expect.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def test_format_compact_on_every_input(ctx, inputs):
    assert len(inputs) == 12 + 12 and {k["mode"] for k in inputs} == {"mem", "greedy"}
    for case in inputs:
        want = format_expect.expected(case, ctx.index.db_length)
        cap = len(want["text"]) + 5
        out = np.full(cap + 32, 0xA5, dtype=np.uint8)
        out, info = ctx.for_case(case).format_compact(case["recs"], case["off"], case["text1"], case["names"], paired=case["paired"], out_cap=cap, out=out)
        compare(out, info, want, case["id"])


def test_format_compact_capacity(ctx, inputs):
    jobs = format_inputs.capacity_cases(inputs, lambda k: format_expect.expected(k, ctx.index.db_length))
    assert len(jobs) == 20
    for case, cap in jobs:
        want = format_expect.expected(case, ctx.index.db_length, cap)
        out = np.full(cap + 32, 0xA5, dtype=np.uint8)
        out, info = ctx.for_case(case).format_compact(case["recs"], case["off"], case["text1"], case["names"], out_cap=cap, out=out)
        compare(out, info, want, (case["id"], cap))


def test_device_pointer_form(ctx, inputs):
    """buffers of the caller's, a stream of the caller's: every capacity case and the largest input; what lies at or behind
    out_cap stays as it was"""
    hip = Hip()
    stream = hip.stream()
    jobs = format_inputs.capacity_cases(inputs, lambda k: format_expect.expected(k, ctx.index.db_length))
    jobs += [(k, None) for k in inputs if k["id"] in ("n_0", "n_65537", "gate_pairs_nt_db_golden_E_0.01")]
    for case, cap in jobs:
        want = format_expect.expected(case, ctx.index.db_length, cap)
        cap = len(want["text"]) if cap is None else cap
        n = len(case["recs"])
        text = np.frombuffer(case["text1"] + b"\0", dtype=np.uint8)
        bufs = [hip.malloc(k) for k in (16 * n + 16, 8 * (2 * n + 1), len(text), 8 * n + 8, cap + 64, 32)]
        d_recs, d_off, d_text, d_names, d_out, d_info = bufs
        for d, a in ((d_recs, case["recs"]), (d_off, case["off"]), (d_text, text), (d_names, case["names"]), (d_out, np.full(cap + 64, 0xA5, dtype=np.uint8))):
            if a.nbytes:
                hip.h2d(d, a)
        c = ctx.for_case(case)
        assert d_out % 16 == 0
        c.format_compact_device(d_recs, d_off, n, d_text, len(case["text1"]), d_names, d_out, cap, d_info, paired=case["paired"], stream=stream)
        assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        info = hip.d2h(d_info, 24).view(format_expect.FORMAT_INFO_DTYPE)[0]
        out = hip.d2h(d_out, cap + 64)
        compare(out, info, want, (case["id"], cap))
        if n == 17:
            # an output pointer at +4 bytes
            assert ctx.api.lib().kaiju_gpu_format_compact_device(c._h, d_recs, d_off, n, 0, d_text, len(case["text1"]), d_names, d_out + 4, cap, d_info, None) == -1
        for d in bufs:
            hip.free(d)


def host_reference(ctx, c, t1, t2, fastq, keep, mode):
    """host-parsed buffers -> kaiju_gpu_classify_batch_compact -> kaiju_finalize_compact -> the lines"""
    e = ingest_expect.expected(t1, t2, fastq, keep)
    n = len(e["off"]) // 2
    names = np.zeros(n, dtype=ctx.api.NAME_SPAN_DTYPE)
    names["pos"], names["len"] = e["names"][:, 0], e["names"][:, 1]
    seqs, off = np.ascontiguousarray(e["seqs"], dtype=np.uint8), np.ascontiguousarray(e["off"], dtype=np.uint64)
    recs = c.classify_compact(ctx.dtax, seqs, off, paired=t2 is not None) if n else np.zeros(0, dtype=ctx.api.COMPACT_DTYPE)
    case = {"mode": mode, "protein": False, "min_evalue": 0.01, "paired": t2 is not None, "recs": recs, "off": off, "names": names, "text1": t1}
    return e, format_expect.expected(case, ctx.index.db_length)


@pytest.mark.parametrize("mode", ["mem", "greedy"])
@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_classify_text_to_text_golden(ctx, golden, mode, fmt):
    c = ctx.of(mode)
    files = [os.path.join(golden.dir, f) for f in ("reads.fq", "pairs_1.fq", "pairs_2.fq")]
    texts = [open(f, "rb").read() for f in files] if fmt == "fastq" else [as_fasta(f) for f in files]
    for t1, t2 in ((texts[0], None), (texts[1], texts[2])):
        e, want = host_reference(ctx, c, t1, t2, fmt == "fastq", False, mode)
        got = c.classify_text_to_text(ctx.dtax, t1, t2, fastq=fmt == "fastq")
        assert got["text"] == want["text"]
        for f in format_expect.INFO_FIELDS:
            assert int(got["format_info"][f]) == want["info"][f], f
        assert int(got["info"]["n_records"]) == e["n_records"] and int(got["info"]["name_mismatch"]) == ctx.api.NO_MISMATCH
        assert 0 < want["info"]["n_classified"] < want["info"]["n_records"]


def test_classify_text_to_text_ingest_inputs(ctx, tmp_path_factory):
    T, S = ingest_constants(build_ingest_emu(tmp_path_factory.mktemp("ingest_emu")))
    c = ctx.of("mem")
    ran = 0
    for name, fastq, keep, t1, t2 in ingest_inputs.cases(T, S):
        e = ingest_expect.expected(t1, t2, fastq, keep)
        if e["max_mate_len"] > MAX_READ:
            continue
        _, want = host_reference(ctx, c, t1, t2, fastq, keep, "mem")
        got = c.classify_text_to_text(ctx.dtax, t1, t2, fastq=fastq, keep_names=keep)
        assert got["text"] == want["text"], name
        assert int(got["format_info"]["n_records"]) == want["info"]["n_records"] and int(got["format_info"]["overflow"]) == 0, name
        assert int(got["info"]["name_mismatch"]) == e["name_mismatch"], name
        ran += 1
    assert ran > 50
    # a capacity one byte short: the call says so and reports the size needed
    t1 = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reads.fq"), "rb").read()
    full = c.classify_text_to_text(ctx.dtax, t1, fastq=True)
    with pytest.raises(ctx.api.KaijuGpuError):
        c.classify_text_to_text(ctx.dtax, t1, fastq=True, out_cap=len(full["text"]) - 1)


# ---- the command line programs with both switches -------------------------------------------------------------------------
def cli(golden, args, out, device, prog="kaiju"):
    env = dict(os.environ)
    for k in ("KAIJU_GPU_INGEST", "KAIJU_GPU_OUTPUT"):
        env.pop(k, None)
    if device:
        env.update(KAIJU_GPU_INGEST="device", KAIJU_GPU_OUTPUT="device", KAIJU_GPU_BATCH="1000")
    else:
        env.update(KAIJU_GPU_BATCH="1000")
    exe = os.path.join(os.path.dirname(build.build_cli()), prog)
    return subprocess.run([exe, "-t", golden.nodes, "-f", golden.fmi, "-o", out] + args, env=env, capture_output=True, check=True, timeout=CLI_TIMEOUT)


@pytest.mark.parametrize("leg", ["mem", "greedy", "paired", "gz"])
def test_cli_device_output(gpu_lib, golden, tmp_path, leg):
    reads = os.path.join(golden.dir, "reads.fq")
    if leg == "gz":
        reads = str(tmp_path / "r.fq.gz")
        with gzip.open(reads, "wb") as f:
            f.write(open(os.path.join(golden.dir, "reads.fq"), "rb").read() * 3)
    args = {"mem": ["-i", reads, "-a", "mem"], "greedy": ["-i", reads, "-a", "greedy"], "gz": ["-i", reads, "-a", "mem"],
            "paired": ["-i", os.path.join(golden.dir, "pairs_1.fq"), "-j", os.path.join(golden.dir, "pairs_2.fq"), "-a", "greedy"]}[leg]
    outs = []
    for device in (False, True):
        out = str(tmp_path / ("d.tsv" if device else "h.tsv"))
        r = cli(golden, args, out, device)
        assert b"KAIJU_GPU_OUTPUT" not in r.stderr
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and outs[0].count(b"\n") == (3 if leg == "gz" else 1) * len(golden.pnames if leg == "paired" else golden.reads)
    assert b"C\t" in outs[1] and b"U\t" in outs[1]


def test_cli_device_output_multi(gpu_lib, golden, tmp_path):
    reads = os.path.join(golden.dir, "reads.fq")
    outs = []
    for device in (False, True):
        o = [str(tmp_path / ("%s%d.tsv" % ("d" if device else "h", k))) for k in (0, 1)]
        cli(golden, ["-i", reads + "," + reads, "-a", "mem"], ",".join(o), device, prog="kaiju-multi")
        outs.append([open(p, "rb").read() for p in o])
    assert outs[0] == outs[1] and outs[0][0] == outs[0][1] and outs[0][0].count(b"\n") == len(golden.reads)


def test_cli_device_output_ignored_with_verbose(gpu_lib, golden, tmp_path):
    outs, errs = [], []
    for device in (False, True):
        out = str(tmp_path / ("d.tsv" if device else "h.tsv"))
        r = cli(golden, ["-i", os.path.join(golden.dir, "reads.fq"), "-a", "greedy", "-v"], out, device)
        outs.append(open(out, "rb").read())
        errs.append(r.stderr)
    assert outs[0] == outs[1] and outs[0].count(b"\t") > 3 * len(golden.reads)
    assert errs[1].count(b"KAIJU_GPU_OUTPUT=device is ignored") == 1 and b"KAIJU_GPU_OUTPUT" not in errs[0]
