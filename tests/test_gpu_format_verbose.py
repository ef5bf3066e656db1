"""The lines of kaiju -v on the device (kaiju_amd/csrc/format_verbose.hip): kaiju_gpu_format_verbose on every input of
tests/format_verbose_inputs.py, on a context over an index built of the names those inputs refer to, against
format_verbose_expect; the device-pointer form with buffers and a stream of the caller's; kaiju_gpu_classify_batch_verbose_text
on the golden reads against the reference binary's own files and against lines assembled from
kaiju_gpu_classify_batch_verbose_packed and the host finalisation; and the command line programs with
KAIJU_GPU_VERBOSE_OUTPUT=device against the same command without the switch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import format_verbose_expect as fve
import format_verbose_inputs as fvi
from kaiju_amd import build, mkfmi
from test_format_verbose_emu import build_format_verbose_emu, constants, device_arrays
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

CLI_TIMEOUT = 120       # seconds per run of a command line program


class Small:
    """an index of fvi.index_names() and contexts on it"""

    def __init__(self, api, directory):
        self.api = api
        faa = str(directory / "names.faa")
        with open(faa, "wb") as f:
            for nm, s in zip(fvi.index_names(), fvi.db_proteins()):
                f.write(b">" + nm + b"\n" + s + b"\n")
        self.index = api.Index(mkfmi.build_fmi(faa, str(directory / "names.fmi")), device=0)
        L = api.lib()
        self.db_names = [L.kaiju_gpu_index_seq_name(self.index._h, q) for q in range(len(fvi.DB_NAMES))]
        self.clf = {}

    def of(self, mode, protein=False, min_evalue=0.01):
        key = (mode, bool(protein), min_evalue)
        if key not in self.clf:
            self.clf[key] = self.api.Classifier(self.index, self.api.default_params(mode, min_evalue=min_evalue, input_is_protein=1 if protein else 0))
        return self.clf[key]

    def for_case(self, case):
        return self.of(case["mode"], case["protein"], case["min_evalue"])


def run_host_form(c, case, cap, slack=32):
    out = np.full(cap + slack, 0xA5, dtype=np.uint8)
    return c.format_verbose(case["hits"], case["v"], case["text_pos"], case["pep"], case["recs"], case["off"], case["text1"], case["names"],
                            paired=case["paired"], text_cap=case["text_cap"], out_cap=cap, out=out)


@pytest.fixture(scope="module")
def small(gpu_lib, tmp_path_factory):
    s = Small(gpu_lib, tmp_path_factory.mktemp("names_index"))
    # the sequences of the index are the names of the inputs (the builder numbers them in an order of its own)
    assert sorted(s.db_names) == sorted(fvi.index_names()) and len(set(s.db_names)) == len(s.db_names)
    # in front of the upload the passes refuse to run and say which call is missing
    case = fvi.make("one", [fvi.rec(b"r")])
    with pytest.raises(gpu_lib.KaijuGpuError, match="kaiju_gpu_index_upload_accessions"):
        run_host_form(s.of("mem"), case, 64)
    assert gpu_lib.lib().kaiju_gpu_index_accession_bytes(s.index._h) == 0
    want = sum(len(p) for p in (fve.prefix(nm) for nm in s.db_names) if p is not None) + 16 * len(s.db_names)
    assert s.index.upload_accessions() == want
    assert s.index.upload_accessions() == want                  # (a second upload changes nothing)
    yield s
    for k in s.clf.values():
        k.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, small):
    B, S, K = constants(build_format_verbose_emu(tmp_path_factory.mktemp("format_verbose_emu")))
    # the inputs number the sequences as fvi.DB_NAMES does: renumbered to the index's order
    number = np.asarray([small.db_names.index(nm) for nm in fvi.index_names()], dtype=np.uint32)
    all_cases = fvi.cases(B, S, K, small.index.db_length)
    for case in all_cases:
        acc = case["v"]["acc_iseq"]
        known = acc < len(number)
        acc[known] = number[acc[known]]
    return all_cases


@pytest.fixture(scope="module")
def want_of(small, inputs):
    memo = {}

    def get(case):
        if case["id"] not in memo:
            memo[case["id"]] = fve.expected(case, small.index.db_length, db_names=small.db_names)
        return memo[case["id"]]
    return get


def compare(out, info, want, what):
    for f in fve.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def test_format_verbose_on_every_input(small, inputs, want_of):
    assert len(inputs) == 8 + 6 + 12 and {k["mode"] for k in inputs} == {"mem", "greedy"}
    for case in inputs:
        want = want_of(case)
        cap = len(want["text"]) + 5
        out, info = run_host_form(small.for_case(case), case, cap)
        compare(out, info, want, case["id"])
    gates = [want_of(k)["res"]["classified"] for k in inputs if k["id"].startswith("gate_")]
    assert all(g.any() and not g.all() for g in gates)          # (the gate cuts on this index's db_length too)


def test_format_verbose_capacity(small, inputs, want_of):
    jobs = fvi.capacity_cases(inputs, want_of)
    assert len(jobs) == 36
    for case, cap in jobs:
        want = fve.expected(case, small.index.db_length, cap, db_names=small.db_names)
        out, info = run_host_form(small.for_case(case), case, cap)
        compare(out, info, want, (case["id"], cap))


def test_device_pointer_form(small, inputs, want_of):
    """buffers of the caller's, a stream of the caller's: every capacity case and the largest input; what lies at or behind
    out_cap stays as it was"""
    hip = Hip()
    stream = hip.stream()
    jobs = fvi.capacity_cases(inputs, want_of) + [(k, None) for k in inputs if k["id"] in ("n_0", "n_65537", "gate_pairs_nt_db_golden_E_0.01")]
    assert len(jobs) == 39
    for case, cap in jobs:
        want = fve.expected(case, small.index.db_length, cap, db_names=small.db_names)
        cap = len(want["text"]) if cap is None else cap
        n = len(case["recs"])
        text = np.frombuffer(case["text1"] + b"\0", dtype=np.uint8)
        pep = np.frombuffer(case["pep"] + b"\0", dtype=np.uint8)
        nacc, acc, tlen, _ = device_arrays(case)
        arrays = [case["hits"], case["recs"], case["off"], nacc, acc, case["text_pos"], tlen, pep, text, case["names"], np.full(cap + 64, 0xA5, dtype=np.uint8)]
        bufs = [hip.malloc(a.nbytes + 16) for a in arrays] + [hip.malloc(32)]
        for d, a in zip(bufs, arrays):
            if a.nbytes:
                hip.h2d(d, a)
        d_hits, d_recs, d_off, d_nacc, d_acc, d_tpos, d_tlen, d_pep, d_text, d_names, d_out, d_info = bufs
        c = small.for_case(case)
        assert d_out % 16 == 0
        c.format_verbose_device(d_hits, d_recs, d_off, n, d_nacc, d_acc, d_tpos, d_tlen, d_pep, case["text_cap"], d_text, len(case["text1"]), d_names,
                                d_out, cap, d_info, paired=case["paired"], stream=stream)
        assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        info = hip.d2h(d_info, 32).view(small.api.FORMAT_VERBOSE_INFO_DTYPE)[0]
        out = hip.d2h(d_out, cap + 64)
        if case["id"] == "texts":
            # (no flags in the device form: a record is truncated iff its text_len exceeds text_cap)
            want["info"]["n_truncated"] -= int(np.count_nonzero(case["v"]["truncated"]))
        compare(out, info, want, (case["id"], cap))
        if n == 17:
            # an output pointer at +4 bytes
            assert small.api.lib().kaiju_gpu_format_verbose_device(c._h, d_hits, d_recs, d_off, n, 0, d_nacc, d_acc, d_tpos, d_tlen, d_pep, case["text_cap"],
                                                                   d_text, len(case["text1"]), d_names, d_out + 4, cap, d_info, None) == -1
        for d in bufs:
            hip.free(d)


# ---- reads in, text out: the golden reads ---------------------------------------------------------------------------------
class Gold:
    def __init__(self, api, golden):
        self.api = api
        self.index = api.Index(golden.fmi, device=0)
        self.index.upload_accessions()
        self.tax = api.Taxonomy(golden.nodes)
        self.dtax = api.DeviceTaxonomy(self.tax, 0)


@pytest.fixture(scope="module")
def gold(gpu_lib, golden):
    return Gold(gpu_lib, golden)


def names_blob(api, names):
    """the names one behind the other and their spans"""
    spans = np.zeros(len(names), dtype=api.NAME_SPAN_DTYPE)
    at = 0
    for r, nm in enumerate(names):
        spans[r] = (at, len(nm))
        at += len(nm)
    return b"".join(names), spans


def assembled(gold, c, seqs, off, names, paired):
    """the lines from kaiju_gpu_classify_batch_verbose_packed and the finalisation on the host (LCA included)"""
    hits, v, pos, text = c.classify_verbose_packed(seqs, off, paired=paired)
    res = c.finalize(gold.tax, hits, off, paired=paired)
    L = gold.api.lib()
    out = []
    for r in range(len(hits)):
        if not res[r]["classified"]:
            out.append(b"U\t" + names[r] + b"\t0\n")
            continue
        acc = [L.kaiju_gpu_index_seq_name(gold.index._h, int(q)) for q in v[r]["acc_iseq"][: int(v[r]["n_acc"])]]
        out.append(fve.verbose_line(names[r], int(res[r]["taxon"]), int(res[r]["best"]), [int(x) for x in hits[r]["taxid"][: int(hits[r]["n_ids"])]], acc,
                                    text[int(pos[r]): int(pos[r]) + int(v[r]["text_len"])]))
    return b"".join(out)


@pytest.mark.parametrize("mode", ["mem", "greedy"])
@pytest.mark.parametrize("shape", ["single", "paired", "protein"])
def test_classify_verbose_text_golden(gold, golden, mode, shape):
    api = gold.api
    c = api.Classifier(gold.index, api.default_params(mode, input_is_protein=1 if shape == "protein" else 0))
    seqs, off, names, ref = {"single": (golden.seqs, golden.off, golden.names, f"ref_{mode}_1.tsv"),
                             "paired": (golden.pseqs, golden.poff, golden.pnames, f"ref_{mode}_1_pe.tsv"),
                             "protein": (golden.prot_seqs, golden.prot_off, golden.prot_names, f"refp_{mode}_1.tsv")}[shape]
    names = [nm.encode() for nm in names]
    blob, spans = names_blob(api, names)
    text, info = c.classify_verbose_text(gold.dtax, seqs, off, blob, spans, paired=shape == "paired")
    want = open(os.path.join(golden.dir, ref), "rb").read()
    assert text == want                                                    # the reference binary's own file, every line
    assert text == assembled(gold, c, seqs, off, names, shape == "paired")
    assert int(info["text_bytes"]) == len(want) and int(info["n_records"]) == len(names) and int(info["overflow"]) == 0
    assert int(info["n_classified"]) == want.count(b"\nC\t") + (1 if want.startswith(b"C\t") else 0) and 0 < int(info["n_classified"]) < len(names)
    assert int(info["n_inexact"]) == 0 and int(info["n_truncated"]) == 0
    st = c.stats()
    assert int(st.n_reads) == len(names) and int(st.error_flags) == 0
    c.close()


# ---- the command line programs with the switch ----------------------------------------------------------------------------
def cli(golden, args, out, device, prog="kaiju", extra=None):
    env = dict(os.environ)
    for k in ("KAIJU_GPU_INGEST", "KAIJU_GPU_OUTPUT", "KAIJU_GPU_VERBOSE_OUTPUT", "KAIJU_GPU_VERBOSE_BUDGET", "KAIJU_GPU_BATCH"):
        env.pop(k, None)
    env.update(extra or {})
    if device:
        env.update(KAIJU_GPU_VERBOSE_OUTPUT="device")
    exe = os.path.join(os.path.dirname(build.build_cli()), prog)
    pre = [] if prog in ("kaijux", "kaijup") else ["-t", golden.nodes]
    return subprocess.run([exe] + pre + ["-f", golden.fmi, "-o", out, "-v"] + args, env=env, capture_output=True, check=True, timeout=CLI_TIMEOUT)


@pytest.mark.parametrize("leg", ["mem", "greedy", "paired", "pieces", "batches"])
def test_cli_verbose_device_output(gpu_lib, golden, tmp_path, leg):
    reads = os.path.join(golden.dir, "reads.fq")
    args = {"mem": ["-i", reads, "-a", "mem"], "greedy": ["-i", reads, "-a", "greedy"], "pieces": ["-i", reads, "-a", "greedy"],
            "batches": ["-i", reads, "-a", "mem"],
            "paired": ["-i", os.path.join(golden.dir, "pairs_1.fq"), "-j", os.path.join(golden.dir, "pairs_2.fq"), "-a", "greedy"]}[leg]
    extra = {"pieces": {"KAIJU_GPU_VERBOSE_BUDGET": "100000"}, "batches": {"KAIJU_GPU_BATCH": "1000"}}.get(leg)
    outs = []
    for device in (False, True):
        out = str(tmp_path / ("d.tsv" if device else "h.tsv"))
        r = cli(golden, args, out, device, extra=extra)
        assert b"KAIJU_GPU_VERBOSE_OUTPUT" not in r.stderr
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and outs[0].count(b"\n") == len(golden.pnames if leg == "paired" else golden.reads)
    assert outs[1].count(b"\t") > 3 * outs[1].count(b"\n") and b"U\t" in outs[1]
    if leg in ("mem", "greedy", "paired"):
        ref = {"mem": "ref_mem_1.tsv", "greedy": "ref_greedy_1.tsv", "paired": "ref_greedy_1_pe.tsv"}[leg]
        assert outs[1] == open(os.path.join(golden.dir, ref), "rb").read()


def test_cli_verbose_device_output_multi(gpu_lib, golden, tmp_path):
    reads = os.path.join(golden.dir, "reads.fq")
    outs = []
    for device in (False, True):
        o = [str(tmp_path / ("%s%d.tsv" % ("d" if device else "h", k))) for k in (0, 1)]
        cli(golden, ["-i", reads + "," + reads, "-a", "mem"], ",".join(o), device, prog="kaiju-multi")
        outs.append([open(p, "rb").read() for p in o])
    assert outs[0] == outs[1] and outs[0][0] == outs[0][1] and outs[0][0].count(b"\n") == len(golden.reads)


def test_cli_switch_ignored_by_kaijux(gpu_lib, golden, tmp_path):
    outs, errs = [], []
    for device in (False, True):
        out = str(tmp_path / ("d.tsv" if device else "h.tsv"))
        r = cli(golden, ["-i", os.path.join(golden.dir, "reads.fq"), "-a", "greedy"], out, device, prog="kaijux")
        assert r.returncode == 0
        outs.append(open(out, "rb").read())
        errs.append(r.stderr)
    assert outs[0] == outs[1] and outs[0].count(b"\n") == len(golden.reads)
    assert errs[1].count(b"KAIJU_GPU_VERBOSE_OUTPUT=device is ignored") == 1 and b"KAIJU_GPU_VERBOSE_OUTPUT" not in errs[0]
