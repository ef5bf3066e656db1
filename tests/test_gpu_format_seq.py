"""The lines of kaijux / kaijup on the device (kaiju_amd/csrc/format_seq.hip): kaiju_gpu_format_seq on every input of
tests/format_seq_inputs.py, on contexts over an index of sequence ids built of the names those inputs refer to, against
format_seq_expect; the device-pointer form with buffers and a stream of the caller's; the name table of the golden index read back
through the formatter; kaiju_gpu_classify_batch_seq_text on the golden reads against the reference binaries' own files; and
kaijux / kaijup with KAIJU_GPU_SEQ_OUTPUT=device against the same command without the switch and against those files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import format_seq_expect as fse
import format_seq_inputs as fsi
from kaiju_amd import build, mkfmi
from test_format_seq_emu import build_format_seq_emu, constants, device_arrays
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

CLI_TIMEOUT = 120       # seconds per run of a command line program


class Small:
    """an index of fsi.index_names(), loaded for sequence ids, and contexts on it"""

    def __init__(self, api, directory):
        self.api = api
        faa = str(directory / "names.faa")
        with open(faa, "wb") as f:
            for nm, s in zip(fsi.index_names(), fsi.db_proteins()):
                f.write(b">" + nm + b"\n" + s + b"\n")
        self.fmi = mkfmi.build_fmi(faa, str(directory / "names.fmi"))
        self.index = api.Index(self.fmi, device=0, id_mode=api.IDS_SEQUENCE)
        L = api.lib()
        self.db_names = [L.kaiju_gpu_index_seq_name(self.index._h, q) for q in range(len(fsi.DB_NAMES))]
        self.clf = {}

    def of(self, mode, protein=False, min_evalue=0.01, min_frag=fsi.M, min_score=fsi.MIN_SCORE):
        key = (mode, bool(protein), min_evalue, min_frag, min_score)
        if key not in self.clf:
            self.clf[key] = self.api.Classifier(self.index, self.api.default_params(mode, min_evalue=min_evalue, input_is_protein=1 if protein else 0,
                                                                                    min_fragment_length=min_frag, min_score=min_score))
        return self.clf[key]

    def for_case(self, case):
        return self.of(case["mode"], case["protein"], case["min_evalue"], case["min_frag"], case["min_score"])


def run_host_form(c, case, cap, slack=32):
    out = np.full(cap + slack, 0xA5, dtype=np.uint8)
    return c.format_seq(case["hits"], case["off"], case["text1"], case["names"], paired=case["paired"], u_rule=case["u_rule"],
                        seqs=case["seqs"] if case["u_rule"] == fse.U_PROTEIN else None, v=case["v"], text_pos=case["text_pos"], text=case["pep"],
                        text_cap=case["text_cap"], out_cap=cap, out=out)


@pytest.fixture(scope="module")
def small(gpu_lib, tmp_path_factory):
    s = Small(gpu_lib, tmp_path_factory.mktemp("seq_names_index"))
    L = gpu_lib.lib()
    L.kaiju_gpu_index_seq_name.restype = C.c_char_p
    # the sequences of the index are the names of the inputs (the builder numbers them in an order of its own)
    assert sorted(s.db_names) == sorted(fsi.index_names()) and len(set(s.db_names)) == len(s.db_names)
    # in front of the upload the passes refuse to run and say which call is missing
    case = fsi.make("one", [fsi.rec(b"r")])
    with pytest.raises(gpu_lib.KaijuGpuError, match="kaiju_gpu_index_upload_seq_names"):
        run_host_form(s.of("mem"), case, 64)
    assert L.kaiju_gpu_index_seq_name_bytes(s.index._h) == 0
    want = sum(len(nm) for nm in s.db_names) + 12 * len(s.db_names)
    assert s.index.upload_seq_names() == want
    assert s.index.upload_seq_names() == want                   # (a second upload changes nothing)
    assert L.kaiju_gpu_index_seq_name_bytes(s.index._h) == want
    yield s
    for k in s.clf.values():
        k.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, small):
    B, S, K = constants(build_format_seq_emu(tmp_path_factory.mktemp("format_seq_emu")))
    # the inputs number the sequences as fsi.DB_NAMES does: renumbered to the index's order.  A context on a device has the
    # db_length of its index: the cases made for another one stay with the emulation
    number = np.asarray([small.db_names.index(nm) for nm in fsi.index_names()], dtype=np.uint64)
    all_cases = [k for k in fsi.cases(B, S, K, small.index.db_length) if k["db"] == "golden"]
    for case in all_cases:
        ids = case["hits"]["taxid"]
        known = ids < len(number)
        ids[known] = number[ids[known].astype(np.int64)]
    return all_cases


@pytest.fixture(scope="module")
def want_of(small, inputs):
    memo = {}

    def get(case):
        if case["id"] not in memo:
            memo[case["id"]] = fse.expected(case, small.index.db_length, db_names=small.db_names)
        return memo[case["id"]]
    return get


def compare(out, info, want, what):
    for f in fse.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def test_format_seq_on_every_input(small, inputs, want_of):
    assert {k["mode"] for k in inputs} == {"mem", "greedy"} and {k["u_rule"] for k in inputs} == {0, 1} and len(inputs) >= 10 + 9 + 8 + 12
    for case in inputs:
        want = want_of(case)
        cap = len(want["text"]) + 5
        out, info = run_host_form(small.for_case(case), case, cap)
        compare(out, info, want, case["id"])
    gates = [want_of(k)["res"]["classified"] for k in inputs if k["id"].startswith("gate_")]
    assert len(gates) == 6 and all(g.any() and not g.all() for g in gates)          # (the gate cuts on this index's db_length too)


def test_format_seq_capacity(small, inputs, want_of):
    jobs = fsi.capacity_cases(inputs, want_of)
    assert len(jobs) == 8 * len(fsi.CAPACITY_IDS)
    for case, cap in jobs:
        want = fse.expected(case, small.index.db_length, cap, db_names=small.db_names)
        out, info = run_host_form(small.for_case(case), case, cap)
        compare(out, info, want, (case["id"], cap))


def test_device_pointer_form(small, inputs, want_of):
    """buffers of the caller's, a stream of the caller's: capacity cases and whole inputs, small ones first so that the scratch of
    the context grows and is used again; what lies at or behind out_cap stays as it was"""
    hip = Hip()
    stream = hip.stream()
    ids = ("n_3", "u_protein_greedy", "ids_plain", "n_257", "alignment_grid", "n_3")
    jobs = [(k, cap) for k, cap in fsi.capacity_cases(inputs, want_of) if k["id"] in ids]
    jobs += [(k, None) for i in ids for k in inputs if k["id"] == i] + [(k, None) for k in inputs if k["id"] in ("n_0", "n_%d" % fsi.BIG_COUNT, "gate_pairs_nt_db_golden_E_0.01")]
    assert len(jobs) == 5 * 8 + 6 + 3
    contexts = set()
    for case, cap in jobs:
        want = fse.expected(case, small.index.db_length, cap, db_names=small.db_names)
        cap = len(want["text"]) if cap is None else cap
        n = len(case["hits"])
        text = np.frombuffer(case["text1"] + b"\0", dtype=np.uint8)
        pep = np.frombuffer((case["pep"] or b"") + b"\0", dtype=np.uint8)
        seqs = np.frombuffer(case["seqs"] + b"\0", dtype=np.uint8)
        tlen, _ = device_arrays(case)
        arrays = [case["hits"], case["off"], seqs, case["text_pos"], tlen, pep, text, case["names"], np.full(cap + 64, 0xA5, dtype=np.uint8)]
        bufs = [hip.malloc(a.nbytes + 16) for a in arrays] + [hip.malloc(32)]
        for d, a in zip(bufs, arrays):
            if a.nbytes:
                hip.h2d(d, a)
        d_hits, d_off, d_seqs, d_tpos, d_tlen, d_pep, d_text, d_names, d_out, d_info = bufs
        c = small.for_case(case)
        contexts.add(id(c))
        assert d_out % 16 == 0
        protein_rule = case["u_rule"] == fse.U_PROTEIN
        c.format_seq_device(d_hits, d_off, n, d_seqs if protein_rule else 0, d_tpos, d_tlen, 0 if case["pep"] is None else d_pep, case["text_cap"], d_text,
                            len(case["text1"]), d_names, d_out, cap, d_info, paired=case["paired"], u_rule=case["u_rule"], stream=stream)
        assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        info = hip.d2h(d_info, 32).view(small.api.FORMAT_VERBOSE_INFO_DTYPE)[0]
        out = hip.d2h(d_out, cap + 64)
        if case["id"] == "texts":
            # (no flags in the device form: a record is truncated iff its text_len exceeds text_cap)
            want["info"]["n_truncated"] -= int(np.count_nonzero(case["v"]["truncated"]))
        compare(out, info, want, (case["id"], cap))
        if n == 3:
            # an output pointer at +4 bytes
            assert small.api.lib().kaiju_gpu_format_seq_device(c._h, d_hits, d_off, n, 0, 0, None, d_tpos, d_tlen, d_pep, case["text_cap"], d_text,
                                                               len(case["text1"]), d_names, d_out + 4, cap, d_info, None) == -1
        for d in bufs:
            hip.free(d)
    assert len(contexts) < len(jobs)                              # (contexts were used more than once)


def test_bad_arguments(small, gpu_lib, golden):
    case = fsi.make("one", [fsi.rec(b"r")])
    c = small.of("mem")
    with pytest.raises(gpu_lib.KaijuGpuError, match="u_rule"):
        c.format_seq(case["hits"], case["off"], case["text1"], case["names"], u_rule=2, out_cap=64)
    with pytest.raises(gpu_lib.KaijuGpuError, match="NULL"):       # the kaijup rule without the reads
        c.format_seq(case["hits"], case["off"], case["text1"], case["names"], u_rule=1, out_cap=64)
    # an index of taxon ids: the table can be uploaded, the lines are refused
    tix = gpu_lib.Index(golden.fmi, device=0)
    assert tix.upload_seq_names() > 0
    tc = gpu_lib.Classifier(tix, gpu_lib.default_params("mem"))
    with pytest.raises(gpu_lib.KaijuGpuError, match="KAIJU_GPU_IDS_SEQUENCE"):
        tc.format_seq(case["hits"], case["off"], case["text1"], case["names"], out_cap=64)
    blob, spans = names_blob(gpu_lib, [nm.encode() for nm in golden.names[:4]])
    with pytest.raises(gpu_lib.KaijuGpuError, match="KAIJU_GPU_IDS_SEQUENCE"):
        tc.classify_seq_text(golden.seqs[: int(golden.off[8])], golden.off[:9], blob, spans)
    tc.close()
    tix.close()


# ---- the golden index -----------------------------------------------------------------------------------------------------
class Gold:
    def __init__(self, api, golden):
        self.api = api
        self.index = api.Index(golden.fmi, device=0, id_mode=api.IDS_SEQUENCE)
        self.index.upload_seq_names()


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


def test_name_table_read_back(gold):
    """one record per sequence of the golden index, its only id that sequence: column 4 is the name kaiju_gpu_index_seq_name gives"""
    api = gold.api
    L = api.lib()
    L.kaiju_gpu_index_seq_name.restype = C.c_char_p
    nseq = int(gold.index.info.nseq)
    names = [L.kaiju_gpu_index_seq_name(gold.index._h, q) for q in range(nseq)]
    assert nseq > 20 and all(nm for nm in names) and L.kaiju_gpu_index_seq_name(gold.index._h, nseq) is None
    assert int(L.kaiju_gpu_index_seq_name_bytes(gold.index._h)) == sum(len(nm) for nm in names) + 12 * nseq
    hits = np.zeros(nseq, dtype=api.HIT_DTYPE)
    hits["best"], hits["n_ids"] = 20, 1
    hits["taxid"][:, 0] = np.arange(nseq)
    off = np.zeros(2 * nseq + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.tile(np.asarray([150, 0], dtype=np.uint64), nseq))
    blob, spans = names_blob(api, [b"s%d" % q for q in range(nseq)])
    c = api.Classifier(gold.index, api.default_params("mem"))
    want = b"".join(b"C\ts%d\t20\t%s,\t\n" % (q, names[q]) for q in range(nseq))
    out, info = c.format_seq(hits, off, blob, spans, out_cap=len(want) + 16)
    assert int(info["text_bytes"]) == len(want) and int(info["n_classified"]) == nseq and bytes(out[: len(want)]) == want
    c.close()


@pytest.mark.parametrize("verbose", [False, True])
@pytest.mark.parametrize("mode", ["greedy", "mem"])
@pytest.mark.parametrize("shape", ["single", "paired", "protein"])
def test_classify_seq_text_golden(gold, golden, mode, shape, verbose):
    api = gold.api
    c = api.Classifier(gold.index, api.default_params(mode, input_is_protein=1 if shape == "protein" else 0))
    v = "_v" if verbose else ""
    seqs, off, names, ref = {"single": (golden.seqs, golden.off, golden.names, f"refx_{mode}{v}.tsv"),
                             "paired": (golden.pseqs, golden.poff, golden.pnames, f"refx_{mode}_pe{v}.tsv"),
                             "protein": (golden.prot_seqs, golden.prot_off, golden.prot_fullnames, f"refpx_{mode}{v}.tsv")}[shape]
    names = [nm.encode() for nm in names]
    blob, spans = names_blob(api, names)
    text, info = c.classify_seq_text(seqs, off, blob, spans, paired=shape == "paired", verbose=verbose,
                                     u_rule=api.U_RULE_PROTEIN if shape == "protein" else api.U_RULE_NUCLEOTIDE)
    want = open(os.path.join(golden.dir, ref), "rb").read()
    assert text == want                                                    # the reference binary's own file, every line
    assert int(info["text_bytes"]) == len(want) and int(info["n_records"]) == len(names) and int(info["overflow"]) == 0
    assert int(info["n_classified"]) == want.count(b"\nC\t") + (1 if want.startswith(b"C\t") else 0) and 0 < int(info["n_classified"]) < len(names)
    assert int(info["n_inexact"]) == 0 and int(info["n_truncated"]) == 0
    st = c.stats()
    assert int(st.n_reads) == len(names) and int(st.error_flags) == 0
    c.close()


# ---- the command line programs with the switch ----------------------------------------------------------------------------
def cli(golden, args, out, device, prog, extra=None):
    env = dict(os.environ)
    for k in ("KAIJU_GPU_INGEST", "KAIJU_GPU_OUTPUT", "KAIJU_GPU_VERBOSE_OUTPUT", "KAIJU_GPU_SEQ_OUTPUT", "KAIJU_GPU_VERBOSE_BUDGET", "KAIJU_GPU_BATCH"):
        env.pop(k, None)
    env.update(extra or {})
    if device:
        env.update(KAIJU_GPU_SEQ_OUTPUT="device")
    exe = os.path.join(os.path.dirname(build.build_cli()), prog)
    pre = [] if prog in ("kaijux", "kaijup") else ["-t", golden.nodes]
    return subprocess.run([exe] + pre + ["-f", golden.fmi, "-o", out] + args, env=env, capture_output=True, check=True, timeout=CLI_TIMEOUT)


@pytest.mark.parametrize("verbose", [False, True])
@pytest.mark.parametrize("mode", ["mem", "greedy"])
@pytest.mark.parametrize("prog", ["kaijux", "kaijux_pe", "kaijup"])
def test_cli_seq_device_output(gpu_lib, golden, tmp_path, prog, mode, verbose):
    v = "_v" if verbose else ""
    inp, ref = {"kaijux": (["-i", os.path.join(golden.dir, "reads.fq")], f"refx_{mode}{v}.tsv"),
                "kaijux_pe": (["-i", os.path.join(golden.dir, "pairs_1.fq"), "-j", os.path.join(golden.dir, "pairs_2.fq")], f"refx_{mode}_pe{v}.tsv"),
                "kaijup": (["-i", golden.prot_fa], f"refpx_{mode}{v}.tsv")}[prog]
    outs = []
    for device in (False, True):
        out = str(tmp_path / ("d.tsv" if device else "h.tsv"))
        r = cli(golden, inp + ["-a", mode] + (["-v"] if verbose else []), out, device, prog.split("_")[0])
        assert b"KAIJU_GPU_SEQ_OUTPUT" not in r.stderr
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and outs[1] == open(os.path.join(golden.dir, ref), "rb").read()


@pytest.mark.parametrize("verbose", [False, True])
def test_cli_seq_device_output_batches_and_pieces(gpu_lib, golden, tmp_path, verbose):
    """small batches and a small budget for the rows of -v: the sample spans several batches, with -v every batch several pieces"""
    outs = []
    for device in (False, True):
        out = str(tmp_path / ("d.tsv" if device else "h.tsv"))
        cli(golden, ["-i", os.path.join(golden.dir, "reads.fq"), "-a", "greedy"] + (["-v"] if verbose else []), out, device, "kaijux",
            extra={"KAIJU_GPU_BATCH": "200", "KAIJU_GPU_VERBOSE_BUDGET": "20000"})
        outs.append(open(out, "rb").read())
    assert len(golden.reads) > 3 * 200                             # (and a read of 150 nt takes more than 100 bytes of the budget)
    assert outs[0] == outs[1] and outs[1] == open(os.path.join(golden.dir, "refx_greedy%s.tsv" % ("_v" if verbose else "")), "rb").read()


def test_cli_switch_ignored_by_kaiju(gpu_lib, golden, tmp_path):
    outs, errs = [], []
    for device in (False, True):
        out = str(tmp_path / ("d.tsv" if device else "h.tsv"))
        r = cli(golden, ["-i", os.path.join(golden.dir, "reads.fq"), "-a", "greedy"], out, device, "kaiju")
        assert r.returncode == 0
        outs.append(open(out, "rb").read())
        errs.append(r.stderr)
    assert outs[0] == outs[1] and outs[0].count(b"\n") == len(golden.reads)
    assert errs[1].count(b"KAIJU_GPU_SEQ_OUTPUT=device is ignored") == 1 and b"KAIJU_GPU_SEQ_OUTPUT" not in errs[0]
