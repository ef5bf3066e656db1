"""Record extraction on the device (kaiju_amd/csrc/ingest.hip): kaiju_gpu_parse_block on every input of
tests/ingest_inputs.py against the reading loop of the command line programs (ingest_expect), the capacity and alignment
rules, kaiju_gpu_classify_text_compact against kaiju_gpu_classify_batch_compact on host-parsed buffers, and the command line
programs with KAIJU_GPU_INGEST=device."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import ingest_expect
import ingest_inputs
import util
from kaiju_amd import build
from test_gpu_parity import Hip
from test_ingest_emu import INFO_FIELDS, build_ingest_emu, constants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_lib, golden):
    index = gpu_lib.Index(golden.fmi, device=0)
    clf = {m: gpu_lib.Classifier(index, gpu_lib.default_params(m)) for m in ("mem", "greedy")}
    tax = gpu_lib.Taxonomy(golden.nodes)
    dtax = gpu_lib.DeviceTaxonomy(tax, 0)
    yield gpu_lib, clf, dtax
    for c in clf.values():
        c.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    T, S = constants(build_ingest_emu(tmp_path_factory.mktemp("ingest_emu")))
    return ingest_inputs.cases(T, S)


def compare(got, want, what):
    n = len(want["off"]) // 2
    for f in INFO_FIELDS:
        assert int(got["info"][f]) == int(want[f]), (what, f, int(got["info"][f]), want[f])
    assert np.array_equal(got["off"], want["off"]), (what, "off")
    assert bytes(got["seqs"]) == bytes(want["seqs"]), (what, "seqs")
    assert got["names"].shape == (n, 2) and np.array_equal(got["names"], want["names"]), (what, "names")


def test_parse_block_on_every_input(ctx, inputs):
    api, clf, _ = ctx
    for name, fastq, keep, t1, t2 in inputs:
        want = ingest_expect.expected(t1, t2, fastq, keep)
        compare(api.parse_block(clf["mem"], t1, t2, fastq=fastq, keep_names=keep), want, name)


def test_capacity_one_below_the_record_count(ctx, inputs):
    api, clf, _ = ctx
    for name, fastq, keep, t1, t2 in inputs:
        if name not in ("fuzz_fastq_crlf_blanks", "fuzz_fasta", "pair_equal", "fa_header_only"):
            continue
        cap = len(ingest_expect.expected(t1, t2, fastq, keep)["off"]) // 2 - 1
        want = ingest_expect.expected(t1, t2, fastq, keep, rec_cap=cap)
        assert want["overflow"] == 1
        got = api.parse_block(clf["mem"], t1, t2, fastq=fastq, keep_names=keep, rec_cap=cap + 3, names_fill=0xdead)
        assert int(got["info"]["overflow"]) == 0
        got = api.parse_block(clf["mem"], t1, t2, fastq=fastq, keep_names=keep, rec_cap=cap, names_fill=0xdead)
        compare(got, want, name)
    # the name entries behind the capacity: the device-pointer form, whose buffers the caller owns
    hip = Hip()
    t1 = [c for c in inputs if c[0] == "fuzz_fastq"][0][3]
    n = len(ingest_expect.ref_spans(t1, True))
    d_text, d_seqs, d_off, d_names, d_info = (hip.malloc(k) for k in (len(t1) + 64, len(t1) + 64, (2 * n + 1) * 8, n * 8, 32))
    hip.h2d(d_text, np.frombuffer(t1, dtype=np.uint8))
    hip.h2d(d_off, np.full(2 * n + 1, 0xdead, dtype=np.uint64))
    hip.h2d(d_names, np.full((n, 2), 0xdead, dtype=np.uint32))
    clf["mem"].parse_block_device(d_text, len(t1), 0, 0, n - 1, d_seqs, d_off, d_names, d_info, fastq=True)
    clf["mem"].synchronize()
    info = hip.d2h(d_info, 32).view(api.PARSE_INFO_DTYPE)[0]
    names = hip.d2h(d_names, n * 8).view(np.uint32).reshape(n, 2)
    off = hip.d2h(d_off, (2 * n + 1) * 8).view(np.uint64)
    for d in (d_text, d_seqs, d_off, d_names, d_info):
        hip.free(d)
    assert int(info["overflow"]) == 1 and int(info["n_records"]) == n
    assert names[n - 1].tolist() == [0xdead, 0xdead] and names[n - 2].tolist() != [0xdead, 0xdead]
    assert off[2 * (n - 1) + 1:].tolist() == [0xdead, 0xdead]


def test_device_pointer_form_and_alignment(ctx, inputs):
    api, clf, _ = ctx
    hip = Hip()
    name, fastq, keep, t1, t2 = [c for c in inputs if c[0] == "pair_mismatch_1"][0]
    want = ingest_expect.expected(t1, t2, fastq, keep)
    n = want["n_records"]
    d1, d2, d_seqs, d_off, d_names, d_info = (hip.malloc(k) for k in (len(t1) + 64, len(t2) + 64, len(t1) + len(t2) + 64, (2 * n + 1) * 8, n * 8, 32))
    hip.h2d(d1, np.frombuffer(t1, dtype=np.uint8))
    hip.h2d(d2, np.frombuffer(t2, dtype=np.uint8))
    stream = hip.stream()
    c = clf["greedy"]
    c.parse_block_device(d1, len(t1), d2, len(t2), n, d_seqs, d_off, d_names, d_info, fastq=True, stream=stream)
    assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
    info = hip.d2h(d_info, 32).view(api.PARSE_INFO_DTYPE)[0]
    got = {"info": info, "seqs": hip.d2h(d_seqs, int(info["seq_bytes"])), "off": hip.d2h(d_off, (2 * n + 1) * 8).view(np.uint64),
           "names": hip.d2h(d_names, n * 8).view(np.uint32).reshape(n, 2)}
    compare(got, want, name)
    # a text pointer at +4 bytes
    assert d1 % 16 == 0
    assert api.lib().kaiju_gpu_parse_block_device(c._h, d1 + 4, len(t1) - 4, None, 0, 1, 0, n, d_seqs, d_off, d_names, d_info, None) == -1
    assert api.lib().kaiju_gpu_parse_block_device(c._h, d1, len(t1), d2 + 4, len(t2) - 4, 1, 0, n, d_seqs, d_off, d_names, d_info, None) == -1
    with pytest.raises(api.KaijuGpuError):
        c.parse_block_device(d1 + 4, len(t1) - 4, 0, 0, n, d_seqs, d_off, d_names, d_info, fastq=True)
    for d in (d1, d2, d_seqs, d_off, d_names, d_info):
        hip.free(d)


def test_torch_tensor_form(gpu_lib, golden):
    """Classifier.parse_block_tensors in a process of its own: torch first, then the library (one HIP runtime per process)"""
    code = (
        "import sys, torch, numpy as np\n"
        "sys.path[:0] = [%r, %r]\n"
        "import ingest_expect\n"
        "from kaiju_amd import api\n"
        "t1 = open(%r, 'rb').read()\n"
        "want = ingest_expect.expected(t1, None, True)\n"
        "c = api.Classifier(api.Index(%r, device=0), api.default_params('mem'))\n"
        "d = torch.frombuffer(bytearray(t1), dtype=torch.uint8).cuda()\n"
        "torch.cuda.synchronize()\n"
        "out = c.parse_block_tensors(d, fastq=True, rec_cap=want['n_records'])\n"
        "c.synchronize()\n"
        "info = out['info'].cpu().numpy().view(api.PARSE_INFO_DTYPE)[0]\n"
        "n = want['n_records']\n"
        "assert int(info['n_records']) == n and int(info['seq_bytes']) == want['seq_bytes'] and int(info['max_mate_len']) == want['max_mate_len']\n"
        "assert bytes(out['seqs'].cpu().numpy()[:want['seq_bytes']]) == bytes(want['seqs'])\n"
        "assert np.array_equal(out['off'].cpu().numpy().view(np.uint64), want['off'])\n"
        "assert np.array_equal(out['names'].cpu().numpy().view(np.uint32)[:n], want['names'])\n"
        "print('TENSORS_OK')\n"
    ) % (util.ROOT, os.path.join(util.ROOT, "tests"), os.path.join(golden.dir, "reads.fq"), golden.fmi)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"TENSORS_OK" in r.stdout, r.stderr[-2000:].decode()


def as_fasta(path, width=60):
    names, reads = util.read_fastq(path)
    out = []
    for n, r in zip(names, reads):
        out.append(b">" + n.encode() + b" wrapped/1\n" + b"".join(r[k:k + width] + b"\n" for k in range(0, len(r), width)))
    return b"".join(out)


@pytest.mark.parametrize("mode", ["mem", "greedy"])
@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_classify_text_compact(ctx, golden, mode, fmt):
    """text in == host-parsed buffers in, byte for byte: reads.fq, the pairs, and both rewritten as wrapped FASTA"""
    api, clf, dtax = ctx
    c = clf[mode]
    files = [os.path.join(golden.dir, f) for f in ("reads.fq", "pairs_1.fq", "pairs_2.fq")]
    texts = [open(f, "rb").read() for f in files] if fmt == "fastq" else [as_fasta(f) for f in files]
    for t1, t2, seqs, off, names in ((texts[0], None, golden.seqs, golden.off, golden.names), (texts[1], texts[2], golden.pseqs, golden.poff, golden.pnames)):
        seqs, off = np.ascontiguousarray(seqs, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
        want = c.classify_compact(dtax, seqs, off, paired=t2 is not None)
        got = c.classify_text_compact(dtax, t1, t2, fastq=fmt == "fastq")
        assert int(got["info"]["name_mismatch"]) == api.NO_MISMATCH and int(got["info"]["overflow"]) == 0
        assert np.array_equal(got["off"], off)
        assert got["compact"].tobytes() == want.tobytes()
        assert [t1[p:p + l].decode() for p, l in got["names"]] == list(names)


# ---- the command line programs with KAIJU_GPU_INGEST=device ------------------------------------------------------------
def cli(golden, args, out, device, extra_env=None, check=True):
    env = dict(os.environ, **(extra_env or {}))
    env.pop("KAIJU_GPU_INGEST", None)
    if device:
        env["KAIJU_GPU_INGEST"] = "device"
    return subprocess.run([build.build_cli(), "-t", golden.nodes, "-f", golden.fmi, "-o", out] + args, env=env, capture_output=True, check=check)


def rows(path, k=3):
    return [tuple(l.rstrip("\n").split("\t")[:k]) for l in open(path)]


@pytest.mark.parametrize("mode,ref,pair", [("mem", "ref_mem_1.tsv", False), ("greedy", "ref_greedy_1.tsv", False), ("greedy", "ref_greedy_1_pe.tsv", True)])
def test_cli_device_ingest_columns(gpu_lib, golden, tmp_path, mode, ref, pair):
    out = str(tmp_path / "d.tsv")
    files = ["-i", os.path.join(golden.dir, "pairs_1.fq"), "-j", os.path.join(golden.dir, "pairs_2.fq")] if pair else ["-i", os.path.join(golden.dir, "reads.fq")]
    cli(golden, files + ["-a", mode], out, device=True)
    assert rows(out) == rows(os.path.join(golden.dir, ref))


def test_cli_device_ingest_many_blocks_gz(gpu_lib, golden, tmp_path):
    gz = str(tmp_path / "r.fq.gz")
    with gzip.open(gz, "wb") as f:
        f.write(open(os.path.join(golden.dir, "reads.fq"), "rb").read() * 3)
    outs = []
    for device in (False, True):
        out = str(tmp_path / ("d.tsv" if device else "h.tsv"))
        cli(golden, ["-i", gz, "-a", "mem"], out, device, {"KAIJU_GPU_BATCH": "1000"})
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and outs[0].count(b"\n") == 3 * len(golden.reads)


def test_cli_device_ingest_renamed_read(gpu_lib, golden, tmp_path):
    p2 = open(os.path.join(golden.dir, "pairs_2.fq"), "rb").read().split(b"\n")
    p2[4 * 7] = b"@renamed/2"
    bad = tmp_path / "bad_2.fq"
    bad.write_bytes(b"\n".join(p2))
    msgs = []
    for device in (False, True):
        r = cli(golden, ["-i", os.path.join(golden.dir, "pairs_1.fq"), "-j", str(bad), "-a", "mem"], str(tmp_path / "x.tsv"), device, check=False)
        assert r.returncode != 0
        msgs.append(r.stderr)
    assert b"Read names are not identical between the two input files" in msgs[1] and msgs[0] == msgs[1]


def test_cli_device_ingest_ignored_with_verbose(gpu_lib, golden, tmp_path):
    outs = []
    for device in (False, True):
        out = str(tmp_path / ("d.tsv" if device else "h.tsv"))
        cli(golden, ["-i", os.path.join(golden.dir, "reads.fq"), "-a", "greedy", "-v"], out, device)
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and rows(str(tmp_path / "d.tsv"), 7)[0] == tuple(open(os.path.join(golden.dir, "ref_greedy_1.tsv")).readline().rstrip("\n").split("\t")[:7])
