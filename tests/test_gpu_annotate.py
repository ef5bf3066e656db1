"""The stand-alone annotator on the device (kaiju_amd/csrc/annotate.hip): kaiju_gpu_annotate_text on the fixtures the reference
tool wrote, on the small texts and the capacity cases of tests/test_annotate_emu.py, against tests/annotate_expect.py; the
device-pointer form with buffers and a stream of the caller's; kaiju_gpu_format_verbose_device and kaiju_gpu_annotate_text_device
behind each other on one stream for the golden reads; the refusals; and kaiju_amd/bin/kaiju-addTaxonNames against the files the
unmodified tool wrote."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import annotate_expect
import annotate_inputs as ai
import names_inputs
from kaiju_amd import api, build
from test_format_verbose_emu import device_arrays
from test_gpu_format_verbose import names_blob
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

GUARD = 37
CLI_TIMEOUT = 120       # seconds per run of the command line program


class Trees:
    """per mode the tables on the device, an annotator on them and the expectation"""

    def __init__(self, api, golden):
        self.api, self.t = api, {}
        jobs = [(m, names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, ai.deep_names(m)) for m in names_inputs.MODES]
        jobs += [("golden:" + m, golden.nodes, names_inputs.GOLDEN_NAMES, ai.golden_names(m)) for m in ("name", "path")]
        for key, nodes, names, expect in jobs:
            host = api.TaxonNames(nodes, names, key.split(":", 1)[1] if key.startswith("golden:") else key)
            dev = api.DeviceTaxonNames(host, 0)
            self.t[key] = (api.Annotator(dev), expect, dev, host)

    def __getitem__(self, key):
        return self.t[key]

    def close(self):
        for an, _, dev, host in self.t.values():
            an.close(); dev.close(); host.close()


@pytest.fixture(scope="module")
def trees(gpu_lib, golden):
    t = Trees(gpu_lib, golden)
    yield t
    t.close()


def run_host_form(an, text, drop, cap):
    out = np.full(cap + GUARD, 0xA5, dtype=np.uint8)
    _, info = an.annotate(text, drop_unclassified=drop, out_cap=cap, out=out)
    return out, info


def compare(out, info, want, what):
    for f in annotate_expect.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def test_fixtures_against_the_tools_files(trees):
    for fixture in ("deep", "odd"):
        text = ai.fixture_input(fixture)
        for out, mode, drop in ai.FOUR_MODES:
            got, info = trees[mode][0].annotate(text, drop_unclassified=drop)
            assert got == ai.fixture_output(fixture, out), (fixture, out)
            assert int(info["overflow"]) == 0 and int(info["text_bytes"]) == len(got)
    for run in ("mem", "greedy"):
        for kind in ("name", "path"):
            got, info = trees["golden:" + kind][0].annotate(ai.verbose_input(run))
            assert got == ai.verbose_output(run, kind), (run, kind)


def test_small_cases_in_every_variant(trees):
    cases = ai.small_cases() + [("deep", ai.fixture_input("deep")), ("odd", ai.fixture_input("odd"))]
    assert len(cases) > 30
    for what, text in cases:
        for mode, drop in ai.VARIANTS:
            an, names = trees[mode][0], trees[mode][1]
            want = annotate_expect.expected(names, text, drop)
            assert len(want["text"]) <= an.bound(text)
            out, info = run_host_form(an, text, drop, len(want["text"]) + 5)
            compare(out, info, want, (what, mode, drop))


def test_second_step_of_the_scan_at_the_exact_capacity(trees):
    text = ai.big()
    an, names = trees["path"][0], trees["path"][1]
    want = annotate_expect.expected(names, text)
    assert want["info"]["n_lines"] == names_inputs.BIG_COUNT and want["info"]["n_empty"] > 6000
    out, info = run_host_form(an, text, False, len(want["text"]))
    compare(out, info, want, "big")


def capacity_jobs(trees):
    text = ai.capacity_text()
    jobs = []
    for mode, drop in (("path", False), ("path", True), ("name", True), (ai.RANKS_DEEP, False)):
        full = annotate_expect.expected(trees[mode][1], text, drop)
        jobs += [(mode, drop, cap) for cap in ai.capacity_caps(full, mode)]
    assert len(jobs) == 2 * 7 + 2 * 6
    return text, jobs


def test_capacity(trees):
    text, jobs = capacity_jobs(trees)
    for mode, drop, cap in jobs:
        want = annotate_expect.expected(trees[mode][1], text, drop, cap)
        out, info = run_host_form(trees[mode][0], text, drop, cap)
        compare(out, info, want, (mode, drop, cap))


def device_run(hip, an, text, drop, cap, stream):
    """the device-pointer form on buffers of the caller's; returns (out with 64 bytes behind cap, info)"""
    d_text, d_out, d_info = hip.malloc(len(text) + 64), hip.malloc(cap + 64 + 16), hip.malloc(64)
    assert d_text % 16 == 0 and d_out % 16 == 0
    if text:
        hip.h2d(d_text, np.frombuffer(text, dtype=np.uint8))
    hip.h2d(d_out, np.full(cap + 64, 0xA5, dtype=np.uint8))
    an.annotate_device(d_text, len(text), d_out, cap, d_info, drop_unclassified=drop, stream=stream)
    assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
    info = hip.d2h(d_info, 48).view(api.ANNOTATE_INFO_DTYPE)[0]
    out = hip.d2h(d_out, cap + 64)
    for d in (d_text, d_out, d_info):
        hip.free(d)
    return out, info


def test_device_pointer_form(trees):
    hip = Hip()
    stream = hip.stream()
    text, jobs = capacity_jobs(trees)
    for mode, drop, cap in jobs:
        want = annotate_expect.expected(trees[mode][1], text, drop, cap)
        out, info = device_run(hip, trees[mode][0], text, drop, cap, stream)
        compare(out, info, want, (mode, drop, cap))
    for what, text in ai.small_cases():
        if what in ("bytes_0", "bytes_4097", "only_newlines", "no_newline", "body_32_off1_shifted", "long_line", "tab_and_run_over_tile_3"):
            want = annotate_expect.expected(trees["path"][1], text, False)
            out, info = device_run(hip, trees["path"][0], text, False, len(want["text"]) + 5, stream)
            compare(out, info, want, what)


@pytest.mark.parametrize("mode", ["mem", "greedy"])
def test_verbose_lines_and_names_on_one_stream(gpu_lib, golden, trees, mode):
    """kaiju_gpu_format_verbose_device writes the lines of kaiju -v, kaiju_gpu_annotate_text_device reads them where they lie:
    no host round trip between the two.  mem: the annotator is told the size of the text; greedy: the buffer between the two
    is filled with newlines first and handed over whole - lines of length 0 give nothing"""
    api, hip = gpu_lib, Hip()
    stream = hip.stream()
    index = api.Index(golden.fmi, device=0)
    index.upload_accessions()
    tax = api.Taxonomy(golden.nodes)
    dtax = api.DeviceTaxonomy(tax, 0)
    c = api.Classifier(index, api.default_params(mode))
    names = [nm.encode() for nm in golden.names]
    blob, spans = names_blob(api, names)
    hits, v, pos, pep = c.classify_verbose_packed(golden.seqs, golden.off)
    recs = c.lca(dtax, hits)
    verbose = ai.verbose_input(mode)                       # the reference binary's own kaiju -v
    n, mid_cap = len(hits), len(verbose) + 1000
    nacc, acc, tlen, _ = device_arrays({"v": v})
    pep_a, blob_a = np.frombuffer(bytes(pep) + b"\0", dtype=np.uint8), np.frombuffer(blob + b"\0", dtype=np.uint8)
    arrays = [hits, recs, np.ascontiguousarray(golden.off, dtype=np.uint64), nacc, acc, pos, tlen, pep_a, blob_a, spans]
    bufs = [hip.malloc(a.nbytes + 16) for a in arrays]
    for d, a in zip(bufs, arrays):
        if a.nbytes:
            hip.h2d(d, a)
    d_hits, d_recs, d_off, d_nacc, d_acc, d_tpos, d_tlen, d_pep, d_text, d_names = bufs
    d_mid, d_vinfo, d_info = hip.malloc(mid_cap + 64), hip.malloc(64), hip.malloc(64)
    hip.ck(hip.L.hipMemset(C.c_void_p(d_mid), 10, C.c_size_t(mid_cap + 64)))
    for kind in ("name", "path"):
        an, expect = trees["golden:" + kind][0], trees["golden:" + kind][1]
        want_text = ai.verbose_output(mode, kind)
        given = len(verbose) if mode == "mem" else mid_cap
        want = annotate_expect.expected(expect, verbose + b"\n" * (given - len(verbose)))
        assert want["text"] == want_text                  # (the tool's recorded output for the reference's -v lines)
        cap = len(want_text) + 5
        d_out = hip.malloc(cap + 64 + 16)
        hip.h2d(d_out, np.full(cap + 64, 0xA5, dtype=np.uint8))
        c.format_verbose_device(d_hits, d_recs, d_off, n, d_nacc, d_acc, d_tpos, d_tlen, d_pep, 0xffffffff, d_text, len(blob), d_names, d_mid, mid_cap, d_vinfo,
                                paired=False, stream=stream)
        an.annotate_device(d_mid, given, d_out, cap, d_info, stream=stream)
        assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        assert bytes(hip.d2h(d_mid, len(verbose))) == verbose
        compare(hip.d2h(d_out, cap + 64), hip.d2h(d_info, 48).view(api.ANNOTATE_INFO_DTYPE)[0], want, (mode, kind))
        hip.free(d_out)
    for d in bufs + [d_mid, d_vinfo, d_info]:
        hip.free(d)
    c.close()


def test_refusals(gpu_lib, trees):
    api, hip = gpu_lib, Hip()
    L, an = api.lib(), trees["name"][0]
    d = hip.malloc(256)
    hip.memset(d, 256)
    args = lambda text, nbytes, out: (an._h, text, nbytes, 0, out, 64, d + 192, None)
    assert L.kaiju_gpu_annotate_text_device(*args(d, 16, d + 64)) == 0
    assert L.kaiju_gpu_annotate_text_device(*args(d + 4, 16, d + 64)) == -1          # KAIJU_GPU_ERR_ARG: the text is misaligned
    assert b"16-byte aligned" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_annotate_text_device(*args(d, 16, d + 68)) == -1              # ... the output is
    assert L.kaiju_gpu_annotate_text_device(*args(d, 0xfffffff1, d + 64)) == -1      # more than kji::kMaxBytes
    assert b"2^32" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_annotate_text_device(*args(d, 16, d + 64)[:6], None, None) == -1
    assert L.kaiju_gpu_annotate_text_device(None, d, 16, 0, d + 64, 64, d + 192, None) == -1
    assert L.kaiju_gpu_annotator_create(None, None) == -1
    info = np.zeros(1, dtype=api.ANNOTATE_INFO_DTYPE)
    assert L.kaiju_gpu_annotate_text(an._h, None, 5, 0, None, 0, info.ctypes.data) == -1
    assert L.kaiju_gpu_annotate_text(an._h, None, 0, 0, None, 0, info.ctypes.data) == 0 and int(info[0]["text_bytes"]) == 0 and int(info[0]["n_lines"]) == 0
    assert hip.L.hipDeviceSynchronize() == 0
    hip.free(d)


def test_names_on_another_device(gpu_lib, trees):
    """an annotator works on the device of its names, whatever device the caller has current; buffers that lie on another
    device are refused"""
    api = gpu_lib
    if api.device_count() < 2:
        pytest.skip("one device visible")
    hip = Hip()
    dev = api.DeviceTaxonNames(trees["path"][3], 1)
    an = api.Annotator(dev)
    got, _ = an.annotate(ai.fixture_input("odd"))
    assert got == ai.fixture_output("odd", "out_path.tsv")
    assert hip.L.hipSetDevice(0) == 0
    d = hip.malloc(256)                                      # on device 0
    hip.memset(d, 256)
    assert api.lib().kaiju_gpu_annotate_text_device(an._h, d, 16, 0, d + 64, 64, d + 192, None) == -1
    assert b"another device" in api.lib().kaiju_gpu_last_error()
    hip.free(d)
    an.close(); dev.close()


# ---- the command line program -------------------------------------------------------------------------------------------
def cli(args, block=None, check=True):
    env = dict(os.environ)
    env.pop("KAIJU_ANNOTATE_BLOCK", None)
    if block:
        env["KAIJU_ANNOTATE_BLOCK"] = str(block)
    exe = build.build_annotate_cli()
    return subprocess.run([exe] + args, env=env, capture_output=True, check=check, timeout=CLI_TIMEOUT)


MODE_ARGS = {"out_name.tsv": [], "out_path.tsv": ["-p"], "out_ranks.tsv": ["-r", "genus,species,phylum,genus"], "out_path_u.tsv": ["-u", "-p"]}


@pytest.mark.parametrize("fixture", ["deep", "odd"])
def test_cli_against_the_tools_files(gpu_lib, tmp_path, fixture):
    inp = os.path.join(ai.fixture_dir(fixture), "in.tsv")
    base = ["-t", names_inputs.DEEP_NODES, "-n", names_inputs.DEEP_NAMES, "-i", inp]
    for k, (out, args) in enumerate(MODE_ARGS.items()):
        want = ai.fixture_output(fixture, out)
        o = str(tmp_path / out)
        r = cli(base + ["-o", o] + args, block=(64, 4096, 1, None)[k])
        with open(o, "rb") as f:
            assert f.read() == want, (fixture, out)
        assert r.stdout == b""
        e = annotate_expect.expected(ai.deep_names("path"), ai.fixture_input(fixture))["info"]
        for count, word in ((e["n_bad_id"], b"readable taxon id"), (e["n_unknown_taxon"], b"is no node of"), (e["n_unnamed_taxon"], b"no scientific name")):
            lines = [l for l in r.stderr.split(b"\n") if word in l]
            assert len(lines) == (1 if count else 0) and (not count or (b" %d " % count) in lines[0]), (word, r.stderr[-500:])
    r = cli(base + ["-p"], block=333)                        # standard output
    assert r.stdout == ai.fixture_output(fixture, "out_path.tsv")


def test_cli_verbose_lines(gpu_lib, golden, tmp_path):
    r = cli(["-t", golden.nodes, "-n", names_inputs.GOLDEN_NAMES, "-i", os.path.join(ai.GOLDEN, "ref_greedy_1.tsv"), "-p", "-v"], block=5000)
    assert r.stdout == ai.verbose_output("greedy", "path") and b"Annotating" in r.stderr


def test_cli_failures(gpu_lib, tmp_path):
    inp = os.path.join(ai.fixture_dir("odd"), "in.tsv")
    t, n = ["-t", names_inputs.DEEP_NODES], ["-n", names_inputs.DEEP_NAMES]
    for args, word in ((t + n + ["-i", inp, "-p", "-r", "genus"], b"-p and -r"), (n + ["-i", inp], b"-t"), (t + ["-i", inp], b"-n"), (t + n, b"-i"),
                       (t + n + ["-i", str(tmp_path / "none.tsv")], b"none.tsv"), (["-t", str(tmp_path / "none.dmp")] + n + ["-i", inp], b"none.dmp"),
                       (t + n + ["-i", inp, "-o", str(tmp_path / "no" / "dir" / "o.tsv")], b"o.tsv")):
        r = cli(args, check=False)
        assert r.returncode == 1 and word in r.stderr and r.stdout == b"", (args, r.returncode, r.stderr[-300:])
