"""The lines with the column of kaiju-addTaxonNames on the device (kaiju_amd/csrc/format_names.hip): the tables the upload
builds, read back, against the host's; kaiju_gpu_format_names on the inputs of tests/format_inputs.py a context on the golden
index can have and on records drawn over every taxon of tests/golden/names/deep/, in the three modes with and without the
unclassified lines, against tests/names_expect.py; the capacity cases; the device-pointer form with buffers of the caller's;
kaiju_gpu_classify_text_to_text_names and the command line programs against the reference tool's own outputs
(tests/golden/names/golden/)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import format_expect
import format_inputs
import names_expect
import names_inputs
from kaiju_amd import build
from test_format_names_emu import build_format_names_emu, compare, constants, load
from test_gpu_format import Ctx
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

CLI_TIMEOUT = 120       # seconds per run of a command line program
GOLDEN_KINDS = {"name": "name", "path": "path", "ranks": names_inputs.RANKS_GOLDEN}
RUNS = {"mem": ("mem", False), "mem_pe": ("mem", True), "greedy": ("greedy", False), "greedy_pe": ("greedy", True)}


@pytest.fixture(scope="module")
def ctx(gpu_lib, golden):
    c = Ctx(gpu_lib, golden)
    yield c
    for k in c.clf.values():
        k.close()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_format_names_emu(tmp_path_factory.mktemp("format_names_emu"))


@pytest.fixture(scope="module")
def trees(gpu_lib):
    """per mode: deep/ on the device, and the expectation"""
    t = {}
    for m in names_inputs.MODES:
        host = gpu_lib.TaxonNames(names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, m)
        t[m] = (gpu_lib.DeviceTaxonNames(host, 0), names_inputs.deep_expect(m), host)
    yield t
    for d, _, h in t.values():
        d.close()
        h.close()


@pytest.fixture(scope="module")
def inputs(emu, ctx):
    B, S, K = constants(emu)
    cases = [k for k in format_inputs.cases(B, S, K, ctx.index.db_length) if k["db"] == "golden"]
    return cases + [names_inputs.drawn(n) for n in (1, 255, 256, 257, 300, 4096)]


@pytest.fixture(scope="module")
def base(inputs, ctx):
    return {k["id"]: format_expect.expected(k, ctx.index.db_length) for k in inputs}


def test_device_tables_match_the_host(gpu_lib, emu, trees):
    for mode in names_inputs.MODES:
        dev, _, _ = trees[mode]
        h = load(emu, names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, mode)
        most = C.c_uint64()
        cap = emu.format_names_emu_table(h, 0, None, 0, C.byref(most), 0, 1)
        assert dev.max_annotation == most.value and 0 < most.value < 2 ** 24 and (mode == names_inputs.RANKS_DEEP or most.value >= 300)
        n_ranks = 3
        tables = [("key", 0, "<u8", 1), ("parent", 1, "<u4", 1), ("name_pos", 2, "<u4", 1), ("name_len", 3, "<u4", 1), ("rank", 7, "u1", 1)]
        tables += {"name": [], "path": [("path_len", 4, "<u4", 1)], names_inputs.RANKS_DEEP: [("rank_len", 5, "<u4", 1), ("rank_src", 6, "<u4", n_ranks)]}[mode]
        for name, which, dt, per in tables:
            want = np.zeros(cap * per, dtype=dt)
            assert emu.format_names_emu_table(h, which, want.ctypes.data, want.nbytes, None, 2, 9) == cap
            got = dev.table(name, per)
            assert len(got) == len(want) and np.array_equal(got, want), (mode, name)
        if mode != "path":
            with pytest.raises(gpu_lib.KaijuGpuError):
                dev.table("path_len")
        emu.kaiju_taxon_names_free(h)


def test_format_names_on_every_input(ctx, trees, inputs, base):
    assert len(inputs) == 12 + 12 + 6
    seen = {f: 0 for f in ("n_unknown_taxon", "n_unnamed_taxon", "n_dropped")}
    for case in inputs:
        for mode, drop in names_inputs.VARIANTS:
            dev, expect, _ = trees[mode]
            want = names_expect.expected(expect, base[case["id"]], drop)
            for f in seen:
                seen[f] += want["info"][f]
            cap = len(want["text"]) + 5
            out = np.full(cap + 32, 0xA5, dtype=np.uint8)
            out, info = ctx.for_case(case).format_names(case["recs"], case["off"], case["text1"], case["names"], dev, paired=case["paired"],
                                                        drop_unclassified=drop, out_cap=cap, out=out)
            compare(out, info, want, (case["id"], mode, drop))
    assert all(v > 0 for v in seen.values()), seen
    # the bound never overflows
    case = next(k for k in inputs if k["id"] == "drawn_4096")
    dev, expect, _ = trees["path"]
    out, info = ctx.for_case(case).format_names(case["recs"], case["off"], case["text1"], case["names"], dev)
    bound = ctx.api.lib().kaiju_gpu_format_names_bound(len(case["text1"]), len(case["recs"]), dev._h)
    assert bound == len(case["text1"]) + len(case["recs"]) * (25 + dev.max_annotation) and int(info["overflow"]) == 0 and int(info["text_bytes"]) <= bound
    # lines that straddle the 4096-byte blocks of the output, a 300-byte name across 19 chunks
    want = names_expect.expected(expect, base[case["id"]])
    assert len(want["text"]) > 100 * 4096 and b"L" * 300 in want["text"] and np.diff(want["line_off"]).max() > 1000


def test_second_step_of_the_scan_at_the_exact_capacity(ctx, trees):
    """more records than the one block on top of the prefix sum takes in a step, into a buffer of exactly the text's length"""
    case = names_inputs.big()
    dev, expect, _ = trees["path"]
    want = names_expect.expected(expect, format_expect.expected(case, ctx.index.db_length), False)
    cap = len(want["text"])
    out = np.full(cap + 32, 0xA5, dtype=np.uint8)
    out, info = ctx.for_case(case).format_names(case["recs"], case["off"], case["text1"], case["names"], dev, out_cap=cap, out=out)
    compare(out, info, want, case["id"])


def test_format_names_capacity(ctx, trees, inputs, base):
    jobs = names_inputs.capacity_jobs(inputs, lambda k, m, d: names_expect.expected(trees[m][1], base[k["id"]], d))
    assert len(jobs) == 4 * (2 * 6 + 2 * 5)
    for case, mode, drop, cap in jobs:
        want = names_expect.expected(trees[mode][1], base[case["id"]], drop, cap)
        out = np.full(cap + 32, 0xA5, dtype=np.uint8)
        out, info = ctx.for_case(case).format_names(case["recs"], case["off"], case["text1"], case["names"], trees[mode][0], drop_unclassified=drop,
                                                    out_cap=cap, out=out)
        compare(out, info, want, (case["id"], mode, drop, cap))


def test_device_pointer_form(ctx, trees, inputs, base):
    """buffers of the caller's, a stream of the caller's: capacity cases and whole inputs; what lies at or behind out_cap
    stays as it was"""
    hip = Hip()
    stream = hip.stream()
    jobs = [j for j in names_inputs.capacity_jobs(inputs, lambda k, m, d: names_expect.expected(trees[m][1], base[k["id"]], d)) if j[0]["id"] in ("n_17", "drawn_300")]
    jobs += [(k, m, d, None) for k in inputs if k["id"] in ("n_0", "drawn_1", "drawn_257", "gate_pairs_nt_db_golden_E_0.01") for m, d in names_inputs.VARIANTS[1:4]]
    for case, mode, drop, cap in jobs:
        dev, expect, _ = trees[mode]
        want = names_expect.expected(expect, base[case["id"]], drop, cap)
        cap = len(want["text"]) if cap is None else cap
        n = len(case["recs"])
        text = np.frombuffer(case["text1"] + b"\0", dtype=np.uint8)
        bufs = [hip.malloc(k) for k in (16 * n + 16, 8 * (2 * n + 1), len(text), 8 * n + 8, cap + 64, 64)]
        d_recs, d_off, d_text, d_names, d_out, d_info = bufs
        for d, a in ((d_recs, case["recs"]), (d_off, case["off"]), (d_text, text), (d_names, case["names"]), (d_out, np.full(cap + 64, 0xA5, dtype=np.uint8))):
            if a.nbytes:
                hip.h2d(d, a)
        c = ctx.for_case(case)
        assert d_out % 16 == 0
        c.format_names_device(d_recs, d_off, n, d_text, len(case["text1"]), d_names, dev, d_out, cap, d_info, paired=case["paired"], drop_unclassified=drop,
                              stream=stream)
        assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        info = hip.d2h(d_info, 40).view(ctx.api.FORMAT_NAMES_INFO_DTYPE)[0]
        out = hip.d2h(d_out, cap + 64)
        compare(out, info, want, (case["id"], mode, drop, cap))
        if n == 17:
            # an output pointer at +4 bytes
            assert ctx.api.lib().kaiju_gpu_format_names_device(c._h, d_recs, d_off, n, 0, d_text, len(case["text1"]), d_names, dev._h, 0, d_out + 4, cap, d_info,
                                                               None) == -1
        for d in bufs:
            hip.free(d)


# ---- against the reference tool's outputs on the golden index ------------------------------------------------------------
def golden_file(run, kind):
    return names_inputs.read(os.path.join(names_inputs.NAMES_DIR, "golden", "%s.%s.tsv" % (run, kind)))


def unchanged_lines(golden, want):
    """(unknown, unnamed): the 'C' lines of a golden file without a column, by the reason (the database holds taxa that
    nodes.dmp does not: a hit with one id is printed without a look at the tree)"""
    N = names_expect.Names(names_inputs.read(golden.nodes), names_inputs.read(names_inputs.GOLDEN_NAMES), "name")
    why = [N.why_unchanged(int(l.split(b"\t")[2])) for l in want.split(b"\n") if l[:1] == b"C" and l.count(b"\t") == 2]
    assert all(why)
    return why.count("unknown"), why.count("unnamed")


@pytest.fixture(scope="module")
def golden_trees(gpu_lib, golden):
    t = {}
    for kind, mode in GOLDEN_KINDS.items():
        host = gpu_lib.TaxonNames(golden.nodes, names_inputs.GOLDEN_NAMES, mode)
        t[kind] = (gpu_lib.DeviceTaxonNames(host, 0), host)
    yield t
    for d, h in t.values():
        d.close()
        h.close()


@pytest.mark.parametrize("run", sorted(RUNS))
def test_classify_text_to_text_names_golden(ctx, golden, golden_trees, run):
    mode, pe = RUNS[run]
    c = ctx.of(mode)
    t1 = names_inputs.read(os.path.join(golden.dir, "pairs_1.fq" if pe else "reads.fq"))
    t2 = names_inputs.read(os.path.join(golden.dir, "pairs_2.fq")) if pe else None
    for kind in GOLDEN_KINDS:
        want = golden_file(run, kind)
        got = c.classify_text_to_text_names(ctx.dtax, golden_trees[kind][0], t1, t2, fastq=True)
        assert got["text"] == want, (run, kind)
        fi = got["format_info"]
        unknown, unnamed = unchanged_lines(golden, want)
        assert int(fi["n_unknown_taxon"]) == unknown and int(fi["n_unnamed_taxon"]) == unnamed > 0 and int(fi["n_dropped"]) == 0
        assert int(fi["n_records"]) == want.count(b"\n") and int(fi["n_classified"]) == sum(1 for l in want.split(b"\n") if l[:1] == b"C")
    # without the unclassified lines
    want = b"".join(l + b"\n" for l in golden_file(run, "path").split(b"\n") if l[:1] == b"C")
    got = c.classify_text_to_text_names(ctx.dtax, golden_trees["path"][0], t1, t2, fastq=True, drop_unclassified=True)
    assert got["text"] == want and int(got["format_info"]["n_dropped"]) == int(got["format_info"]["n_records"]) - want.count(b"\n") > 0
    # a capacity one byte short: the call says so
    with pytest.raises(ctx.api.KaijuGpuError):
        c.classify_text_to_text_names(ctx.dtax, golden_trees["path"][0], t1, t2, fastq=True, drop_unclassified=True, out_cap=len(want) - 1)


def test_null_names_are_refused(ctx, inputs):
    case = next(k for k in inputs if k["id"] == "n_17")
    c = ctx.for_case(case)
    info = np.zeros(1, dtype=ctx.api.FORMAT_NAMES_INFO_DTYPE)
    out = np.zeros(64, dtype=np.uint8)
    assert ctx.api.lib().kaiju_gpu_format_names(c._h, case["recs"].ctypes.data, case["off"].ctypes.data, 17, 0, case["text1"], len(case["text1"]),
                                                case["names"].ctypes.data, None, 0, out.ctypes.data, 64, info.ctypes.data) == -1


# ---- the command line programs ------------------------------------------------------------------------------------------
def cli(golden, args, out, env_extra, prog="kaiju", device=True, check=True):
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("KAIJU_GPU_TAXON_NAMES") or k in ("KAIJU_GPU_INGEST", "KAIJU_GPU_OUTPUT"):
            env.pop(k)
    env.update(KAIJU_GPU_BATCH="1000")
    if device:
        env.update(KAIJU_GPU_INGEST="device", KAIJU_GPU_OUTPUT="device")
    env.update(env_extra)
    exe = os.path.join(os.path.dirname(build.build_cli()), prog)
    return subprocess.run([exe, "-t", golden.nodes, "-f", golden.fmi, "-o", out] + args, env=env, capture_output=True, check=check, timeout=CLI_TIMEOUT)


def run_args(golden, run):
    mode, pe = RUNS[run]
    files = ["-i", os.path.join(golden.dir, "pairs_1.fq"), "-j", os.path.join(golden.dir, "pairs_2.fq")] if pe else ["-i", os.path.join(golden.dir, "reads.fq")]
    return files + ["-a", mode]


@pytest.mark.parametrize("run,kind", [("mem", "name"), ("greedy", "path"), ("mem_pe", "ranks"), ("greedy_pe", "path")])
def test_cli_taxon_names(gpu_lib, golden, tmp_path, run, kind):
    out = str(tmp_path / "o.tsv")
    mode = GOLDEN_KINDS[kind]
    r = cli(golden, run_args(golden, run), out, {"KAIJU_GPU_TAXON_NAMES": names_inputs.GOLDEN_NAMES, "KAIJU_GPU_TAXON_NAMES_MODE": mode})
    want = golden_file(run, kind)
    assert names_inputs.read(out) == want
    unknown, unnamed = unchanged_lines(golden, want)
    warn = [l for l in r.stderr.split(b"\n") if b"without a name" in l]
    assert len(warn) == 1 and (b"Warning: %d classified reads" % (unknown + unnamed)) in warn[0]
    assert (b"the taxon of %d is not in" % unknown) in warn[0] and (b"the taxon of %d has no scientific name" % unnamed) in warn[0] and unnamed > 0


def test_cli_taxon_names_default_mode_and_drop(gpu_lib, golden, tmp_path):
    out = str(tmp_path / "o.tsv")
    cli(golden, run_args(golden, "mem"), out, {"KAIJU_GPU_TAXON_NAMES": names_inputs.GOLDEN_NAMES})
    assert names_inputs.read(out) == golden_file("mem", "name")
    cli(golden, run_args(golden, "mem"), out, {"KAIJU_GPU_TAXON_NAMES": names_inputs.GOLDEN_NAMES, "KAIJU_GPU_TAXON_NAMES_MODE": "path", "KAIJU_GPU_TAXON_NAMES_DROP_U": "1"})
    assert names_inputs.read(out) == b"".join(l + b"\n" for l in golden_file("mem", "path").split(b"\n") if l[:1] == b"C")


def test_cli_taxon_names_multi(gpu_lib, golden, tmp_path):
    reads = os.path.join(golden.dir, "reads.fq")
    o = [str(tmp_path / ("m%d.tsv" % k)) for k in (0, 1)]
    cli(golden, ["-i", reads + "," + reads, "-a", "greedy"], ",".join(o), {"KAIJU_GPU_TAXON_NAMES": names_inputs.GOLDEN_NAMES, "KAIJU_GPU_TAXON_NAMES_MODE": "path"},
        prog="kaiju-multi")
    for p in o:
        assert names_inputs.read(p) == golden_file("greedy", "path")


def test_cli_taxon_names_refusals(gpu_lib, golden, tmp_path):
    """lines without names under a switch that asked for them are never written: -v, host output, kaijux, a bad mode, a
    names.dmp that is not there - exit status 1 and a message that says why"""
    out = str(tmp_path / "o.tsv")
    names = {"KAIJU_GPU_TAXON_NAMES": names_inputs.GOLDEN_NAMES}
    r = cli(golden, run_args(golden, "greedy") + ["-v"], out, names, check=False)
    assert r.returncode == 1 and b"KAIJU_GPU_TAXON_NAMES" in r.stderr and b"-v" in r.stderr and not (os.path.exists(out) and os.path.getsize(out))
    r = cli(golden, run_args(golden, "mem"), out, names, device=False, check=False)
    assert r.returncode == 1 and b"made on the host" in r.stderr and not (os.path.exists(out) and os.path.getsize(out))
    r = cli(golden, run_args(golden, "mem"), out, names, prog="kaijux", check=False)
    assert r.returncode == 1 and b"kaijux" in r.stderr
    r = cli(golden, run_args(golden, "mem"), out, dict(names, KAIJU_GPU_TAXON_NAMES_MODE="lineage"), check=False)
    assert r.returncode == 1 and b"KAIJU_GPU_TAXON_NAMES_MODE" in r.stderr
    r = cli(golden, run_args(golden, "mem"), out, {"KAIJU_GPU_TAXON_NAMES": str(tmp_path / "none.dmp")}, check=False)
    assert r.returncode == 1 and b"KAIJU_GPU_TAXON_NAMES" in r.stderr
