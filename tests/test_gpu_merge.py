"""The merger on the device (kaiju_amd/csrc/merge.hip): kaiju_gpu_merge_text on the fixtures the reference tool wrote, on the
small texts, the name comparisons and the capacity cases of tests/test_merge_emu.py, against tests/merge_expect.py; the
device-pointer form with buffers and a stream of the caller's; two kaiju_gpu_classify_text_to_text outputs merged where they
lie; the refusals; and kaiju_amd/bin/kaiju-mergeOutputs against the files the unmodified tool wrote."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import merge_expect as me
import merge_inputs as mi
from kaiju_amd import api, build
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

GUARD = 37
CLI_TIMEOUT = 120       # seconds per run of the command line program


class Mergers:
    """(nodes.dmp bytes or None, mode, use_score) -> a merger on device 0; nodes.dmp bytes -> the model's tree"""

    def __init__(self, api, directory):
        self.api, self.dir, self.trees, self.m = api, directory, {}, {}

    def tree(self, nodes):
        if nodes is None:
            return None, {}, None
        if nodes not in self.trees:
            path = str(self.dir / ("nodes%d.dmp" % len(self.trees)))
            with open(path, "wb") as f:
                f.write(nodes)
            host = self.api.Taxonomy(path)
            self.trees[nodes] = (self.api.DeviceTaxonomy(host, 0), me.parse_nodes(nodes), host, path)
        return self.trees[nodes][:3]

    def path(self, nodes):
        self.tree(nodes)
        return self.trees[nodes][3]

    def get(self, nodes, mode, use_score):
        key = (nodes, mode, use_score)
        dtax, parent, _ = self.tree(nodes)
        if key not in self.m:
            self.m[key] = self.api.Merger(dtax, mode, use_score)
        return self.m[key], parent

    def close(self):
        for m in self.m.values():
            m.close()
        for dtax, _, host, _ in self.trees.values():
            dtax.close()


@pytest.fixture(scope="module")
def mergers(gpu_lib, tmp_path_factory):
    m = Mergers(gpu_lib, tmp_path_factory.mktemp("merge_gpu"))
    yield m
    m.close()


def run_host_form(merger, t1, t2, final, cap):
    out = np.full(cap + GUARD, 0xA5, dtype=np.uint8)
    _, info = merger.merge(t1, t2, final=final, out_cap=cap, out=out)
    return out, info


def compare(out, info, want, what):
    for f in me.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    w = len(want["written"])
    assert bytes(out[:w]) == want["written"], (what, "text")
    assert np.all(out[w:] == 0xA5), (what, "bytes behind the lines written")


def check(mergers, nodes, t1, t2, mode, use_score, final, what):
    merger, parent = mergers.get(nodes, mode, use_score)
    want = me.expected(parent, t1, t2, mode, use_score, final)
    assert len(want["text"]) <= merger.bound(t1, t2)
    out, info = run_host_form(merger, t1, t2, final, len(want["text"]) + 5)
    compare(out, info, want, what)
    return want


@pytest.mark.parametrize("mode,use_score", mi.VARIANTS)
def test_goldens(mergers, mode, use_score):
    for what, (nodes, t1, t2), (text, summary) in (("odd", mi.odd(), mi.odd_output(mode, use_score)), ("real", mi.real(), mi.real_output(mode, use_score))):
        merger, _ = mergers.get(nodes, mode, use_score)
        got, info = merger.merge(t1, t2)
        assert got == text, what                                  # the file the tool wrote
        assert me.summary({f: int(info[f]) for f in me.INFO_FIELDS}) == summary
        check(mergers, nodes, t1, t2, mode, use_score, True, what)
    if mode == "lowest":
        _, t1, t2 = mi.odd()
        assert check(mergers, None, t1, t2, mode, use_score, True, "odd without a tree")["text"] == mi.odd_output(mode, use_score, tree=False)[0]


def test_golden_stops(mergers):
    for name in mi.stop_names():
        t1, t2, use_score, text, summary = mi.stop_case(name)
        want = check(mergers, None, t1, t2, "1", use_score, True, name)
        assert want["text"] == text and me.summary(want["info"]) == summary


def test_small_cases(mergers):
    """pair counts around a block of 256, text 1 over three tiles against one; stops at pair 0, 256, the last and two of them;
    LCAs of 1, 10, 19 and 20 digits; ids that are no number or no node; scores outside the domain; final 0 and 1 on ragged ends"""
    cases = mi.small_cases()
    assert len(cases) > 60
    for what, nodes, t1, t2, mode, use_score, final in cases:
        check(mergers, nodes, t1, t2, mode, use_score, final, what)


def test_name_compare(mergers):
    """names of 0, 1, 15, 16, 17 and 33 bytes at every relative alignment of the two lines modulo 16: equal, and differing in
    the first byte, in the last byte, by length only"""
    for what, t1, t2 in mi.name_compare_cases():
        want = check(mergers, None, t1, t2, "1", False, True, what)
        assert want["info"]["stop_pair"] == (me.NO_PAIR if "equal" in what else 7)


def capacity_jobs(mergers):
    nodes, t1, t2 = mi.odd()
    _, parent = mergers.get(nodes, "lca", True)
    full = me.expected(parent, t1, t2, "lca", True)
    total = len(full["text"])
    last = len(full["text"].rstrip(b"\n").rsplit(b"\n", 1)[0]) + 1
    return nodes, t1, t2, parent, total, (total, total - 1, last, last - 1, 0, 1, 7, 8, 4096, 4097, total + 100)


def test_capacity(mergers):
    nodes, t1, t2, parent, total, caps = capacity_jobs(mergers)
    merger, _ = mergers.get(nodes, "lca", True)
    for cap in caps:
        want = me.expected(parent, t1, t2, "lca", True, True, cap)
        assert want["info"]["overflow"] == (1 if cap < total else 0)
        out, info = run_host_form(merger, t1, t2, True, cap)
        compare(out, info, want, cap)


def test_carry_over_in_two_calls_equals_one(mergers):
    nodes, t1, t2 = mi.real()
    whole = me.expected(me.parse_nodes(nodes), t1, t2, "lowest", True)
    for cut1, cut2 in ((5000, 3000), (3000, 5000), (1, 20000), (len(t1), 100)):
        a = check(mergers, nodes, t1[:cut1], t2[:cut2], "lowest", True, False, ("first call", cut1, cut2))
        u1, u2 = a["info"]["used1"], a["info"]["used2"]
        b = check(mergers, nodes, t1[u1:], t2[u2:], "lowest", True, True, ("second call", cut1, cut2))
        assert a["text"] + b["text"] == whole["text"] and a["info"]["count"] + b["info"]["count"] == whole["info"]["count"]


def device_run(hip, merger, t1, t2, final, cap, stream):
    """the device-pointer form on buffers of the caller's; returns (out with 64 bytes behind cap, info)"""
    d1, d2, d_out, d_info = hip.malloc(len(t1) + 64), hip.malloc(len(t2) + 64), hip.malloc(cap + 64 + 16), hip.malloc(128)
    assert d1 % 16 == 0 and d2 % 16 == 0 and d_out % 16 == 0
    for d, t in ((d1, t1), (d2, t2)):
        if t:
            hip.h2d(d, np.frombuffer(t, dtype=np.uint8))
    hip.h2d(d_out, np.full(cap + 64, 0xA5, dtype=np.uint8))
    merger.merge_device(d1, len(t1), d2, len(t2), d_out, cap, d_info, final=final, stream=stream)
    assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
    info = hip.d2h(d_info, 112).view(api.MERGE_INFO_DTYPE)[0]
    out = hip.d2h(d_out, cap + 64)
    for d in (d1, d2, d_out, d_info):
        hip.free(d)
    return out, info


def test_device_pointer_form(mergers):
    hip = Hip()
    stream = hip.stream()
    nodes, t1, t2, parent, total, caps = capacity_jobs(mergers)
    merger, _ = mergers.get(nodes, "lca", True)
    for cap in caps:
        want = me.expected(parent, t1, t2, "lca", True, True, cap)
        out, info = device_run(hip, merger, t1, t2, True, cap, stream)
        compare(out, info, want, cap)
    for what, nodes, t1, t2, mode, use_score, final in mi.small_cases():
        if what in ("pairs_0", "pairs_700", "stop_two", "lca_digits_lca_s", "ragged_final0", "ragged_final1", "both_empty_final1", "long_name", "score_wide_s"):
            merger, parent = mergers.get(nodes, mode, use_score)
            want = me.expected(parent, t1, t2, mode, use_score, final)
            out, info = device_run(hip, merger, t1, t2, final, len(want["text"]) + 5, stream)
            compare(out, info, want, what)


def test_two_classifications_merged_on_one_stream(gpu_lib, golden, mergers):
    """kaiju_gpu_classify_text_to_text in MEM and in Greedy mode on the golden reads; the two texts, in device buffers, merged by
    kaiju_gpu_merge_text_device on a stream of the caller's, in every mode"""
    api, hip = gpu_lib, Hip()
    stream = hip.stream()
    index = api.Index(golden.fmi, device=0)
    nodes = mi.read(golden.nodes)
    dtax, parent, _ = mergers.tree(nodes)
    reads = mi.read(os.path.join(golden.dir, "reads.fq"))
    texts = []
    for mode in ("mem", "greedy"):
        c = api.Classifier(index, api.default_params(mode))
        texts.append(c.classify_text_to_text(dtax, reads)["text"])
        c.close()
    t1, t2 = texts
    assert t1 != t2 and t1.count(b"\n") == t2.count(b"\n") > 500
    seen = set()
    for mode in me.MODES:
        merger, _ = mergers.get(nodes, mode, False)
        want = me.expected(parent, t1, t2, mode, False)
        assert want["info"]["stop_pair"] == me.NO_PAIR and want["info"]["count_c12"] > 300
        out, info = device_run(hip, merger, t1, t2, True, len(want["text"]) + 5, stream)
        compare(out, info, want, mode)
        seen.add(want["text"])
    assert len(seen) >= 2                                        # the two runs disagree somewhere, and the modes about it


def test_refusals(gpu_lib, mergers):
    api, hip = gpu_lib, Hip()
    L = api.lib()
    merger, _ = mergers.get(mi.SMALL_TREE, "lca", False)
    d = hip.malloc(512)
    hip.memset(d, 512)
    args = lambda t1, n1, t2, n2, out: (merger._h, t1, n1, t2, n2, 1, out, 64, d + 384, None)
    assert L.kaiju_gpu_merge_text_device(*args(d, 16, d + 64, 16, d + 128)) == 0
    assert L.kaiju_gpu_merge_text_device(*args(d + 4, 16, d + 64, 16, d + 128)) == -1     # KAIJU_GPU_ERR_ARG: text 1 is misaligned
    assert b"16-byte aligned" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_merge_text_device(*args(d, 16, d + 68, 16, d + 128)) == -1         # ... text 2
    assert L.kaiju_gpu_merge_text_device(*args(d, 16, d + 64, 16, d + 132)) == -1         # ... the output
    assert L.kaiju_gpu_merge_text_device(*args(d, 0xfffffff1, d + 64, 16, d + 128)) == -1 # more than kji::kMaxBytes
    assert b"2^32" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_merge_text_device(*args(d, 16, d + 64, 0xfffffff1, d + 128)) == -1
    assert L.kaiju_gpu_merge_text_device(*args(d, 16, None, 16, d + 128)) == -1
    assert L.kaiju_gpu_merge_text_device(*args(d, 16, d + 64, 16, d + 128)[:8], None, None) == -1
    assert L.kaiju_gpu_merge_text_device(None, d, 16, d + 64, 16, 1, d + 128, 64, d + 384, None) == -1
    h = C.c_void_p()
    assert L.kaiju_gpu_merger_create(None, 0, api.MERGE_LCA, 0, C.byref(h)) == -1 and b"tree" in L.kaiju_gpu_last_error()   # -c lca without -t
    assert L.kaiju_gpu_merger_create(None, 0, 4, 0, C.byref(h)) == -1 and L.kaiju_gpu_merger_create(None, 0, 0, 0, None) == -1
    info = np.zeros(1, dtype=api.MERGE_INFO_DTYPE)
    assert L.kaiju_gpu_merge_text(merger._h, None, 5, None, 0, 1, None, 0, info.ctypes.data) == -1
    assert L.kaiju_gpu_merge_text(merger._h, None, 0, None, 0, 1, None, 0, info.ctypes.data) == 0 and int(info[0]["text_bytes"]) == 0 and int(info[0]["count"]) == 0
    assert hip.L.hipDeviceSynchronize() == 0
    hip.free(d)


def test_pass_times(gpu_lib, mergers, monkeypatch):
    """kaiju_gpu_merge_pass_ms: the events of a merger created with KAIJU_GPU_MERGE_TIMES=1, refused by any other"""
    api = gpu_lib
    L = api.lib()
    L.kaiju_gpu_merge_pass_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    ms = (C.c_float * 6)(*([-1.0] * 6))
    plain, _ = mergers.get(None, "1", False)
    assert L.kaiju_gpu_merge_pass_ms(plain._h, ms, 6) == -7 and b"KAIJU_GPU_MERGE_TIMES" in L.kaiju_gpu_last_error()      # KAIJU_GPU_ERR_UNSUPPORTED
    monkeypatch.setenv("KAIJU_GPU_MERGE_TIMES", "1")
    timed = api.Merger(None, "1", False)
    monkeypatch.delenv("KAIJU_GPU_MERGE_TIMES")
    t1, t2 = mi.counted(700)
    got, info = timed.merge(t1, t2)
    assert got == me.expected({}, t1, t2, "1", False)["text"]
    assert L.kaiju_gpu_merge_pass_ms(timed._h, ms, 6) == 0 and all(0.0 <= x < 1000.0 for x in ms) and sum(ms) > 0.0
    assert L.kaiju_gpu_merge_pass_ms(timed._h, None, 6) == -1 and L.kaiju_gpu_merge_pass_ms(None, ms, 6) == -1
    timed.close()


def test_merger_on_another_device(gpu_lib, mergers):
    """a merger works on its device, whatever device the caller has current; buffers that lie on another device are refused"""
    api = gpu_lib
    if api.device_count() < 2:
        pytest.skip("one device visible")
    hip = Hip()
    _, t1, t2 = mi.odd()
    merger = api.Merger(None, "1", True, device=1)
    got, _ = merger.merge(t1, t2)
    assert got == mi.odd_output("1", True)[0]
    assert hip.L.hipSetDevice(0) == 0
    d = hip.malloc(512)                                      # on device 0
    hip.memset(d, 512)
    assert api.lib().kaiju_gpu_merge_text_device(merger._h, d, 16, d + 64, 16, 1, d + 128, 64, d + 384, None) == -1
    assert b"another device" in api.lib().kaiju_gpu_last_error()
    hip.free(d)
    merger.close()


# ---- the command line program -------------------------------------------------------------------------------------------
def cli(args, block=None):
    env = dict(os.environ)
    env.pop("KAIJU_MERGE_BLOCK", None)
    if block:
        env["KAIJU_MERGE_BLOCK"] = str(block)
    exe = build.build_merge_cli()
    return subprocess.run([exe] + args, env=env, capture_output=True, timeout=CLI_TIMEOUT)


def summary_of(stderr):
    text = stderr.decode("latin-1")
    return text[text.rindex("Number of all reads in input:"):]


def cli_jobs(which, every_variant):
    """(arguments, (the tool's output, its summary)) of a set of fixtures; every_variant: all of -c x -s, else four of the eight"""
    odd, real = os.path.join(mi.MERGE, "odd"), os.path.join(mi.MERGE, "real")
    variants = mi.VARIANTS if every_variant else [("lca", True), ("lowest", False), ("1", True), ("2", False)]
    jobs = []
    if which == "odd":
        for mode, s in variants:
            jobs.append((["-i", os.path.join(odd, "in1.tsv"), "-j", os.path.join(odd, "in2.tsv"), "-t", os.path.join(odd, "nodes.dmp"), "-c", mode] + (["-s"] if s else []),
                         mi.odd_output(mode, s)))
        for s in (False, True):
            jobs.append((["-i", os.path.join(odd, "in1.tsv"), "-j", os.path.join(odd, "in2.tsv"), "-c", "lowest", "-d"] + (["-s"] if s else []), mi.odd_output("lowest", s, tree=False)))
    elif which == "real":
        for mode, s in variants:
            jobs.append((["-i", os.path.join(mi.GOLDEN, "ref_mem_1.tsv"), "-j", os.path.join(mi.GOLDEN, "ref_greedy_1.tsv"), "-t", os.path.join(mi.GOLDEN, "nodes.dmp"), "-c", mode] +
                         (["-s"] if s else []), mi.real_output(mode, s)))
    else:
        names = mi.stop_names()
        for name in names[:len(names) // 2] if which == "stops_a" else names[len(names) // 2:]:
            _, _, s, text, summary = mi.stop_case(name)
            d = os.path.join(mi.MERGE, "stops", name)
            jobs.append((["-i", d + ".1.tsv", "-j", d + ".2.tsv", "-c", "1"] + (["-s"] if s else []), (text, summary)))
    return jobs


@pytest.mark.parametrize("which", ["odd", "real", "stops_a", "stops_b"])
@pytest.mark.parametrize("block", [512, None])
def test_cli_against_the_tools_files(gpu_lib, tmp_path, block, which):
    """the program on the three sets of fixtures, in pieces of 512 bytes a side and with the default block: the output file and
    the summary of -v are the tool's, the status is 0 also where the run stops.  (A start of the program costs a third of a
    second: the sets are cases of their own, and with the default block, where one piece holds the files, odd/ and real/ run
    in four of the eight variants.)"""
    jobs = cli_jobs(which, block is not None)
    assert len(jobs) == {"odd": 10 if block else 6, "real": 8 if block else 4, "stops_a": 13, "stops_b": 13}[which]
    o = str(tmp_path / "out.tsv")
    for args, (text, summary) in jobs:
        r = cli(args + ["-v", "-o", o], block)
        assert r.returncode == 0 and r.stdout == b"", (args, r.returncode, r.stderr[-500:])
        with open(o, "rb") as f:
            assert f.read() == text, args
        assert summary_of(r.stderr) == summary, args
    if which == "odd":
        r = cli(jobs[0][0], block)                            # standard output, no summary
        assert r.returncode == 0 and r.stdout == jobs[0][1][0] and b"Number of all reads" not in r.stderr


def test_cli_statuses(gpu_lib, tmp_path):
    a, b = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    with open(a, "wb") as f:
        f.write(b"C\ta\t4\t1\nC\tb\t4\t9007199254740993\nC\tc\t4\t1\n")
    with open(b, "wb") as f:
        f.write(b"C\ta\t5\t1\nC\tb\t5\t9007199254740992\nC\tc\t5\t1\n")
    r = cli(["-i", a, "-j", b, "-c", "1", "-s", "-v"])
    assert r.returncode == 3 and r.stdout == b"C\ta\t4\t1\n" and b"line 2" in r.stderr and summary_of(r.stderr).startswith("Number of all reads in input:\t         2\n")
    r = cli(["-i", a, "-j", b, "-c", "1"], block=16)
    assert r.returncode == 0 and r.stdout == b"C\ta\t4\nC\tb\t4\nC\tc\t4\n"
    for args, word in ((["-i", a, "-j", b], b"LCA mode requires"), (["-i", a, "-j", b, "-c", "x"], b"-c must be"), (["-j", b, "-c", "1"], b"-i option"), (["-i", a, "-c", "1"], b"-j option"),
                       (["-i", str(tmp_path / "none.tsv"), "-j", b, "-c", "1"], b"none.tsv"), (["-i", a, "-j", b, "-t", str(tmp_path / "none.dmp")], b"none.dmp"),
                       (["-i", a, "-j", b, "-c", "1", "-o", str(tmp_path / "no" / "dir" / "o.tsv")], b"o.tsv"), (["-h"], b"usage")):
        r = cli(args)
        assert r.returncode == 1 and word in r.stderr and r.stdout == b"", (args, r.returncode, r.stderr[-300:])
