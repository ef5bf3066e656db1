"""The Krona text on the device (kaiju_amd/csrc/krona.hip): kaiju_gpu_krona_text / _text_device over the counts of tallies, on
the fixtures the reference tool read and on the shapes at which the passes can go wrong, against tests/krona_expect.py byte for
byte and against the files the unmodified tool wrote as sorted lines; two tallies, reset, repeated calls; capacities; the
device-pointer form behind the formatter and the tally on one stream of the caller's; the refusals; and
kaiju_amd/bin/kaiju2krona against the tool's files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import krona_expect as ke
import krona_inputs as ki
import table_expect as te
import table_inputs as ti
from kaiju_amd import api, build
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

CLI_TIMEOUT = 120       # seconds per run of the command line program
N_TAXA = ti.WIDE_TAXA    # species of the wide tree
DEPTH = 64               # nodes of the chain


class World:
    """a tree on device 0 with the model's reading of it, two tallies and a Krona object per list of ranks"""

    def __init__(self, nodes, names, mode="name"):
        self.tree = te.Tree(ti.read(nodes), ti.read(names))
        self.host = api.TaxonNames(nodes, names, mode)
        self.dev = api.DeviceTaxonNames(self.host, 0)
        self.tally = [api.Tally(self.dev), api.Tally(self.dev)]
        self.kronas = {}

    def krona(self, ranks=None):
        if ranks not in self.kronas:
            self.kronas[ranks] = api.Krona(self.dev, ranks)
        return self.kronas[ranks]

    def count(self, text, more=None):
        """text into the first tally (and `more` into the second): ({taxon: reads}, unclassified lines) of the model"""
        for t in self.tally:
            t.reset()
        self.tally[0].add(text)
        if more is not None:
            self.tally[1].add(more)
        return ke.direct_of(self.tree, [text] + ([more] if more is not None else []))

    def close(self):
        for k in self.kronas.values():
            k.close()
        for t in self.tally:
            t.close()
        self.dev.close()
        self.host.close()


@pytest.fixture(scope="module")
def worlds(gpu_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("krona_gpu")
    for name, (nodes, names) in (("wide", ti.many_taxa_tree(N_TAXA)), ("chain", ki.chain_tree(DEPTH))):
        (d / (name + "_nodes.dmp")).write_bytes(nodes)
        (d / (name + "_names.dmp")).write_bytes(names)
    w = {"fixture": World(ki.NODES, ki.NAMES), "real": World(ti.REAL_NODES, ti.REAL_NAMES, "path"),      # (names of any mode serve)
         "wide": World(str(d / "wide_nodes.dmp"), str(d / "wide_names.dmp")), "chain": World(str(d / "chain_nodes.dmp"), str(d / "chain_names.dmp"))}
    yield w
    for x in w.values():
        x.close()


def same(world, direct, n_u, unclassified, ranks, what, tallies=None, out_cap=None):
    want = ke.expected(world.tree, direct, n_u, unclassified, ranks, out_cap)
    got, info = world.krona(ranks).text(tallies or world.tally, unclassified=unclassified, out_cap=out_cap)
    assert got == want["written"], what
    for f in ke.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f, int(info[f]), want["info"][f])
    assert int(info["reserved"]) == 0
    return got


# ---- 1. the fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ki.SETS))
def test_fixtures_against_the_model_and_the_tools_files(worlds, name):
    u, ranks = ki.SETS[name]
    for label, _, text in ki.cases():
        w = worlds["real" if label == "real" else "fixture"]
        direct, n_u = w.count(text)
        got = same(w, direct, n_u, u, ranks, (label, name))
        assert ke.sorted_lines(got) == ke.sorted_lines(ki.golden(label, name)), (label, name)


# ---- 2. the shapes of the passes ------------------------------------------------------------------------------------------
def test_more_taxa_with_reads_than_one_block_compacts(worlds):
    """selection and scan cross blocks: 3001 of 4000 species and every third genus hold reads, the species in 1 .. 4 lines"""
    w = worlds["wide"]
    text = b"".join(ti.line_of(1000 + k, k) * (1 + k % 4) for k in range(N_TAXA) if k % 4 != 3) + b"".join(ti.line_of(100000 + k, k) for k in range(0, N_TAXA, 3))
    text += b"U\tu\t0\n" * 11 + ti.line_of(1, 0) * 3
    direct, n_u = w.count(text)
    assert len(direct) > 4000 and n_u == 11
    for u, ranks in ((True, None), (False, "species"), (True, "genus,no rank")):
        got = same(w, direct, n_u, u, ranks, (u, ranks))
        assert got.count(b"\n") == len(direct) - (N_TAXA + 2) // 3 + (1 if u else 0)          # the genera have no names: no lines
    # every capacity class once more on many short lines
    full = ke.expected(w.tree, direct, n_u, True, None)["text"]
    for cap in (len(full) - 1, 4096, 4097, 70001):
        same(w, direct, n_u, True, None, cap, out_cap=cap)


def test_a_deep_chain_with_names_of_1_and_of_200_bytes(worlds):
    """one line is longer than a write block's share, and the lines cross every 16-byte phase"""
    w = worlds["chain"]
    text = b"".join(ti.line_of(tid, 0) * (1 + tid % 5) for tid in w.tree.nodes)
    direct, n_u = w.count(text)
    for ranks in (None, "genus,no rank", "species"):
        got = same(w, direct, n_u, False, ranks, ranks)
        assert max(len(x) for x in got.split(b"\n")) > (20 if ranks == "species" else 4096)      # (the long names are those of the genera)
    starts = {m.start() % 16 for m in __import__("re").finditer(b"\n", same(w, direct, n_u, False, None, "phases"))}
    assert len(starts) > 8
    full = ke.expected(w.tree, direct, 0, False, None)["text"]
    for cap in (len(full) // 2, 4096, 5000):
        same(w, direct, 0, False, None, cap, out_cap=cap)


def test_counts_at_the_digit_boundaries(worlds):
    """9, 10, 999 999 and 1 000 000 reads, from texts of 6-byte lines"""
    w = worlds["chain"]
    line = lambda tid: b"C\tr\t%d\n" % tid
    text = line(3) * 9 + line(4) * 10 + line(5) * 999999 + line(6) * 1000000 + b"U\tr\t0\n" * 99
    assert len(text) == 6 * (9 + 10 + 999999 + 1000000 + 99)
    for t in w.tally:
        t.reset()
    info = w.tally[1].add(text)
    assert int(info["n_total"]) == len(text) // 6
    direct, n_u = {3: 9, 4: 10, 5: 999999, 6: 1000000}, 99
    got = same(w, direct, n_u, True, None, "digits")
    assert sorted(int(x.split(b"\t")[0]) for x in got.split(b"\n")[:-1]) == [9, 10, 99, 999999, 1000000]


# ---- 3. tallies, reset, repetition -----------------------------------------------------------------------------------------
def test_two_tallies_a_reset_and_two_calls_in_a_row(worlds):
    w = worlds["fixture"]
    text = ti.read(ki.FILES["odd"])
    cut = text.index(b"\n", len(text) // 3) + 1
    direct, n_u = w.count(text[:cut], text[cut:] + b"\n" + ti.read(ki.FILES["allu"]))
    two = same(w, direct, n_u, True, None, "two tallies")
    again = same(w, direct, n_u, True, None, "again")
    assert two == again
    direct1, n_u1 = w.count(text + b"\n" + ti.read(ki.FILES["allu"]))
    assert (direct1, n_u1) == (direct, n_u)
    assert same(w, direct, n_u, True, None, "one tally of the joined text", tallies=[w.tally[0]]) == two
    assert same(w, direct, n_u, True, None, "the second one is empty") == two
    # the counts stay: the tally's own result is what it was
    ent, tot = w.tally[0].result()
    assert int(tot["n_unclassified"]) == n_u and sum(int(e["direct"]) for e in ent) == sum(direct.values()) - direct[1]
    w.tally[0].reset()
    assert same(w, {}, 0, True, None, "after the reset") == b""
    direct, n_u = w.count(ti.read(ki.FILES["allu"]))
    assert same(w, direct, n_u, True, None, "allu") == b"7\tUnclassified\n"
    # the same tally twice counts twice
    d2 = {t: 2 * c for t, c in ke.direct_of(w.tree, [text])[0].items()}
    w.count(text)
    same(w, d2, 0, False, None, "twice", tallies=[w.tally[0], w.tally[0]])


# ---- 4. capacities, with the bytes behind untouched ------------------------------------------------------------------------
def test_capacities_leave_the_bytes_behind_untouched(worlds):
    hip = Hip()
    w = worlds["fixture"]
    direct, n_u = w.count(ti.read(ki.FILES["odd"]))
    full = ke.expected(w.tree, direct, n_u, True, None)
    size = len(full["text"])
    lines = full["text"].split(b"\n")
    inside = len(lines[0]) + 1 + len(lines[1]) // 2
    d_out, d_info = hip.malloc(size + 256), hip.malloc(256)
    for cap in (0, inside, size - 1, size, size + 100):
        want = ke.expected(w.tree, direct, n_u, True, None, cap)
        hip.h2d(d_out, np.full(size + 256, 0xA5, dtype=np.uint8))
        hip.h2d(d_info, np.full(256, 0xA5, dtype=np.uint8))
        w.krona().text_device(w.tally, d_out if cap else 0, cap, d_info, unclassified=True)
        assert hip.L.hipDeviceSynchronize() == 0
        out, got = bytes(hip.d2h(d_out, size + 256)), hip.d2h(d_info, 256)
        n = len(want["written"])
        assert out[:n] == want["written"] and out[n:] == b"\xa5" * (size + 256 - n), cap
        assert np.all(got[64:] == 0xA5)
        info = got[:64].view(api.KRONA_INFO_DTYPE)[0]
        for f in ke.INFO_FIELDS:
            assert int(info[f]) == want["info"][f], (cap, f)
    hip.free(d_out)
    hip.free(d_info)


# ---- 5. the device-pointer form ------------------------------------------------------------------------------------------
def test_formatter_tally_and_krona_on_one_stream(gpu_lib, golden, worlds):
    """kaiju_gpu_format_compact_device writes the lines, kaiju_gpu_tally_add_text_device counts them where they lie and
    kaiju_gpu_krona_text_device writes the Krona text from the counts: device pointers only, one stream, one synchronisation"""
    hip = Hip()
    stream = hip.stream()
    w = worlds["real"]
    index = api.Index(golden.fmi, device=0)
    tax = api.Taxonomy(golden.nodes)
    dtax = api.DeviceTaxonomy(tax, 0)
    c = api.Classifier(index, api.default_params("greedy"))
    fastq = ti.read(os.path.join(ti.GOLDEN, "reads.fq"))
    r = c.classify_text_compact(dtax, fastq)
    recs, off, names = r["compact"], np.ascontiguousarray(r["off"], dtype=np.uint64), np.zeros(len(r["compact"]), dtype=api.NAME_SPAN_DTYPE)
    names["pos"], names["len"] = r["names"][:, 0], r["names"][:, 1]
    n, mid_cap, out_cap = len(recs), api.format_bound(len(fastq), len(recs)), 1 << 16
    text = np.frombuffer(fastq + b"\0", dtype=np.uint8)
    bufs = [hip.malloc(a.nbytes + 16) for a in (recs, off, text, names)]
    for d, a in zip(bufs, (recs, off, text, names)):
        hip.h2d(d, a)
    d_recs, d_off, d_text, d_names = bufs
    d_mid, d_finfo, d_tinfo, d_out, d_info = hip.malloc(mid_cap + 64), hip.malloc(64), hip.malloc(64), hip.malloc(out_cap + 64), hip.malloc(256)
    hip.ck(hip.L.hipMemset(C.c_void_p(d_mid), 10, C.c_size_t(mid_cap + 64)))
    hip.h2d(d_out, np.full(out_cap + 64, 0xA5, dtype=np.uint8))
    hip.h2d(d_info, np.full(256, 0xA5, dtype=np.uint8))
    for t in w.tally:
        t.reset()
    c.format_compact_device(d_recs, d_off, n, d_text, len(fastq), d_names, d_mid, mid_cap, d_finfo, paired=False, stream=stream)
    w.tally[0].add_device(d_mid, mid_cap, d_tinfo, final=True, stream=stream)
    w.krona().text_device([w.tally[0]], d_out, out_cap, d_info, unclassified=True, stream=stream)
    assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
    lines = bytes(hip.d2h(d_mid, mid_cap))
    direct, n_u = ke.direct_of(w.tree, [lines])
    want = ke.expected(w.tree, direct, n_u, True, None, out_cap)
    assert len(direct) > 10 and not want["info"]["overflow"]
    out, got = bytes(hip.d2h(d_out, out_cap + 64)), hip.d2h(d_info, 256)
    size = len(want["text"])
    assert out[:size] == want["text"] and out[size:] == b"\xa5" * (out_cap + 64 - size)
    assert np.all(got[64:] == 0xA5)
    info = got[:64].view(api.KRONA_INFO_DTYPE)[0]
    for f in ke.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], f
    for d in bufs + [d_mid, d_finfo, d_tinfo, d_out, d_info]:
        hip.free(d)
    c.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(gpu_lib, worlds):
    hip = Hip()
    L, w = api.lib(), worlds["fixture"]
    k, t = w.krona(), w.tally[0]
    w.count(ti.read(ki.FILES["odd"]))
    d = hip.malloc(4096)
    hip.memset(d, 4096)
    one = (C.c_void_p * 1)(t._h)
    five = (C.c_void_p * 5)(*[t._h] * 5)
    assert L.kaiju_gpu_krona_text_device(k._h, one, 1, 1, d, 2048, d + 2048, None) == 0
    assert L.kaiju_gpu_krona_text_device(k._h, one, 1, 1, d + 4, 2048, d + 2048, None) == -1           # KAIJU_GPU_ERR_ARG: the output is misaligned
    assert b"16-byte aligned" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_krona_text_device(k._h, one, 0, 1, d, 2048, d + 2048, None) == -1
    assert b"tallies" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_krona_text_device(k._h, five, 5, 1, d, 2048, d + 2048, None) == -1
    assert L.kaiju_gpu_krona_text_device(k._h, five, 4, 1, d, 2048, d + 2048, None) == 0
    assert L.kaiju_gpu_krona_text_device(k._h, None, 1, 1, d, 2048, d + 2048, None) == -1
    assert L.kaiju_gpu_krona_text_device(k._h, one, 1, 1, d, 2048, None, None) == -1
    assert L.kaiju_gpu_krona_text_device(k._h, one, 1, 1, None, 2048, d + 2048, None) == -1
    assert L.kaiju_gpu_krona_text_device(None, one, 1, 1, d, 2048, d + 2048, None) == -1
    other = (C.c_void_p * 1)(worlds["real"].tally[0]._h)                                               # a tally of another tree
    assert L.kaiju_gpu_krona_text_device(k._h, other, 1, 1, d, 2048, d + 2048, None) == -1
    assert b"other taxon names" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_krona_create(None, None, None) == -1
    h = C.c_void_p()
    assert L.kaiju_gpu_krona_create(w.dev._h, ",".join("r%d" % i for i in range(65)).encode(), C.byref(h)) == -1 and not h.value
    assert b"list of ranks" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_krona_create(w.dev._h, ",".join("r%d" % i for i in range(64)).encode(), C.byref(h)) == 0
    L.kaiju_gpu_krona_free(h)
    info = np.zeros(1, dtype=api.KRONA_INFO_DTYPE)
    assert L.kaiju_gpu_krona_text(k._h, one, 1, 1, None, 5, info.ctypes.data) == -1
    assert L.kaiju_gpu_krona_text(k._h, one, 1, 1, None, 0, None) == -1
    ms = np.zeros(5, dtype=np.float32)
    assert L.kaiju_gpu_krona_pass_ms(k._h, ms.ctypes.data, 5) == -7                                    # KAIJU_GPU_ERR_UNSUPPORTED: created without the switch
    assert hip.L.hipDeviceSynchronize() == 0
    hip.free(d)


def test_pass_times_with_the_switch(worlds, monkeypatch):
    monkeypatch.setenv("KAIJU_GPU_KRONA_TIMES", "1")
    w = worlds["fixture"]
    k = api.Krona(w.dev)
    w.count(ti.read(ki.FILES["odd"]))
    k.text(w.tally)
    ms = k.pass_ms()
    assert len(ms) == api.KRONA_PASSES and np.all(ms >= 0) and np.all(np.isfinite(ms))
    k.close()


# ---- 7. the command line program -----------------------------------------------------------------------------------------
def cli(args, cwd, block=None):
    env = dict(os.environ)
    env.pop("KAIJU_TABLE_BLOCK", None)
    if block:
        env["KAIJU_TABLE_BLOCK"] = str(block)
    return subprocess.run([build.build_krona_cli()] + args, env=env, cwd=cwd, capture_output=True, timeout=CLI_TIMEOUT)


@pytest.mark.parametrize("name", sorted(ki.SETS))
def test_cli_against_the_tools_files(gpu_lib, tmp_path, name):
    out = str(tmp_path / "out.txt")
    for label, path in ki.FILES.items():
        r = cli(["-t", "nodes.dmp", "-n", "names.dmp", "-i", path, "-o", out] + ki.argv_of(name), ki.KRONA, block=4096)
        assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
        assert ke.sorted_lines(ti.read(out)) == ke.sorted_lines(ki.golden(label, name)), label
        u, ranks = ki.SETS[name]
        assert ti.read(out) == ke.text_of(ki.fixture_tree(), [ti.read(path)], u, ranks), label
        if label == "odd":                                   # one line per reason
            assert r.stderr.count(b"\n") == 3 and b"bad taxon id" in r.stderr and b"taxonomic tree file nodes.dmp" in r.stderr and b"2 taxon ids with 2 reads" in r.stderr


def test_cli_on_the_golden_reads_and_its_failures(gpu_lib, tmp_path):
    out = str(tmp_path / "out.txt")
    real = os.path.join(ki.KRONA, "real")
    tree = ["-t", "../../nodes.dmp", "-n", "../../names/golden/names.dmp"]
    for name in ("u", "l4"):
        r = cli(tree + ["-i", "../../ref_mem_1.tsv", "-o", out, "-v"] + ki.argv_of(name), real, block=1000)
        assert r.returncode == 0 and b"Processing ../../ref_mem_1.tsv" in r.stderr, r.stderr[-2000:]
        assert ke.sorted_lines(ti.read(out)) == ke.sorted_lines(ki.golden("real", name))
    r = cli(tree + ["-i", "no_such_file.tsv", "-o", out], real)
    assert r.returncode == 1 and b"no_such_file.tsv" in r.stderr
    r = cli(["-t", "no_such_nodes.dmp", "-n", "../../names/golden/names.dmp", "-i", "../../ref_mem_1.tsv", "-o", out], real)
    assert r.returncode == 1 and b"no_such_nodes.dmp" in r.stderr
    r = cli(tree + ["-i", "../../ref_mem_1.tsv"], real)
    assert r.returncode == 1 and b"usage:" in r.stderr
