"""The tally on the device (kaiju_amd/csrc/tally.hip): kaiju_gpu_tally_add_text / _result on the fixtures the reference tool
read and on the shapes at which the count pass can go wrong, against tests/table_expect.py; api.table_text over the device's
counts against the tables the unmodified tool wrote; texts added in pieces, reset, and what earlier calls leave behind; the
device-pointer form behind kaiju_gpu_format_compact_device on one stream of the caller's; the refusals; and
kaiju_amd/bin/kaiju2table against the tool's files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import table_expect as te
import table_inputs as ti
from kaiju_amd import api, build
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

TILE = 4096
CLI_TIMEOUT = 120       # seconds per run of the command line program
N_TAXA = ti.WIDE_TAXA    # species of the wide tree: more than a block's table holds


class World:
    """a tree on device 0 with the model's reading of it"""

    def __init__(self, api, nodes, names):
        self.tree = te.Tree(ti.read(nodes), ti.read(names))
        self.host = api.TaxonNames(nodes, names)
        self.dev = api.DeviceTaxonNames(self.host, 0)
        self.tally = api.Tally(self.dev)

    def close(self):
        self.tally.close()
        self.dev.close()
        self.host.close()


@pytest.fixture(scope="module")
def worlds(gpu_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("tally_gpu")
    nodes, names = ti.many_taxa_tree(N_TAXA)
    (d / "nodes.dmp").write_bytes(nodes)
    (d / "names.dmp").write_bytes(names)
    w = {"fixture": World(gpu_lib, ti.NODES, ti.NAMES), "real": World(gpu_lib, ti.REAL_NODES, ti.REAL_NAMES),
         "wide": World(gpu_lib, str(d / "nodes.dmp"), str(d / "names.dmp"))}
    yield w
    for x in w.values():
        x.close()


def same_info(info, want, what, fields=te.INFO_FIELDS):
    for f in fields:
        assert int(info[f]) == want[f], (what, f, int(info[f]), want[f])


def listed(ent):
    assert not np.any(ent["reserved"])
    return [(int(e["taxon"]), int(e["direct"]), int(e["summed"]), int(e["virus"])) for e in ent]


def check(world, texts, what, tally=None):
    """the texts added one behind the other, all but the last with final=0 and the rest carried as a caller would: every call's
    info, the totals and the entries are the model's"""
    t = tally or world.tally
    t.reset()
    carry, whole = b"", b"".join(texts)
    for k, text in enumerate(texts):
        final = k + 1 == len(texts)
        info = t.add(carry + text, final)
        same_info(info, te.count_text(world.tree, carry + text, final)[0], (what, "call", k))
        carry = (carry + text)[int(info["used"]):]
    totals, entries = te.tally(world.tree, [whole])
    ent, tot = t.result()
    same_info(tot, totals, what, te.INFO_FIELDS[2:])
    assert int(tot["used"]) == len(whole), what
    assert listed(ent) == entries, what
    return ent, tot


# ---- 1. the fixtures ----------------------------------------------------------------------------------------------------
def test_fixtures_counts_and_every_golden_table(worlds):
    for world, files, sub in ((worlds["fixture"], ti.fixture_texts(), ""), (worlds["real"], ti.real_texts(), "real")):
        counted = [(label, check(world, [text], label)) for label, text in files]
        for name, opt in ti.SETS.items():
            got = te.HEADER + b"".join(api.table_text(world.host, ent, tot, label, **opt) for label, (ent, tot) in counted)
            assert got == ti.read(os.path.join(ti.TABLE, sub, "out_%s.tsv" % name)), (sub, name)


# ---- 2. the shapes of the count pass -------------------------------------------------------------------------------------
def shapes():
    line = ti.line_of
    rng = np.random.default_rng(11)
    S = {
        "one_taxon_x64": b"".join(line(1007, k) for k in range(64)),
        "64_taxa": b"".join(line(1000 + k, k) for k in range(64)),
        "5_taxa_per_wavefront": b"".join(line(1000 + k % 5, k) for k in range(256)),           # one more than the grouping rounds of =wave
        "many_taxa_in_three_sweeps": b"".join(line(1000 + (k * 7) % N_TAXA, k) for k in range(3 * 256 + 19)),
        "skewed_and_odd": ti.random_text(rng, te.Tree(*ti.many_taxa_tree(N_TAXA)), 3000),
        "only_newlines": b"\n" * 5000,
        "one_line_longer_than_a_tile": b"C\t" + b"n" * 5000 + b"\t1003\n" + line(1003, 1),
        "no_final_newline": line(1001) + line(1002)[:-1],
    }
    body = b"".join(line(1000 + k % 9, k) for k in range(400))
    S["exactly_one_tile"] = body[:TILE - 9] + b"C\tpad\t1004"[:8] + b"\n"
    assert len(S["exactly_one_tile"]) == TILE
    S["one_tile_and_a_byte"] = S["exactly_one_tile"] + b"C"
    last = b"C\tspans_two_tiles\t1005\n"
    S["last_line_spans_two_tiles"] = body[:TILE - 9] + last
    assert len(S["last_line_spans_two_tiles"]) > TILE > len(S["last_line_spans_two_tiles"]) - len(last)
    # more lines than one sweep of the count pass's grid looks at (4096 blocks of 256): the lines behind are its second sweep
    S["second_sweep_of_the_grid"] = b"\n" * (4096 * 256) + b"".join(line(1000 + k % 70, k) for k in range(300))
    # more taxa in one block than its table holds: the lanes that find no room add for themselves (tests/test_tally_emu.py
    # counts them on the host)
    S.update(ti.table_shapes())
    return S


def test_shapes_of_the_count_pass(worlds):
    for what, text in shapes().items():
        check(worlds["wide"], [text], what)


@pytest.mark.parametrize("way", ["lane", "wave"])
def test_the_other_ways_of_counting_give_the_same(worlds, monkeypatch, way):
    """KAIJU_GPU_TALLY_COUNT=lane / =wave: the two ways the table of a block was measured against"""
    monkeypatch.setenv("KAIJU_GPU_TALLY_COUNT", way)
    t = api.Tally(worlds["wide"].dev)
    S = shapes()
    for what in ("one_taxon_x64", "64_taxa", "5_taxa_per_wavefront", "many_taxa_in_three_sweeps", "skewed_and_odd", "second_sweep_of_the_grid", "one_block_3600_taxa"):
        check(worlds["wide"], [S[what]], what, tally=t)
    t.close()


# ---- 3. accumulation -----------------------------------------------------------------------------------------------------
def test_three_calls_cut_inside_lines_equal_one(worlds):
    text = ti.fixture_texts()[0][1]
    a, b = 777, 6001                                        # inside the short lines, inside the long one
    assert text[a - 1:a] != b"\n" and text[b - 1:b] != b"\n"
    one = check(worlds["fixture"], [text], "one call")
    three = check(worlds["fixture"], [text[:a], text[a:b], text[b:]], "three calls")
    assert listed(one[0]) == listed(three[0])


def test_reset_gives_what_a_fresh_tally_gives(worlds):
    w = worlds["fixture"]
    (_, first), (_, second) = ti.real_texts()[0], ti.fixture_texts()[0]
    w.tally.reset()
    w.tally.add(first)
    w.tally.add(second)
    both, tot = w.tally.result()
    totals, direct = {}, {}
    for text in (first, second):
        te.add_counts(totals, direct, *te.count_text(w.tree, text))
    assert listed(both) == te.entries_of(w.tree, direct)
    same_info(tot, totals, "two texts")
    w.tally.reset()
    w.tally.add(second)
    again = w.tally.result()
    fresh = api.Tally(w.dev)
    fresh.add(second)
    new = fresh.result()
    fresh.close()
    assert listed(again[0]) == listed(new[0]) == te.tally(w.tree, [second])[1]
    assert again[1].tobytes() == new[1].tobytes()


def test_what_earlier_calls_left_in_the_scratch_changes_nothing(worlds):
    """the line tables of a larger text with a line at every byte, the entries of a result with many nodes: a later, smaller
    call reads none of it"""
    w = worlds["wide"]
    small = shapes()["no_final_newline"]
    for poison in (b"\n" * 300000, b"".join(ti.line_of(1000 + k % N_TAXA, k) for k in range(20000)), b"C\tx\t1001" * 9000):
        w.tally.reset()
        w.tally.add(poison)
        w.tally.result()
        check(w, [small], "after %d bytes" % len(poison))
        check(w, [b""], "nothing after %d bytes" % len(poison))


# ---- 4. the device-pointer form ------------------------------------------------------------------------------------------
def test_formatter_and_tally_on_one_stream(gpu_lib, golden, worlds):
    """kaiju_gpu_format_compact_device writes the lines, kaiju_gpu_tally_add_text_device counts them where they lie: no host
    round trip between the two.  The buffer between them is filled with newlines first and handed over whole - lines of
    length 0 count nowhere"""
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
    n, mid_cap = len(recs), api.format_bound(len(fastq), len(recs))
    text = np.frombuffer(fastq + b"\0", dtype=np.uint8)
    bufs = [hip.malloc(a.nbytes + 16) for a in (recs, off, text, names)]
    for d, a in zip(bufs, (recs, off, text, names)):
        hip.h2d(d, a)
    d_recs, d_off, d_text, d_names = bufs
    d_mid, d_finfo, d_info = hip.malloc(mid_cap + 64), hip.malloc(64), hip.malloc(256)
    assert d_mid % 16 == 0
    hip.ck(hip.L.hipMemset(C.c_void_p(d_mid), 10, C.c_size_t(mid_cap + 64)))
    hip.h2d(d_info, np.full(256, 0xA5, dtype=np.uint8))
    w.tally.reset()
    c.format_compact_device(d_recs, d_off, n, d_text, len(fastq), d_names, d_mid, mid_cap, d_finfo, paired=False, stream=stream)
    w.tally.add_device(d_mid, mid_cap, d_info, final=True, stream=stream)
    assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
    mid = bytes(hip.d2h(d_mid, mid_cap + 64))
    lines = mid[:mid_cap]
    assert lines.count(b"\n") > n and lines.rstrip(b"\n").count(b"\n") == n - 1 and mid[mid_cap:] == b"\n" * 64      # the formatter's lines, untouched
    got = hip.d2h(d_info, 256)
    assert np.all(got[56:] == 0xA5)
    info = got[:56].view(api.TALLY_INFO_DTYPE)[0]
    want, _ = te.count_text(w.tree, lines, True)
    same_info(info, want, "the call")
    assert want["n_total"] == n and want["n_lines"] == mid_cap - len(lines.rstrip(b"\n")) + n - 1
    ent, tot = w.tally.result()
    totals, entries = te.tally(w.tree, [lines])
    assert listed(ent) == entries and len(entries) > 10
    same_info(tot, totals, "totals")
    for d in bufs + [d_mid, d_finfo, d_info]:
        hip.free(d)
    c.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(gpu_lib, worlds):
    hip = Hip()
    L, t = api.lib(), worlds["fixture"].tally
    d = hip.malloc(512)
    hip.memset(d, 512)
    t.reset()
    assert L.kaiju_gpu_tally_add_text_device(t._h, d, 16, 1, d + 256, None) == 0
    assert L.kaiju_gpu_tally_add_text_device(t._h, d + 4, 16, 1, d + 256, None) == -1          # KAIJU_GPU_ERR_ARG: the text is misaligned
    assert b"16-byte aligned" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_tally_add_text_device(t._h, d, 0xfffffff1, 1, d + 256, None) == -1      # more than kji::kMaxBytes
    assert b"2^32" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_tally_add_text_device(t._h, d, 16, 1, None, None) == -1
    assert L.kaiju_gpu_tally_add_text_device(None, d, 16, 1, d + 256, None) == -1
    assert L.kaiju_gpu_tally_create(None, None) == -1
    info = np.zeros(1, dtype=api.TALLY_INFO_DTYPE)
    assert L.kaiju_gpu_tally_add_text(t._h, None, 5, 1, info.ctypes.data) == -1
    assert L.kaiju_gpu_tally_add_text(t._h, None, 0xfffffff1, 1, info.ctypes.data) == -1
    assert L.kaiju_gpu_tally_add_text(t._h, None, 0, 1, info.ctypes.data) == 0 and int(info[0]["n_lines"]) == 0
    ms = np.zeros(3, dtype=np.float32)
    assert L.kaiju_gpu_tally_pass_ms(t._h, ms.ctypes.data, 3) == -7                             # KAIJU_GPU_ERR_UNSUPPORTED: created without the switch
    # room for fewer entries than there are: the number is said, nothing is written
    t.reset()
    t.add(ti.fixture_texts()[0][1])
    n_all = len(t.result()[0])
    ent = np.zeros(n_all, dtype=api.TALLY_ENTRY_DTYPE)
    n, tot = C.c_uint64(), np.zeros(1, dtype=api.TALLY_INFO_DTYPE)
    assert L.kaiju_gpu_tally_result(t._h, ent.ctypes.data, n_all - 1, C.byref(n), tot.ctypes.data) == -1
    assert n.value == n_all and not np.any(ent["taxon"]) and b"entries" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_tally_result(t._h, ent.ctypes.data, n_all, C.byref(n), tot.ctypes.data) == 0 and n.value == n_all and np.all(ent["summed"] > 0)
    assert hip.L.hipDeviceSynchronize() == 0
    hip.free(d)


def test_pass_times_with_the_switch(worlds, monkeypatch):
    monkeypatch.setenv("KAIJU_GPU_TALLY_TIMES", "1")
    t = api.Tally(worlds["fixture"].dev)
    t.add(ti.fixture_texts()[0][1])
    ms = t.pass_ms()
    assert len(ms) == api.TALLY_PASSES and np.all(ms >= 0) and np.all(np.isfinite(ms))
    t.close()


def test_names_on_another_device(gpu_lib, worlds):
    """a tally works on the device of its names, whatever device the caller has current; a text on another device is refused"""
    if api.device_count() < 2:
        pytest.skip("one device visible")
    hip = Hip()
    w = worlds["fixture"]
    dev = api.DeviceTaxonNames(w.host, 1)
    t = api.Tally(dev)
    check(w, [ti.fixture_texts()[0][1]], "device 1", tally=t)
    assert hip.L.hipSetDevice(0) == 0
    d = hip.malloc(512)                                      # on device 0
    hip.memset(d, 512)
    assert api.lib().kaiju_gpu_tally_add_text_device(t._h, d, 16, 1, d + 256, None) == -1
    assert b"another device" in api.lib().kaiju_gpu_last_error()
    hip.free(d)
    t.close(); dev.close()


# ---- 6. the command line program -----------------------------------------------------------------------------------------
def cli(args, cwd, block=None):
    env = dict(os.environ)
    env.pop("KAIJU_TABLE_BLOCK", None)
    if block:
        env["KAIJU_TABLE_BLOCK"] = str(block)
    return subprocess.run([build.build_table_cli()] + args, env=env, cwd=cwd, capture_output=True, timeout=CLI_TIMEOUT)


@pytest.mark.parametrize("name", sorted(ti.SETS))
def test_cli_against_the_tools_files(gpu_lib, tmp_path, name):
    out = str(tmp_path / "out.tsv")
    r = cli(["-t", "nodes.dmp", "-n", "names.dmp", "-o", out] + ti.argv_of(ti.SETS[name]) + ti.FILES, ti.TABLE, block=4096)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert ti.read(out) == ti.read(os.path.join(ti.TABLE, "out_%s.tsv" % name))
    assert r.stderr.count(b"\n") == 2 and b"no readable taxon id" in r.stderr and b"not contained in nodes.dmp" in r.stderr       # one line per reason


def test_cli_on_the_golden_reads_and_its_failures(gpu_lib, tmp_path):
    out = str(tmp_path / "out.tsv")
    real = os.path.join(ti.TABLE, "real")
    tree = ["-t", "../../nodes.dmp", "-n", "../../names/golden/names.dmp"]
    for name in ("species_eup", "genus_l"):
        r = cli(tree + ["-o", out, "-v"] + ti.argv_of(ti.SETS[name]) + ti.REAL_FILES, real, block=1000)
        assert r.returncode == 0 and b"Processing ../../ref_greedy_1.tsv" in r.stderr, r.stderr[-2000:]
        assert ti.read(out) == ti.read(os.path.join(real, "out_%s.tsv" % name))
    # a file that is not there: status 1, and what was written before it stays, as with the tool
    r = cli(tree + ["-o", out, "-r", "species", ti.REAL_FILES[0], "no_such_file.tsv"], real)
    assert r.returncode == 1 and b"no_such_file.tsv" in r.stderr
    want = ti.read(os.path.join(real, "out_species.tsv"))
    assert ti.read(out) == want[:len(ti.read(out))] and ti.read(out).count(b"\n") > 3
    r = cli(["-t", "no_such_nodes.dmp", "-n", "../../names/golden/names.dmp", "-o", out, "-r", "species", ti.REAL_FILES[0]], real)
    assert r.returncode == 1 and b"no_such_nodes.dmp" in r.stderr
