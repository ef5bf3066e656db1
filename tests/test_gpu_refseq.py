"""The rule set of kaiju-convertRefSeq on the device (k_am_parse with refseq_map_line in kaiju_amd/csrc/accmap.hip, k_cv_first in
kaiju_amd/csrc/convert.hip) through the C-ABI, kaiju_amd.api and kaiju_amd/bin/kaiju-convertRefSeq: the fixtures of
tests/golden/refseq against the files the unmodified tool wrote, in one block and in small ones, and the cases below against
tests/refseq_expect.py - out_cap at 0, one byte short, exact and at one record, the first space of a header around the 16-byte
chunks, a header of 40 000 bytes without a space and one whose space is its last byte, two thousand records across several write
blocks, a map that grows between two conversions, the device-pointer form on a stream of the caller's, the refusals, the command
line with a plain and a gzip-compressed map, and the kept FASTA through the index builder."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import refseq_expect as rs
from kaiju_amd import api, build
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

NODES = os.path.join(rs.GOLD, "nodes.dmp")
CLI_TIMEOUT = 120       # seconds per run of the command line program
ERR_ARG, ERR_UNSUPPORTED = -1, -7


class World:
    def __init__(self, api):
        self.fx = rs.Fixture()
        self.host = api.Taxonomy(NODES)
        self.dtax = api.DeviceTaxonomy(self.host, 0)
        self.map = api.AccMap(self.dtax, self.fx.pairs, initial_slots=8, rules="refseq").add_text(rs.golden("map.tsv"))
        self.conv = {}

    def get(self, name):
        a, l = rs.SETS[name]
        if name not in self.conv:
            self.conv[name] = api.Converter(self.dtax, self.map, include=self.fx.listed if l else None, add_acc=a, rules="refseq")
        return self.conv[name]

    def close(self):
        for c in self.conv.values():
            c.close()
        for x in (self.map, self.dtax):
            x.close()


@pytest.fixture(scope="module")
def world(gpu_lib):
    w = World(gpu_lib)
    yield w
    w.close()


def same(conv, want, text, cap, what):
    got, info = conv.convert(text, out_cap=cap)
    assert got == want["written"], what
    for f in rs.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f)
    assert int(info["reserved0"]) == 0 and not info["reserved"].any()


def test_the_map_of_the_fixture(world):
    fx, m = world.fx, world.map
    keys = sorted({l.split(b"\t")[0] for l in rs.golden("map.tsv").split(b"\n")} | {b"WP", b"WP_", b"WP_5.", b"WP_12", b"WP_34", b"nope", b""})
    assert m.lookup(keys) == [fx.model.lookup(k) for k in keys]
    st = m.info()
    assert (int(st["entries"]), int(st["lines"]), int(st["lines_no_insert"]), int(st["duplicates"])) == (len(fx.model.map), fx.model.lines, fx.model.no_insert, fx.model.duplicates)
    assert int(st["rehashes"]) >= 1
    # in blocks of three lines, the collisions of a truncated key with a full one across blocks included; add_keys on such a map
    lines = rs.golden("map.tsv").split(b"\n")
    lines = [l + b"\n" for l in lines[:-1]] + [lines[-1]]
    small = api.AccMap(world.dtax, fx.pairs, initial_slots=8, rules="refseq")
    for k in range(0, len(lines), 3):
        small.add_text(b"".join(lines[k:k + 3]), first_block=k == 0)
    assert small.lookup(keys) == [fx.model.lookup(k) for k in keys]
    small.add_keys(b"NP_whole line\tas it is\n", value=564)
    assert small.lookup([b"NP_whole line\tas it is", b"WP_12"]) == [564, 562]
    small.close()


@pytest.mark.parametrize("name", sorted(rs.SETS))
def test_the_fixtures_are_the_tools_files(world, name):
    conv = world.get(name)
    assert conv.convert_file(world.fx.faa) == rs.golden("out_%s.txt" % name)
    assert conv.convert_file(world.fx.faa, block_bytes=64) == rs.golden("out_%s.txt" % name)     # (the largest record has 52 bytes)
    assert conv.convert_file(world.fx.faa_none) == rs.file_of(world.fx.expected(name, text=world.fx.faa_none)["text"]) and conv.convert_file(b"") == b"\n"
    assert "l" in name or conv.convert_file(world.fx.faa_none) == rs.golden("none_default.txt") == b"\n"
    full = world.fx.expected(name)
    n = len(full["text"])
    for cap in (0, n - 1, n, n + 40, len(full["records"][0]), len(full["records"][0]) + 1):
        same(conv, world.fx.expected(name, out_cap=cap), world.fx.faa, cap, (name, cap))
    same(conv, world.fx.expected(name, text=world.fx.faa_none, out_cap=16), world.fx.faa_none, 16, "none")
    same(conv, world.fx.expected(name, text=b"", out_cap=16), b"", 16, "empty")
    got, info = conv.convert(world.fx.faa)                     # sized by a call without a buffer
    assert got == full["text"] and int(info["overflow"]) == 0 and int(info["dropped_excluded"]) == 0 and int(info["dropped_no_lca"]) == 0


def test_the_first_space_around_the_chunk_boundaries_and_long_headers(world):
    """one text: headers whose first space is byte 15 .. 33 of the line, each at every residue of the line start mod 16 (a
    sequence line in front of the header puts it there), with and without the space; then a header of 40 000 bytes without a space
    and one of 40 000 bytes whose only space is the last byte"""
    fx = world.fx
    at_of = (15, 16, 17, 31, 32, 33)
    keys = {at: b"WP_" + b"K" * (at - 4) for at in at_of}
    long_key = b"WP_" + b"L" * 39995
    m = api.AccMap(world.dtax, fx.pairs, initial_slots=8, rules="refseq")
    m.add_text(b"".join(b"%s\t%d\n" % (k, 562 if at & 1 else 564) for at, k in keys.items()) + long_key + b"\t1423\n", first_block=False)
    amap = {k: (562 if at & 1 else 564) for at, k in keys.items()}
    amap[long_key] = 1423
    text, starts = b"", set()
    for at in at_of:
        for tail in (b" d e", b" ", b""):
            for j in range(16):                                # a sequence line that puts the header at residue j
                text += b"ACDEFGHIKLMNPQRSx"[:(j - len(text) - 1) % 16] + b"\n"
                starts.add((at, tail, len(text) % 16))
                text += b">" + keys[at] + tail + b"\n"
    assert len(starts) == 6 * 3 * 16
    text += b"AAA\n>" + long_key + b"L\nAAA\n>" + long_key + b" \nCCC\n>" + long_key[:-1] + b" x\nDDD\n"
    assert all(len(h) == 40000 for h in text.split(b"\n")[-7:-3:2])
    conv = api.Converter(world.dtax, m, add_acc=True, rules="refseq")
    want = rs.convert(fx.nodes, rs.DEFAULT_INCLUDE, amap, text, add_acc=True)
    assert want["info"]["n_kept"] == 6 * 2 * 16 + 1 and want["info"]["n_entries"] == 6 * 2 * 16 + 2 and want["text"].endswith(b"_1423\nCCC\n")
    n = len(want["text"])
    for cap in (n, n - 1):
        same(conv, rs.convert(fx.nodes, rs.DEFAULT_INCLUDE, amap, text, add_acc=True, out_cap=cap), text, cap, cap)
    conv.close()
    m.close()


def test_two_thousand_records_across_write_blocks(world):
    fx, conv = world.fx, world.get("a")
    rng = random.Random(29)
    accs = [b"WP_1.1", b"WP_5.", b"WP_5.1", b"WP", b"WP_", b"", b"ZZ", b"WP_H.1", b"WP_B1.1", b"WP_\x011.1", b"WP_R1", b"WP_8.1", b"WP_LAST.1"]
    tails = (b" d%d", b" d%d\x01WP_1.1 x", b"%d", b" ", b" a b %d\r")
    text = b""
    for k in range(2000):
        tail = rng.choice(tails)
        text += b">" + rng.choice(accs) + (tail % k if b"%d" in tail else tail) + b"\n" + b"ACDEFGHIKLMNPQRSTVWYxX*"[:k % 24] * (1 + k % 7) + b"\n"
    model = lambda cap=None: rs.convert(fx.nodes, rs.DEFAULT_INCLUDE, fx.model.map, text, add_acc=True, out_cap=cap)
    full = model()
    assert full["info"]["n_records"] == 2000 and len(full["text"]) > 3 * 4096 and 300 < full["info"]["n_kept"] < 1500
    for cap in (len(full["text"]), 4096, 4097, 8191, 0):
        same(conv, model(cap), text, cap, cap)
    assert conv.convert_file(text, block_bytes=5000) == full["text"]
    for t in (b">WP_1.1 z\nEFG\n", b"", text):                 # calls on one converter do not see each other
        want = rs.convert(fx.nodes, rs.DEFAULT_INCLUDE, fx.model.map, t, add_acc=True)
        same(conv, want, t, len(want["text"]), len(t))


def test_a_map_that_grows_between_two_conversions(world):
    m = api.AccMap(world.dtax, world.fx.pairs, initial_slots=8, rules="refseq").add_text(b"WP_A1.1\t562\n", first_block=False)
    conv = api.Converter(world.dtax, m, rules="refseq")
    text = b">WP_A1.1 a\x01WP_NEW0.1 b\nAAA\n>WP_NEW77.1 c\nCCC\n>WP_NEW7. d\nDDD\n"
    assert conv.convert(text)[0] == b">562\nAAA\n"
    m.add_text(b"".join(b"WP_NEW%d.1\t%d\n" % (k, 666 if k == 7 else 1423) for k in range(500)), first_block=False)
    assert int(m.info()["rehashes"]) >= 1
    assert conv.convert(text)[0] == b">562\nAAA\n>1423\nCCC\n>562\nDDD\n"
    conv.close()
    m.close()


def test_the_device_pointer_form_on_a_stream_of_the_callers(world):
    hip = Hip()
    stream = hip.stream()
    conv = world.get("al")
    for text, cap_delta in ((world.fx.faa, 0), (world.fx.faa, -1), (world.fx.faa_none, 5), (world.fx.faa, 7)):
        want_full = world.fx.expected("al", text=text)
        cap = max(0, len(want_full["text"]) + cap_delta)
        want = world.fx.expected("al", text=text, out_cap=cap)
        d_text, d_out, d_info = hip.malloc(len(text) + 64), hip.malloc(cap + 64 + 16), hip.malloc(256)
        hip.h2d(d_text, np.concatenate([np.frombuffer(text, dtype=np.uint8), np.full(64, 0x20, dtype=np.uint8)]))     # spaces behind the text
        hip.h2d(d_out, np.full(cap + 64, 0xA5, dtype=np.uint8))
        hip.h2d(d_info, np.full(256, 0xA5, dtype=np.uint8))
        conv.convert_device(d_text, len(text), d_out, cap, d_info, stream=stream)
        assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        info = hip.d2h(d_info, 256)
        out = hip.d2h(d_out, cap + 64)
        assert (info[128:] == 0xA5).all() and (out[cap:] == 0xA5).all()
        info = info[:128].view(api.CONVERT_INFO_DTYPE)[0]
        n = int(info["written_bytes"])
        assert bytes(out[:n]) == want["written"] and (out[n:] == 0xA5).all()
        for f in rs.INFO_FIELDS:
            assert int(info[f]) == want["info"][f], f
        assert int(info["reserved0"]) == 0 and not info["reserved"].any()
        for d in (d_text, d_out, d_info):
            hip.free(d)


def test_refusals(gpu_lib, world):
    L = gpu_lib.lib()
    h = C.c_void_p()
    nr_map = api.AccMap(world.dtax, world.fx.pairs)
    keys_map = api.AccMap(None).add_keys(b"WP_1.1\n")
    # a map of the other rule set, either way round; an exclusion map (no taxonomy, the rules of the old create) as the map
    assert L.kaiju_gpu_converter_create_rules(world.dtax._h, None, 0, nr_map._h, 1, 0, C.byref(h)) == ERR_ARG and b"rule set" in L.kaiju_gpu_last_error() and not h.value
    assert L.kaiju_gpu_converter_create_rules(world.dtax._h, None, 0, world.map._h, 0, 0, C.byref(h)) == ERR_ARG and b"rule set" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_converter_create(world.dtax._h, None, 0, world.map._h, None, 0, C.byref(h)) == ERR_ARG and b"rule set" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_converter_create_rules(world.dtax._h, None, 0, keys_map._h, 1, 0, C.byref(h)) == ERR_ARG and not h.value
    assert L.kaiju_gpu_converter_create_rules(world.dtax._h, None, 0, world.map._h, 2, 0, C.byref(h)) == ERR_ARG
    assert L.kaiju_gpu_converter_create_rules(world.dtax._h, None, 0, None, 1, 0, C.byref(h)) == ERR_ARG
    assert L.kaiju_gpu_converter_create_rules(world.dtax._h, None, 2, world.map._h, 1, 0, C.byref(h)) == ERR_ARG
    assert L.kaiju_gpu_converter_create_rules(world.dtax._h, None, 0, world.map._h, 1, 0, None) == ERR_ARG
    with pytest.raises(api.KaijuGpuError, match="excluded"):
        api.Converter(world.dtax, world.map, excluded=keys_map, rules="refseq")
    with pytest.raises(api.KaijuGpuError, match="rules"):
        api.AccMap(world.dtax, rules="refseq_nr")
    # the rule set of the map; the old create keeps its refusal of other columns
    assert L.kaiju_gpu_accmap_create_rules(world.dtax._h, 0, None, 0, 2, 0, C.byref(h)) == ERR_ARG and b"rule set" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_accmap_create_rules(world.dtax._h, 0, None, 0, 1, 0, None) == ERR_ARG and L.kaiju_gpu_accmap_create_rules(world.dtax._h, 0, None, 3, 1, 0, C.byref(h)) == ERR_ARG
    assert L.kaiju_gpu_accmap_create(world.dtax._h, 0, None, 0, 0, 1, 0, C.byref(h)) == ERR_UNSUPPORTED and b"other columns are not built yet" in L.kaiju_gpu_last_error()
    assert not h.value
    # a map of KAIJU_GPU_CONVERT_RULES_NR through the new create is the map of the old one
    assert L.kaiju_gpu_accmap_create_rules(world.dtax._h, 0, None, 0, 0, 8, C.byref(h)) == 0 and h.value
    line = b"x\tA1.1\t562\t1\n"
    assert L.kaiju_gpu_accmap_add_text(h, line, len(line), 0) == 0
    taxa, n = np.zeros(2, dtype=np.uint64), C.c_uint64()
    assert L.kaiju_gpu_accmap_lookup(h, b"A1.1\nx\n", 7, taxa.ctypes.data, 2, C.byref(n)) == 0 and [int(t) for t in taxa] == [562, rs.MISS]
    L.kaiju_gpu_accmap_free(h)
    nr_map.close()
    keys_map.close()


def test_the_fasta_of_the_fixtures_goes_through_the_index_builder(world, tmp_path):
    from kaiju_amd import mkfmi
    faa = tmp_path / "db.faa"
    faa.write_bytes(world.get("a").convert_file(world.fx.faa))
    out = mkfmi.build_fmi(str(faa), str(tmp_path / "db.fmi"))
    assert os.path.getsize(out) > 100


# ---- the command line program -------------------------------------------------------------------------------------------
def cli(args, block=None, stdin=b""):
    env = dict(os.environ)
    env.pop("KAIJU_CONVERT_BLOCK", None)
    if block:
        env["KAIJU_CONVERT_BLOCK"] = str(block)
    exe = build.build_refseq_cli()
    return subprocess.run([exe] + args, env=env, capture_output=True, timeout=CLI_TIMEOUT, input=stdin)


def fixture_args(g="map.tsv"):
    return ["-t", NODES, "-m", os.path.join(rs.GOLD, "merged.dmp"), "-g", g if os.path.isabs(g) else os.path.join(rs.GOLD, g)]


@pytest.mark.parametrize("how", ["plain", "gz_small_blocks"])
def test_cli_against_the_tools_files(gpu_lib, tmp_path, how):
    o = str(tmp_path / "out.faa")
    gz = str(tmp_path / "map.tsv.gz")
    with gzip.open(gz, "wb") as f:
        f.write(rs.golden("map.tsv"))
    opts = {"default": [], "a": ["-a"], "l": ["-l", os.path.join(rs.GOLD, "list.txt")], "al": ["-a", "-l", os.path.join(rs.GOLD, "list.txt")]}
    for name in sorted(rs.SETS):
        if how == "plain":
            r = cli(fixture_args() + ["-o", o] + opts[name], stdin=rs.golden("faa.txt"))
        else:
            r = cli(fixture_args(gz) + ["-o", o, "-v", "-d"] + opts[name], block=100, stdin=rs.golden("faa.txt"))
        assert r.returncode == 0 and r.stdout == b"", (name, r.returncode, r.stderr[-500:])
        with open(o, "rb") as f:
            assert f.read() == rs.golden("out_%s.txt" % name), name
        assert (b" records, " in r.stderr) == (how != "plain")
    r = cli(fixture_args() + ["-o", o], stdin=rs.golden("faa_none.txt"))
    assert r.returncode == 0 and open(o, "rb").read() == rs.golden("none_default.txt") == b"\n"


def test_cli_statuses(gpu_lib, tmp_path):
    o = str(tmp_path / "o.faa")
    full = fixture_args() + ["-o", o]
    for extra in (["-i", os.path.join(rs.GOLD, "faa.txt")], ["-e", os.path.join(rs.GOLD, "list.txt")], ["-r"], ["-h"], ["-x"]):
        r = cli(full + extra, stdin=rs.golden("faa.txt"))
        assert r.returncode == 1 and b"Usage:" in r.stderr and b"standard input" in r.stderr and not os.path.exists(o), extra
    for drop, word in ((0, b"Error: Please specify the location of the nodes.dmp file, using the -t option.\n\n"),
                       (2, b"Error: Please specify the location of the merged.dmp file, using the -m option.\n\n"),
                       (4, b"Error: Please specify the location of the prot.accession2taxid file, using the -g option.\n\n"),
                       (6, b"Error: Please specify the name of the output file, using the -o option.\n\n")):
        r = cli(full[:drop] + full[drop + 2:])
        assert r.returncode == 1 and r.stderr.startswith(word) and b"Usage:" in r.stderr and r.stdout == b"", (drop, r.stderr[:300])
    none = str(tmp_path / "none")
    for at, extra in ((1, []), (3, []), (5, []), (None, ["-l", none])):
        args = list(full) + extra
        if at is not None:
            args[at] = none
        r = cli(args)
        assert r.returncode == 1 and (b"Error: Could not open file " + none.encode() + b"\n\n") in r.stderr and b"Usage:" not in r.stderr, (at, extra, r.stderr[-300:])
    # a record of 309 bytes between two small ones, blocks of 200: an error that names the size; a map line larger than a block, too
    big = b">WP_B8.1 y\nAAA\n>WP_1.1 x\n" + b"ACD" * 100 + b"\n>WP_B8.1 y\nAAA\n"
    r = cli(full, block=200, stdin=big)
    assert r.returncode == 1 and b"Error: a record of more than 200 bytes" in r.stderr, r.stderr[-300:]
    r = cli(full, block=400, stdin=big)
    assert r.returncode == 0 and open(o, "rb").read() == b">564\nAAA\n>562\n" + b"ACD" * 100 + b"\n>564\nAAA\n"
    r = cli(full, block=30, stdin=big)
    assert r.returncode == 1 and b"Error: a line of more than 30 bytes" in r.stderr, r.stderr[-300:]
