"""The converter on the device (kaiju_amd/csrc/convert.hip) through the C-ABI and kaiju_amd/bin/kaiju-convertNR: the fixtures of
tests/golden/convert against the files the unmodified tool wrote, and the cases below against tests/convert_expect.py - a header
of 3000 entries beside headers of one, records across chunks and write blocks, 40 000 letters on one line and on 700, out_cap
at 0, one byte short and exact, two calls on one converter, the device-pointer form on a stream of the caller's, the refusals;
the FASTA of the fixtures through the index builder; the command line with a plain and a gzip-compressed map, from -i and from
standard input."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import convert_expect as ce
from kaiju_amd import api, build
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

NODES = os.path.join(ce.GOLD, "nodes.dmp")
CLI_TIMEOUT = 120       # seconds per run of the command line program


class World:
    def __init__(self, api):
        self.fx = ce.Fixture()
        self.host = api.Taxonomy(NODES)
        self.dtax = api.DeviceTaxonomy(self.host, 0)
        self.map = api.AccMap(self.dtax, ce.merged_pairs(ce.golden("merged.dmp")), initial_slots=8).add_text(ce.golden("map.tsv"))
        self.excl = api.AccMap(None).add_keys(ce.golden("excl.txt"))
        self.conv = {}

    def get(self, name):
        a, l, e = ce.SETS[name]
        if name not in self.conv:
            self.conv[name] = api.Converter(self.dtax, self.map, self.excl if e else None, include=self.fx.listed if l else None, add_acc=a)
        return self.conv[name]

    def close(self):
        for c in self.conv.values():
            c.close()
        for x in (self.map, self.excl, self.dtax):
            x.close()


@pytest.fixture(scope="module")
def world(gpu_lib):
    w = World(gpu_lib)
    yield w
    w.close()


def same(conv, want, text, cap, what):
    got, info = conv.convert(text, out_cap=cap)
    assert got == want["written"], what
    for f in ce.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f)
    assert int(info["reserved0"]) == 0 and not info["reserved"].any()


@pytest.mark.parametrize("name", sorted(ce.SETS))
def test_the_fixtures_are_the_tools_files(world, name):
    conv = world.get(name)
    assert conv.convert_file(world.fx.nr) == ce.golden("out_%s.txt" % name)
    assert conv.convert_file(world.fx.nr, block_bytes=64) == ce.golden("out_%s.txt" % name)       # (the largest record has 61 bytes)
    assert conv.convert_file(world.fx.nr_none) == ce.file_of(world.fx.expected(name, text=world.fx.nr_none)["text"]) and conv.convert_file(b"") == b"\n"
    assert name == "l" or conv.convert_file(world.fx.nr_none) == b"\n"                           # (list.txt has 2759: the human record is kept)
    full = world.fx.expected(name)
    n = len(full["text"])
    for cap in (0, n - 1, n, n + 40, len(full["records"][0]), len(full["records"][0]) + 1):
        same(conv, world.fx.expected(name, out_cap=cap), world.fx.nr, cap, (name, cap))
    same(conv, world.fx.expected(name, text=world.fx.nr_none, out_cap=16), world.fx.nr_none, 16, "none")
    same(conv, world.fx.expected(name, text=b"", out_cap=16), b"", 16, "empty")
    got, info = conv.convert(world.fx.nr)                      # sized by a call without a buffer
    assert got == full["text"] and int(info["overflow"]) == 0


def big_text(rng):
    seq = bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYXx") for _ in range(40000))
    big = b">A1.1 x\x01A2.1 y\x01" + b"\x01".join(rng.choice((b"A1.1 x", b"A2.1 y", b"ZZ.9 z")) for _ in range(2998))
    return (b">A1.1 one line\n" + seq + b"\n>A2.1 many\n" + b"\n".join(seq[k:k + 58] for k in range(0, len(seq), 58)) + b"\n" + big + b"\nACD\n>A3.1 z\nEFG\n" +
            b">A1.1 x\x01" * 3 + b"E1.1 excluded behind many\nAAA\n")


def test_long_headers_long_lines_and_capacities(world):
    fx, conv = world.fx, world.get("ale")
    text = big_text(random.Random(23))
    model = lambda cap=None: ce.convert(fx.nodes, fx.listed, fx.model.map, fx.excluded, text, add_acc=True, out_cap=cap)
    full = model()
    assert full["info"]["n_kept"] == 4 and full["info"]["n_entries"] == 3007 and b">A1.1_561\nACD\n" in full["text"] and full["info"]["dropped_excluded"] == 1
    assert full["text"].count(b"\n") == 8 and len(full["text"]) > 70000       # 700 lines and one line give the same letters
    n = len(full["text"])
    for cap in (n, n - 1, 0, 50000, n + 1):
        same(conv, model(cap), text, cap, cap)


def test_records_across_chunks_and_write_blocks(world):
    """random small texts, then many records whose lengths walk through every phase of the 16-byte chunks and the 4096-byte blocks"""
    fx, conv = world.fx, world.get("a")
    rng = random.Random(29)
    accs = [b"A1.1", b"A2.1", b"A3.1", b"A4.1", b"E1.1", b"ZZ", b"", b"B1.1", b"B3.1", b"V\x011.1"]
    model = lambda t, cap=None: ce.convert(fx.nodes, ce.DEFAULT_INCLUDE, fx.model.map, set(), t, add_acc=True, out_cap=cap)
    for trial in range(25):
        lines = []
        for _ in range(rng.randrange(0, 9)):
            kind = rng.randrange(5)
            if kind == 0:
                lines.append(b">" + b"\x01".join(rng.choice(accs) + rng.choice((b" d", b"", b" ", b" a b")) for _ in range(rng.randrange(0, 5))))
            elif kind == 1:
                lines.append(b"")
            else:
                lines.append(bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYXBJOUZacd*-\r") for _ in range(rng.randrange(0, 70))))
        text = b"\n".join(lines) + rng.choice((b"", b"\n"))
        n = len(model(text)["text"])
        for cap in {n, n // 2}:
            same(conv, model(text, cap), text, cap, (trial, cap, text))
    text = b"".join(b">%s d%d\n%s\n" % (rng.choice(accs[:4]), k, b"ACDEFGHIKLMNPQRSTVWY"[:k % 21] * (1 + k % 7)) for k in range(900))
    full = model(text)
    assert len(full["text"]) > 3 * 4096
    for cap in (len(full["text"]), 4096, 4097, 8191):
        same(conv, model(text, cap), text, cap, cap)


def test_two_calls_on_one_converter_do_not_see_each_other(world):
    fx, conv = world.fx, world.get("a")
    big = big_text(random.Random(5))
    small = b">A3.1 z\nEFG\n"
    model = lambda t: ce.convert(fx.nodes, ce.DEFAULT_INCLUDE, fx.model.map, set(), t, add_acc=True)
    for text in (big, small, fx.nr, small, b"", big):
        same(conv, model(text), text, len(model(text)["text"]), len(text))


def test_the_device_pointer_form_on_a_stream_of_the_callers(world):
    hip = Hip()
    stream = hip.stream()
    conv = world.get("ale")
    for text, cap_delta in ((world.fx.nr, 0), (world.fx.nr, -1), (world.fx.nr_none, 5), (world.fx.nr, 7)):
        want_full = world.fx.expected("ale", text=text)
        cap = max(0, len(want_full["text"]) + cap_delta)
        want = world.fx.expected("ale", text=text, out_cap=cap)
        d_text, d_out, d_info = hip.malloc(len(text) + 64), hip.malloc(cap + 64 + 16), hip.malloc(256)
        hip.h2d(d_text, np.concatenate([np.frombuffer(text, dtype=np.uint8), np.full(64, 0x3e, dtype=np.uint8)]))     # '>' behind the text
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
        for f in ce.INFO_FIELDS:
            assert int(info[f]) == want["info"][f], f
        assert int(info["reserved0"]) == 0 and not info["reserved"].any()
        for d in (d_text, d_out, d_info):
            hip.free(d)


def test_a_map_that_grows_between_two_calls(world):
    fx = world.fx
    m = api.AccMap(world.dtax, (), initial_slots=8).add_text(b"x\tA1.1\t562\n", first_block=False)
    conv = api.Converter(world.dtax, m)
    text = b">A1.1 a\x01NEW0.1 b\nAAA\n>NEW77.1 c\nCCC\n"
    assert conv.convert(text)[0] == b">562\nAAA\n"
    m.add_text(b"".join(b"x\tNEW%d.1\t1423\n" % k for k in range(500)), first_block=False)
    assert int(m.info()["rehashes"]) >= 1
    assert conv.convert(text)[0] == b">2\nAAA\n>1423\nCCC\n"
    conv.close()
    m.close()


def test_refusals(gpu_lib, world):
    L, hip = gpu_lib.lib(), Hip()
    conv = world.get("default")
    d = hip.malloc(1024)
    hip.memset(d, 1024)
    args = lambda text, n, out: (conv._h, text, n, out, 64, d + 512, None)
    assert L.kaiju_gpu_convert_text_device(*args(d, 16, d + 128)) == 0
    assert L.kaiju_gpu_convert_text_device(*args(d + 4, 16, d + 128)) == -1 and b"16-byte aligned" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_convert_text_device(*args(d, 16, d + 132)) == -1
    assert L.kaiju_gpu_convert_text_device(*args(d, 0xfffffff1, d + 128)) == -1 and b"2^32" in L.kaiju_gpu_last_error()    # above kji::kMaxBytes
    assert L.kaiju_gpu_convert_text_device(*args(None, 16, d + 128)) == -1 and L.kaiju_gpu_convert_text_device(*args(d, 16, None)) == -1
    assert L.kaiju_gpu_convert_text_device(conv._h, d, 16, d + 128, 64, None, None) == -1
    assert L.kaiju_gpu_convert_text_device(None, d, 16, d + 128, 64, d + 512, None) == -1
    info = np.zeros(1, dtype=api.CONVERT_INFO_DTYPE)
    assert L.kaiju_gpu_convert_text(conv._h, None, 5, None, 0, info.ctypes.data) == -1 and L.kaiju_gpu_convert_text(conv._h, b"x", 1, None, 0, None) == -1
    assert L.kaiju_gpu_convert_text(conv._h, None, 0, None, 0, info.ctypes.data) == 0 and int(info[0]["text_bytes"]) == 0 and int(info[0]["n_records"]) == 0
    h = C.c_void_p()
    assert L.kaiju_gpu_converter_create(None, None, 0, world.map._h, None, 0, C.byref(h)) == -1
    assert L.kaiju_gpu_converter_create(world.dtax._h, None, 0, None, None, 0, C.byref(h)) == -1
    assert L.kaiju_gpu_converter_create(world.dtax._h, None, 2, world.map._h, None, 0, C.byref(h)) == -1
    other = gpu_lib.DeviceTaxonomy(world.host, 0)              # the same tree, uploaded again: another taxonomy
    assert L.kaiju_gpu_converter_create(other._h, None, 0, world.map._h, None, 0, C.byref(h)) == -1 and b"another taxonomy" in L.kaiju_gpu_last_error()
    assert not h.value
    other.close()
    assert L.kaiju_gpu_convert_pass_ms(conv._h, np.zeros(7, dtype=np.float32).ctypes.data, 7) != 0 and b"KAIJU_GPU_CONVERT_TIMES" in L.kaiju_gpu_last_error()
    assert hip.L.hipDeviceSynchronize() == 0
    hip.free(d)


def test_pass_times(gpu_lib, world, monkeypatch):
    monkeypatch.setenv("KAIJU_GPU_CONVERT_TIMES", "1")
    conv = api.Converter(world.dtax, world.map)
    monkeypatch.delenv("KAIJU_GPU_CONVERT_TIMES")
    conv.convert(world.fx.nr)
    ms = conv.pass_ms()
    assert len(ms) == api.CONVERT_PASSES and (ms >= 0).all() and ms.sum() > 0
    conv.close()


def test_the_fasta_of_the_fixtures_goes_through_the_index_builder(world, tmp_path):
    from kaiju_amd import mkfmi
    faa = tmp_path / "db.faa"
    faa.write_bytes(world.get("a").convert_file(world.fx.nr))
    out = mkfmi.build_fmi(str(faa), str(tmp_path / "db.fmi"))
    assert os.path.getsize(out) > 100


# ---- the command line program -------------------------------------------------------------------------------------------
def cli(args, block=None, stdin=None):
    env = dict(os.environ)
    env.pop("KAIJU_CONVERT_BLOCK", None)
    if block:
        env["KAIJU_CONVERT_BLOCK"] = str(block)
    exe = build.build_convert_cli()
    return subprocess.run([exe] + args, env=env, capture_output=True, timeout=CLI_TIMEOUT, input=stdin)


def fixture_args(g="map.tsv"):
    return ["-t", NODES, "-m", os.path.join(ce.GOLD, "merged.dmp"), "-g", g if os.path.isabs(g) else os.path.join(ce.GOLD, g)]


@pytest.mark.parametrize("how", ["plain_file", "gz_stdin_small_blocks"])
def test_cli_against_the_tools_files(gpu_lib, tmp_path, how):
    o = str(tmp_path / "out.faa")
    gz = str(tmp_path / "map.tsv.gz")
    with gzip.open(gz, "wb") as f:
        f.write(ce.golden("map.tsv"))
    opts = {"default": [], "a": ["-a"], "l": ["-l", os.path.join(ce.GOLD, "list.txt")], "e": ["-e", os.path.join(ce.GOLD, "excl.txt")],
            "ale": ["-a", "-l", os.path.join(ce.GOLD, "list.txt"), "-e", os.path.join(ce.GOLD, "excl.txt")]}
    for name in sorted(ce.SETS):
        if how == "plain_file":
            r = cli(fixture_args() + ["-i", os.path.join(ce.GOLD, "nr.txt"), "-o", o] + opts[name])
        else:
            r = cli(fixture_args(gz) + ["-o", o, "-v"] + opts[name], block=130, stdin=ce.golden("nr.txt"))
        assert r.returncode == 0 and r.stdout == b"", (name, r.returncode, r.stderr[-500:])
        with open(o, "rb") as f:
            assert f.read() == ce.golden("out_%s.txt" % name), name
        assert (b" records, " in r.stderr) == (how != "plain_file")
    r = cli(fixture_args() + ["-i", os.path.join(ce.GOLD, "nr_none.txt"), "-o", o])
    assert r.returncode == 0 and open(o, "rb").read() == ce.golden("none_default.txt") == b"\n"


def test_cli_statuses(gpu_lib, tmp_path):
    o = str(tmp_path / "o.faa")
    nr = os.path.join(ce.GOLD, "nr.txt")
    full = fixture_args() + ["-i", nr, "-o", o]
    big = str(tmp_path / "big.txt")                            # a record of 309 bytes between two small ones, blocks of 200
    with open(big, "wb") as f:
        f.write(b">A2.1 y\nAAA\n>A1.1 x\n" + b"ACD" * 100 + b"\n>A2.1 y\nAAA\n")
    r = cli(fixture_args() + ["-i", big, "-o", o], block=200)
    assert r.returncode == 1 and b"Error: a record of more than 200 bytes" in r.stderr, r.stderr[-300:]
    r = cli(fixture_args() + ["-i", big, "-o", o], block=400)
    assert r.returncode == 0 and open(o, "rb").read() == b">564\nAAA\n>562\n" + b"ACD" * 100 + b"\n>564\nAAA\n"
    for drop, word in ((0, b"Error: Please specify the location of the nodes.dmp file, using the -t option.\n\n"),
                       (2, b"Error: Please specify the location of the merged.dmp file, using the -m option.\n\n"),
                       (4, b"Error: Please specify the location of the prot.accession2taxid file, using the -g option.\n\n"),
                       (8, b"Error: Please specify the name of the output file, using the -o option.\n\n")):
        r = cli(full[:drop] + full[drop + 2:])
        assert r.returncode == 1 and r.stderr.startswith(word) and b"Usage:" in r.stderr and r.stdout == b"", (drop, r.stderr[:300])
    none = str(tmp_path / "none")
    for at, extra in ((1, []), (3, []), (5, []), (7, []), (None, ["-l", none]), (None, ["-e", none])):
        args = list(full) + extra
        if at is not None:
            args[at] = none
        r = cli(args)
        assert r.returncode == 1 and (b"Error: Could not open file " + none.encode() + b"\n\n") in r.stderr and b"Usage:" not in r.stderr, (at, extra, r.stderr[-300:])
    r = cli(fixture_args() + ["-i", nr, "-o", str(tmp_path / "no" / "dir" / "o.faa")])
    assert r.returncode == 1 and b"for writing." in r.stderr
    for args in (["-h"], ["-x"], full + ["-r"]):
        r = cli(args)
        assert r.returncode == 1 and b"Usage:" in r.stderr
