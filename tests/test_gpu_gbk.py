"""The GenBank converter on the device (kaiju_amd/csrc/gbk.hip) through the C-ABI and kaiju_amd/bin/kaiju-gbk2faa: the fixtures
of tests/golden/gbk against the files the unmodified script wrote, whole and with a block cut behind every line, and the cases
below against tests/gbk_expect.py - 100 KB of generated text whose line scans cross scan blocks, a translation of 5000 letters on
one line and one of 700 lines, protein ids of 1 and 300 bytes, a taxon of 25 digits, out_cap at 0, one byte short and exact,
the repeat after an overflow, reset, what the output buffer held before, the device-pointer form on a stream of the
caller's, the missing taxon, the refusals; the command line on a plain and a gzip-compressed input in blocks of 4 KiB; the
FASTA of the fixture through the index builder."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import gbk_expect as ge
from kaiju_amd import api, build
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

CLI_TIMEOUT = 120       # seconds per run of the command line program


@pytest.fixture(scope="module")
def gbk(gpu_lib):
    g = gpu_lib.Gbk(0)
    yield g
    g.close()


def same(gbk, want, text, cap, what, fill=0x77):
    got, info = gbk.convert(text, out_cap=cap, fill=fill)
    assert got == want["written"], what
    for f in ge.INFO_FIELDS:
        assert int(info[f]) == want["info"][f], (what, f)
    assert [int(x) for x in info["lines_kind"]] == want["kinds"], what
    assert int(info["reserved0"]) == 0 and not info["reserved"].any()


def big_text(rng):
    """about 100 KB and 3000 lines: a taxon line at the very start, records with a taxon of 25 digits and protein ids of 300 bytes
    and of 1 byte, 5000 letters on one line, a translation of 700 lines, and a translation that opens in the last tile"""
    long_line = b'                     /translation="' + bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYXBZbz") for _ in range(5000)) + b'"\n'
    many = b' /protein_id="M"\n /translation="' + b"\n".join(bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYx ") for _ in range(rng.randrange(0, 60))) for _ in range(700)) + b'" behind\n'
    return (b'/db_xref="taxon:7"\n /translation="MKV"\n' + ge.genbank_text(rng, 2, cds_per_record=6, origin_lines=20, taxon_digits=25, pid_len=300) + long_line +
            ge.genbank_text(rng, 3, cds_per_record=30, origin_lines=20, pid_len=1) + many + ge.random_text(rng, 700) + b"\n" +
            ge.genbank_text(rng, 2, cds_per_record=20, origin_lines=30) + b' /translation="MKVLA\n ACD\n EFG')


@pytest.fixture(scope="module")
def big():
    text = big_text(random.Random(41))
    full = ge.convert(text)
    assert 90000 < len(text) < 130000 and 2500 < text.count(b"\n") < 3500 and full["state"].in_t and len(text) - text.rindex(b'/translation="') < 4096
    assert full["text"].startswith(b">_7\nMKV\n") and full["kinds"][3] > 20 and full["info"]["letters_dropped"] > 500
    return text, full


@pytest.mark.parametrize("name", ge.FIXTURES)
def test_the_fixtures_are_the_scripts_files(gbk, name):
    text = ge.golden(name + ".gbk")
    want, status = ge.golden(name + ".faa"), ge.convert_file(text)[1]
    longest = max(len(l) for l in text.split(b"\n")) + 1
    for block_bytes in (1 << 24, longest):                     # whole; in blocks of a line or two
        if status:
            with pytest.raises(api.GbkNoTaxon) as e:
                gbk.convert_file(text, block_bytes=block_bytes)
            assert e.value.line == ge.convert(text)["info"]["no_taxon_line"]
        else:
            assert gbk.convert_file(text, block_bytes=block_bytes) == want
    for cut in ge.cuts_behind_lines(text):                     # two blocks, the cut behind every line in turn
        gbk.reset()
        st = ge.State()
        for block in (text[:cut], text[cut:]):
            r = ge.convert(block, st)
            same(gbk, r, block, len(r["text"]), (name, cut))
            st = r["state"]


def test_scans_across_blocks_long_lines_and_capacities(gbk, big):
    text, full = big
    n = len(full["text"])
    first = len(full["lines"][0]) + len(full["lines"][1])
    for cap in (n, n - 1, 0, first, first - 1, 50000, n + 1):
        gbk.reset()
        same(gbk, ge.convert(text, out_cap=cap), text, cap, cap)
    gbk.reset()
    assert gbk.convert_file(text, block_bytes=8192) == full["text"]            # (the 5000 letters fit a block)
    assert gbk.convert_file(text, block_bytes=1 << 24) == full["text"]


def test_the_repeat_after_an_overflow_and_reset(gbk, big):
    text, full = big
    cut = text.index(b"\n", len(text) // 2) + 1
    a = ge.convert(text[:cut])
    b = ge.convert(text[cut:], a["state"])
    assert a["state"].taxon and a["state"].pid and len(b["text"]) > 100
    gbk.reset()
    same(gbk, a, text[:cut], len(a["text"]), "first block")
    short = ge.convert(text[cut:], a["state"], out_cap=len(b["text"]) - 1)
    assert short["info"]["overflow"] == 1 and short["state"] == a["state"]
    same(gbk, short, text[cut:], len(b["text"]) - 1, "one byte short")
    same(gbk, ge.convert(text[cut:], a["state"], out_cap=0), text[cut:], 0, "no room")
    same(gbk, b, text[cut:], len(b["text"]), "the repeat")                     # the state had not advanced
    tail = b"  ACD\n  EFG\"\n /translation=\"KLM\"\n"
    same(gbk, ge.convert(tail, b["state"]), tail, 200, "behind the repeat")    # ... and has now: the last translation is open
    assert ge.convert(tail, b["state"])["text"].startswith(b"ACD\nEFG\n>")
    gbk.reset()
    same(gbk, ge.convert(tail), tail, 200, "behind reset")                     # no taxon any more
    assert ge.convert(tail)["info"]["no_taxon_line"] == 3


def test_two_calls_give_the_same_bytes_whatever_the_buffer_held(gbk, big):
    text, full = big
    small = ge.golden("record.gbk")
    for t, fill in ((text, 0x77), (small, 0x00), (text, 0x00), (b"", 0x41), (small, 0xff), (text, 0x3e)):
        gbk.reset()
        want = ge.convert(t)
        same(gbk, want, t, len(want["text"]) + 16, len(t), fill=fill)


def test_the_missing_taxon(gbk):
    for name in ("notaxon", "notaxon_late"):
        text = ge.golden(name + ".gbk")
        gbk.reset()
        want = ge.convert(text)
        assert want["info"]["no_taxon_line"] and want["text"] == b""
        same(gbk, want, text, 4096, name)
        fixed = b' /db_xref="taxon:3"\n'
        same(gbk, ge.convert(fixed), fixed, 16, "a taxon")                       # the state had not advanced: nothing is open
        same(gbk, ge.convert(text, ge.State(b"3")), text, 4096, "with a taxon")


def test_the_device_pointer_form_on_a_stream_of_the_callers(gbk, big):
    hip = Hip()
    stream = hip.stream()
    text, full = big
    cut = text.index(b"\n", len(text) // 3) + 1
    gbk.reset()
    st = ge.State()
    for block, cap_delta in ((text[:cut], 0), (text[cut:], -1), (text[cut:], 7)):
        want_full = ge.convert(block, st)
        cap = len(want_full["text"]) + cap_delta
        want = ge.convert(block, st, out_cap=cap)
        d_text, d_out, d_info = hip.malloc(len(block) + 64), hip.malloc(cap + 64 + 16), hip.malloc(256)
        hip.h2d(d_text, np.concatenate([np.frombuffer(block, dtype=np.uint8), np.full(64, 0x22, dtype=np.uint8)]))     # '"' behind the text
        hip.h2d(d_out, np.full(cap + 64, 0xA5, dtype=np.uint8))
        hip.h2d(d_info, np.full(256, 0xA5, dtype=np.uint8))
        gbk.convert_device(d_text, len(block), d_out, cap, d_info, stream=stream)
        assert hip.L.hipStreamSynchronize(C.c_void_p(stream)) == 0
        info = hip.d2h(d_info, 256)
        out = hip.d2h(d_out, cap + 64)
        assert (info[128:] == 0xA5).all() and (out[cap:] == 0xA5).all()
        info = info[:128].view(api.GBK_INFO_DTYPE)[0]
        n = int(info["written_bytes"])
        assert bytes(out[:n]) == want["written"] and (out[n:] == 0xA5).all()
        for f in ge.INFO_FIELDS:
            assert int(info[f]) == want["info"][f], f
        assert int(info["reserved0"]) == 0 and not info["reserved"].any()
        st = want["state"]
        for d in (d_text, d_out, d_info):
            hip.free(d)


def test_refusals(gpu_lib, gbk):
    L, hip = gpu_lib.lib(), Hip()
    d = hip.malloc(1024)
    hip.memset(d, 1024)
    gbk.reset()
    args = lambda text, n, out: (gbk._h, text, n, out, 64, d + 512, None)
    assert L.kaiju_gpu_gbk_text_device(*args(d, 16, d + 128)) == 0
    assert L.kaiju_gpu_gbk_text_device(*args(d + 4, 16, d + 128)) == -1 and b"16-byte aligned" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_gbk_text_device(*args(d, 16, d + 132)) == -1
    assert L.kaiju_gpu_gbk_text_device(*args(d, 0xfffffff1, d + 128)) == -1 and b"2^32" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_gbk_text_device(*args(None, 16, d + 128)) == -1 and L.kaiju_gpu_gbk_text_device(*args(d, 16, None)) == -1
    assert L.kaiju_gpu_gbk_text_device(gbk._h, d, 16, d + 128, 64, None, None) == -1
    assert L.kaiju_gpu_gbk_text_device(None, d, 16, d + 128, 64, d + 512, None) == -1
    info = np.zeros(1, dtype=api.GBK_INFO_DTYPE)
    assert L.kaiju_gpu_gbk_text(gbk._h, None, 5, None, 0, info.ctypes.data) == -1 and L.kaiju_gpu_gbk_text(gbk._h, b"x", 1, None, 0, None) == -1
    assert L.kaiju_gpu_gbk_text(gbk._h, None, 0, None, 0, info.ctypes.data) == 0 and int(info[0]["text_bytes"]) == 0 and int(info[0]["n_lines"]) == 0
    h = C.c_void_p()
    assert L.kaiju_gpu_gbk_create(0, None) == -1 and L.kaiju_gpu_gbk_create(4096, C.byref(h)) == -1 and not h.value and L.kaiju_gpu_gbk_reset(None) == -1
    assert L.kaiju_gpu_gbk_pass_ms(gbk._h, np.zeros(6, dtype=np.float32).ctypes.data, 6) != 0 and b"KAIJU_GPU_CONVERT_TIMES" in L.kaiju_gpu_last_error()
    assert hip.L.hipDeviceSynchronize() == 0
    hip.free(d)


def test_pass_times(gpu_lib, monkeypatch):
    monkeypatch.setenv("KAIJU_GPU_CONVERT_TIMES", "1")
    g = api.Gbk(0)
    monkeypatch.delenv("KAIJU_GPU_CONVERT_TIMES")
    g.convert(ge.golden("record.gbk"))
    ms = g.pass_ms()
    assert len(ms) == api.GBK_PASSES and (ms >= 0).all() and ms.sum() > 0
    g.close()


def test_the_fasta_of_the_fixture_goes_through_the_index_builder(gbk, tmp_path):
    from kaiju_amd import mkfmi
    faa = tmp_path / "db.faa"
    faa.write_bytes(gbk.convert_file(ge.golden("record.gbk")))
    assert faa.read_bytes() == ge.golden("record.faa")
    out = mkfmi.build_fmi(str(faa), str(tmp_path / "db.fmi"))
    ix = api.Index(out, 0)
    assert os.path.getsize(out) > 100 and ix.db_length > 0
    ix.close()


# ---- the command line program -------------------------------------------------------------------------------------------
def cli(args, block=None):
    env = dict(os.environ)
    env.pop("KAIJU_GBK_BLOCK", None)
    if block:
        env["KAIJU_GBK_BLOCK"] = str(block)
    return subprocess.run([build.build_gbk_cli()] + args, env=env, capture_output=True, timeout=CLI_TIMEOUT)


@pytest.mark.parametrize("how", ["plain", "gzip"])
def test_cli_in_blocks_of_4_kib(gpu_lib, tmp_path, big, how):
    text, full = big
    src, o = str(tmp_path / ("in.gbff" + (".gz" if how == "gzip" else ""))), str(tmp_path / "out.faa")
    pieces = [(text, full["text"])] + [(ge.golden(n + ".gbk"), ge.golden(n + ".faa")) for n in ("rules", "record", "crlf", "tail_open", "empty")]
    for data, want in pieces:
        with (gzip.open(src, "wb") if how == "gzip" else open(src, "wb")) as f:
            f.write(data)
        block = 8192 if data is pieces[0][0] else 4096          # (the generated text has a line of 5000 letters and headers)
        r = cli(["-v", src, o] if how == "gzip" else [src, o], block=block)
        assert r.returncode == 0 and r.stdout == b"", (r.returncode, r.stderr[-500:])
        with open(o, "rb") as f:
            assert f.read() == want
        assert (b" records, " in r.stderr) == (how == "gzip")
    r = cli([src.replace("in.", "missing."), o])
    assert r.returncode == 255 and b"Opening input file failed" in r.stderr


def test_cli_statuses(gpu_lib, tmp_path):
    o = str(tmp_path / "o.faa")
    with open(o, "wb") as f:
        f.write(b"old content")
    r = cli([os.path.join(ge.GOLD, "notaxon_late.gbk"), o], block=40)
    assert r.returncode == 255 and r.stderr.startswith(b"No taxon id found in gbk file ") and b"(line 6)" in r.stderr and os.path.getsize(o) == 0
    r = cli([os.path.join(ge.GOLD, "rules.gbk"), o], block=30)
    assert r.returncode == 255 and b"a line of more than 30 bytes" in r.stderr
    bz = str(tmp_path / "x.gbff.bz2")
    with open(bz, "wb") as f:
        f.write(b"BZh91AY&SY" + bytes(40))
    r = cli([bz, o])
    assert r.returncode == 255 and b"bzip2" in r.stderr
    for args in ([], [bz], ["-v", bz]):
        r = cli(args)
        assert r.returncode == 255 and r.stderr.startswith(b"Usage: ") and r.stdout == b""
    r = cli(["-x", bz, o])
    assert r.returncode == 255 and b"unknown option -x" in r.stderr
    r = cli([os.path.join(ge.GOLD, "record.gbk"), str(tmp_path / "no" / "dir" / "o.faa")])
    assert r.returncode == 255 and b"for writing." in r.stderr
