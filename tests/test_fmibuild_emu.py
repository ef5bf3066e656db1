"""The stages behind the suffix sort on the host: the per-lane functions of kaiju_amd/csrc/kj_fmibuild.h, which the kernels of
fmibuild.hip are made of, driven by tests/emu/fmibuild_emu.cpp through loops shaped like the kernels' grids, and the host
stages of mkfmi.cpp through kaiju_fmi_arrays_host.  Both must give the numpy expectation of tests/fmibuild_expect.py on every
case: every text of tests/sufsort_inputs.py; the edges of the 65 536-row pieces through `copies` and two texts beyond them;
exponents 0, 2, 3, 5 with copies 1, 3, 7.  The emulation and the host arrays also run as a stand-alone program under the address
and undefined-behaviour sanitizers (tests/tools/fmibuild_san.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fmibuild_expect as fe
import util
from kaiju_amd import build as kbuild, mkfmi

EMU_SRC = os.path.join(util.ROOT, "tests", "emu", "fmibuild_emu.cpp")


@pytest.fixture(scope="module")
def fb_emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fmibuild_emu") / "libfmibuild_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC], check=True)
    L = C.CDLL(so)
    L.fmibuild_emu.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    L.fmibuild_emu.restype = C.c_uint32
    L.fmibuild_emu_constants.argtypes = [C.c_void_p]
    L.fmibuild_emu_scratch_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    L.fmibuild_emu_scratch_bytes.restype = C.c_uint64
    L.fmibuild_emu_sort_bytes_freed.argtypes = [C.c_uint64]
    L.fmibuild_emu_sort_bytes_freed.restype = C.c_uint64
    L.fmibuild_emu_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
    return L


def run_emu(L, name, copies, exponent, recode=True):
    want = fe.expected(name, copies, exponent)
    text, sa = np.ascontiguousarray(fe.text(name)), np.ascontiguousarray(fe.suffix_array(name))
    rows = want["bwtlen"]
    nblk, npieces = (rows + 255) >> 8, (rows + 65535) >> 16
    out = {"read_of_rank": np.full(max(1, want["nseq"]), 0xeeeeeeee, dtype=np.uint32), "samples": np.full(max(1, len(want["samples"])), 0xee, dtype=np.uint8),
           "bwt": np.full(rows, 0xee, dtype=np.uint8), "piece_counts": np.full(npieces * 21, 0xeeeeeeee, dtype=np.uint32),
           "index2_rows": np.full(nblk * 21, 0xeeee, dtype=np.uint16)}
    sl = np.ascontiguousarray(want["startLcode"], dtype=np.int32)
    bad = L.fmibuild_emu(text.ctypes.data, len(text), sa.ctypes.data if len(sa) else None, copies, exponent, sl.ctypes.data, int(recode),
                         *[out[k].ctypes.data for k in ("read_of_rank", "samples", "bwt", "piece_counts", "index2_rows")])
    out["read_of_rank"], out["samples"] = out["read_of_rank"][:want["nseq"]], out["samples"][:len(want["samples"])]
    return bad, out


def test_constants_and_scratch(fb_emu):
    k = np.zeros(8, dtype=np.uint64)
    fb_emu.fmibuild_emu_constants(k.ctypes.data)
    assert [int(x) for x in k] == [256, 65536, 21, 256, 8, 32, 31, 256]
    assert k[3] * k[0] == k[1]                           # a lane per 256-row block of a piece
    # per symbol with copies = 1, exponent 3: B 1 + samples 1/8 x nbytes + index2 42 / 256 + piece counts 84 / 65 536, and 12 bytes a sequence
    tlen, nseq = 10**6 + 2500, 2500
    got = fb_emu.fmibuild_emu_scratch_bytes(tlen, nseq, 1, 3)
    nbytes = (7 + nseq.bit_length() + tlen.bit_length()) // 8
    want = tlen + (tlen >> 3) * nbytes + 42 * tlen / 256 + 84 * tlen / 65536 + 12 * nseq
    assert want <= got <= want + 4096
    # copies: the replicated BWT is a second array; about 8.8 T rows are 8 TiB and more
    assert fb_emu.fmibuild_emu_scratch_bytes(tlen, nseq, 3, 3) >= got + 3 * tlen
    assert fb_emu.fmibuild_emu_scratch_bytes(4097, 1, 2**31 - 2, 3) > 8 << 40
    assert fb_emu.fmibuild_emu_sort_bytes_freed(10**6) == 16 * 10**6


@pytest.mark.parametrize("name,copies,exponent", fe.CASES, ids=fe.CASE_IDS)
def test_plan_is_the_expectations(fb_emu, name, copies, exponent):
    want, t = fe.expected(name, copies, exponent), fe.text(name)
    plan = np.zeros(13, dtype=np.int64)
    from sufsort_inputs import maxlen
    fb_emu.fmibuild_emu_plan(len(t), want["nseq"], maxlen(t), copies, exponent, plan.ctypes.data)
    otlen, onseq, first, nsamp, nfill, nblk, npieces, ncheck, sbits, pbits, nbytes, N1, N2 = (int(x) for x in plan)
    assert (otlen, onseq, ncheck, sbits, pbits, nbytes, N1, N2) == (want["bwtlen"], want["nseq"] * copies, want["ncheck"], want["sbits"], want["pbits"],
                                                                  want["nbytes"], want["N1"], want["N2"])
    step = 1 << exponent
    assert first % step == 0 and onseq <= first < onseq + step
    assert nsamp == len(range(first, otlen, step)) and nfill == min(nsamp, max(ncheck, 0))
    assert nblk == -(-otlen // 256) and npieces == -(-otlen // 65536)


@pytest.mark.parametrize("name,copies,exponent", fe.CASES, ids=fe.CASE_IDS)
def test_emulation_gives_the_expectation(fb_emu, name, copies, exponent):
    want = fe.expected(name, copies, exponent)
    for recode in (True, False):
        bad, got = run_emu(fb_emu, name, copies, exponent, recode)
        assert bad == 0, f"violations {bad:#x}"
        for k in ("read_of_rank", "samples"):
            assert np.array_equal(got[k], want[k]), k
        w = want["bwt"] if recode else want["bwt_raw"]
        d = np.flatnonzero(got["bwt"] != w)
        assert len(d) == 0, ("bwt", recode, "first difference at row", int(d[0]), int(got["bwt"][d[0]]), int(w[d[0]]))
    # the piece counts are the letters of every 65 536 rows; index2's rows those of the file, where the file's last row does not lie over one
    rows = want["bwtlen"]
    npieces, nblk = (rows + 65535) >> 16, (rows + 255) >> 8
    counts = np.stack([np.bincount(want["bwt_raw"][R << 16:(R + 1) << 16], minlength=21) for R in range(npieces)])
    assert np.array_equal(got["piece_counts"].reshape(npieces, 21), counts)
    keep = min(nblk, want["N2"] - 1)
    assert np.array_equal(got["index2_rows"][:keep * 21], want["index2"][:keep * 21])
    assert np.array_equal(got["index2_rows"].reshape(nblk, 21)[0], np.zeros(21))


@pytest.mark.parametrize("name,copies,exponent", fe.CASES, ids=fe.CASE_IDS)
def test_host_stages_give_the_expectation(name, copies, exponent):
    want = fe.expected(name, copies, exponent)
    for recode in (True, False):
        got, stats = mkfmi.fmi_arrays(fe.text(name), copies=copies, exponent=exponent, recode=recode, threads=3)
        assert stats is None
        assert fe.first_difference(got, want, recode=recode) is None, (recode, fe.first_difference(got, want, recode=recode))


def test_cases_reach_the_edges_they_are_there_for():
    rows = {(n, c): len(fe.text(n)) * c for n, c, _ in fe.CASES}
    assert {rows[("iid_4095", 16)], rows[("iid_4096", 16)], rows[("iid_4097", 16)], rows[("iid_4097", 17)]} == {65520, 65536, 65552, 69649}
    assert rows[("big_65537", 1)] == 65537 and rows[("big_131073", 1)] == 131073
    # a letter's count passes the top of its code range (the coding saturates) in the first and in the second half of a block:
    # on the one-letter texts for the terminator, which gets two codes there, and on an i.i.d. text
    for name in ("code_20_only", "identical_40x300A", "iid_4097"):
        w = fe.expected(name, 1, 3)
        top = np.diff(w["startLcode"]) - 1
        halves = set()
        for b in range(0, w["bwtlen"], 256):
            for h, rows in enumerate((w["bwt_raw"][b:b + 128], w["bwt_raw"][b + 128:b + 256])):
                if np.any(np.bincount(rows, minlength=21) - 1 > top):
                    halves.add(h)
        print(name, "saturates in halves", sorted(halves))
        assert halves == ({0, 1} if name != "code_20_only" else set()), name      # (75 letters and one terminator: nothing to saturate)
    # samples on rows r * copies + t with t != 0, and more samples than the header's count as well as fewer
    seen = set()
    for n, c, e in fe.CASES:
        w = fe.expected(n, c, e)
        first = -(-(w["nseq"] * c) // (1 << e)) * (1 << e)
        nsamp = len(range(first, w["bwtlen"], 1 << e))
        seen.add("more" if nsamp > w["ncheck"] else "fewer" if nsamp < w["ncheck"] else "equal")
        if c > 1 and any((first + (q << e)) % c for q in range(min(nsamp, 8))):
            seen.add("t != 0")
    assert {"more", "fewer", "equal", "t != 0"} <= seen
    assert len({fe.expected("iid_4097", c, 3)["nbytes"] for c in (1, 3, 7, 16, 17)} | {fe.expected("sequences_of_length_1", c, 3)["nbytes"] for c in (1, 3, 7)}) > 1


def test_arrays_entry_points_refuse_bad_texts():
    L = mkfmi._lib()
    a = mkfmi.FmiArrays()
    for t in (np.array([1, 2, 3], dtype=np.uint8), np.array([1, 21, 0], dtype=np.uint8)):
        assert L.kaiju_fmi_arrays_sizes(t.ctypes.data, len(t), 1, 3, C.byref(a)) == -1
    t = np.array([1, 2, 0], dtype=np.uint8)
    assert L.kaiju_fmi_arrays_sizes(t.ctypes.data, 0, 1, 3, C.byref(a)) == -1
    assert L.kaiju_fmi_arrays_sizes(t.ctypes.data, len(t), 0, 3, C.byref(a)) == -1
    assert L.kaiju_fmi_arrays_sizes(t.ctypes.data, len(t), 1, 21, C.byref(a)) == -1
    assert L.kaiju_fmi_arrays_sizes(t.ctypes.data, len(t), 1, 3, C.byref(a)) == 0 and a.bwtlen == 3 and a.nseq == 1
    assert L.kaiju_fmi_arrays_host(t.ctypes.data, len(t), 1, 3, 1, 1, C.byref(a)) == -1          # no buffers
    with pytest.raises(ValueError):
        mkfmi.build_fmi("x.faa", "x.fmi", stages="device")                                       # needs a device
    with pytest.raises(ValueError):
        mkfmi.build_fmi("x.faa", "x.fmi", device=0, stages="gpu")


def test_the_host_library_has_the_arrays_but_no_device_entry_points():
    L = C.CDLL(kbuild.build_mkfmi())
    assert hasattr(L, "kaiju_fmi_arrays_sizes") and hasattr(L, "kaiju_fmi_arrays_host")
    assert not hasattr(L, "kaiju_build_fmi_device_ex") and not hasattr(L, "kaiju_fmi_arrays_device")
    needed = subprocess.run(["readelf", "-d", kbuild.MKFMI_LIB], capture_output=True, text=True, check=True).stdout
    assert "amdhip" not in needed and "hsa" not in needed


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """a plain executable of its own: nothing is loaded into this process"""
    exe = str(tmp_path / "fmibuild_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-o", exe, os.path.join(util.ROOT, "tests", "tools", "fmibuild_san.cpp"), EMU_SRC,
                    os.path.join(util.ROOT, "kaiju_amd", "csrc", "mkfmi.cpp"), "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout.rstrip().endswith(b" ok"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
