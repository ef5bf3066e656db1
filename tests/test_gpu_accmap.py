"""The accession map on the device (kaiju_amd/csrc/accmap.hip) through the C-ABI: the map file of tests/golden/convert (the
reference tool pins what it means: tests/test_convert_expect_golden.py) and the cases below against tests/convert_expect.py -
no and one entry, eight slots with probes that wrap, growth by rehash and reallocation over many small blocks, keys of every
length class, prefixes, duplicates across calls in both orders of validity, one block against many, keys only, the refusals."""
import ctypes as C

import numpy as np
import pytest

import convert_expect as ce
from kaiju_amd import api
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

NODES = ce.GOLD + "/nodes.dmp"


@pytest.fixture(scope="module")
def tree(gpu_lib):
    host = gpu_lib.Taxonomy(NODES)
    dtax = gpu_lib.DeviceTaxonomy(host, 0)
    yield dtax
    dtax.close()


@pytest.fixture(scope="module")
def fx():
    return ce.Fixture()


def pairs():
    return ce.merged_pairs(ce.golden("merged.dmp"))


def blocks_of(text, size):
    out, at = [], 0
    while at < len(text):
        end = text.find(b"\n", min(len(text) - 1, at + size)) + 1
        end = end if end > 0 else len(text)
        out.append(text[at:end])
        at = end
    return out


def check(m, model, keys, what=""):
    keys = sorted(set(keys))
    got = m.lookup(keys)
    for k, t in zip(keys, got):
        assert t == model.lookup(k), (what, k, t)
    st = m.info()
    assert (int(st["entries"]), int(st["lines"]), int(st["lines_no_insert"]), int(st["duplicates"])) == (len(model.map), model.lines, model.no_insert, model.duplicates), what
    assert int(st["probe_hist"].sum()) == int(st["entries"]) and int(st["entries"]) * 4 <= int(st["slots"]) * 3 and not st["reserved"].any()
    assert int(st["arena_bytes"]) >= sum(24 + (len(k) + 7) // 8 * 8 for k in model.map) and int(st["arena_bytes"]) <= int(st["arena_cap"])
    return st


def all_keys(text):
    lines = ce.getlines(text)
    return {ce.map_line(l)[0] for l in lines} | set(lines) | {b"nope", b"", b"A1", b"A1.1x"}


def test_the_map_file_of_the_fixture_in_one_block_and_in_many(tree, fx):
    text = ce.golden("map.tsv")
    answers = []
    for size, slots in ((len(text), 0), (len(text), 8), (64, 8), (1, 8)):
        m = api.AccMap(tree, pairs(), initial_slots=slots)
        for k, b in enumerate(blocks_of(text, size)):
            m.add_text(b, first_block=k == 0)
        st = check(m, fx.model, all_keys(text), (size, slots))
        assert (int(st["rehashes"]) >= 1) == (slots == 8)
        answers.append(m.lookup(sorted(all_keys(text))))
        m.close()
    assert all(a == answers[0] for a in answers)
    assert answers[0][sorted(all_keys(text)).index(b"A6.1")] == 1236


def test_no_entry_and_one_entry(tree, fx):
    m = api.AccMap(tree, pairs(), initial_slots=8)
    assert m.lookup([b"A", b""]) == [ce.MISS, ce.MISS] and int(m.info()["entries"]) == 0
    m.add_text(b"", first_block=True)
    m.add_text(b"only the header line\n", first_block=True)
    m.add_text(b"\n\n", first_block=False)
    assert m.lookup([b"A", b""]) == [ce.MISS, ce.MISS] and int(m.info()["entries"]) == 0 and int(m.info()["lines"]) == 0
    m.add_text(b"x\tA\t562", first_block=False)
    model = ce.Model(fx.nodes, fx.merged).add_text(b"x\tA\t562", first_block=False)
    check(m, model, [b"A", b"", b"x", b"AA"])
    assert m.lookup([b"A"]) == [562]
    m.close()


def test_eight_slots_and_six_keys_whose_probes_wrap(tree, fx):
    keys = ce.keys_with_late_homes(6)                           # (the model's hash is pinned on the header's in tests/test_convert_emu.py)
    m = api.AccMap(tree, pairs(), initial_slots=8)
    m.add_text(b"".join(b"x\t%s\t%d\n" % (key, 561 + (i & 1)) for i, key in enumerate(keys)), first_block=False)
    st = m.info()
    assert int(st["slots"]) == 8 and int(st["entries"]) == 6 and int(st["rehashes"]) == 0
    assert int(st["probe_hist"][2:].sum()) >= 3                 # six keys on two homes: at least three need three probes or more
    assert m.lookup(keys + [b"W", b"nope"]) == [561 + (i & 1) for i in range(6)] + [ce.MISS, ce.MISS]
    m.add_text(b"x\tseventh\t564\n", first_block=False)         # 7 of 8 would be above 3/4: the table grows
    assert int(m.info()["slots"]) == 16 and m.lookup(keys + [b"seventh"]) == [561 + (i & 1) for i in range(6)] + [564]
    m.close()


def test_growth_from_eight_slots_to_thousands_of_keys_in_small_blocks(tree, fx):
    rng = np.random.RandomState(3)
    taxa = [b"562", b"564", b"1423", b"666", b"777", b"9606", b"-1", b"12345"]
    lines = [b"a%d\tACC%06d.%d\t%s\t%d\n" % (k, rng.randint(0, 2500), rng.randint(1, 3), taxa[rng.randint(len(taxa))], k) for k in range(4000)]
    text = b"".join(lines)
    model = ce.Model(fx.nodes, fx.merged).add_text(text, first_block=False)
    assert len(model.map) > 2000 and model.duplicates > 300 and model.no_insert > 500
    m = api.AccMap(tree, pairs(), initial_slots=8)
    for at in range(0, len(lines), 7):
        m.add_text(b"".join(lines[at:at + 7]), first_block=False)
    st = check(m, model, all_keys(text), "grown")
    # (a rehash at most quadruples the slots - the table was at most 3/4 full and a block adds 7 keys - so 8 -> 4096 takes five)
    assert int(st["rehashes"]) >= 5 and int(st["slots"]) >= 4096 and int(st["arena_cap"]) > 1 << 16
    one = api.AccMap(tree, pairs())
    one.add_text(text, first_block=False)
    keys = sorted(all_keys(text))
    assert one.lookup(keys) == m.lookup(keys)
    again = api.AccMap(tree, pairs())                          # two runs over the same input answer alike
    again.add_text(text, first_block=False)
    assert again.lookup(keys) == one.lookup(keys)
    for x in (m, one, again):
        x.close()


def test_keys_of_every_length_class_prefixes_and_last_bytes(tree, fx):
    keys = [b"", b"A", b"A" * 15, b"A" * 16, b"A" * 17, b"A" * 33, b"A" * 32 + b"B", b"A" * 15 + b"B", b"A" * 16 + b"B", b"B" * 200, b"B" * 199 + b"C", b"A\x01 x"]
    text = b"".join(b"k\t%s\t%d\n" % (k, (561, 562, 564)[i % 3]) for i, k in enumerate(keys))
    model = ce.Model(fx.nodes, fx.merged).add_text(text, first_block=False)
    m = api.AccMap(tree, pairs(), initial_slots=8).add_text(text, first_block=False)
    check(m, model, keys + [b"AA", b"A" * 14, b"A" * 18, b"A" * 32, b"A" * 32 + b"C", b"B" * 199, b"B" * 201, b"A\x01"])
    assert m.lookup(keys) == [(561, 562, 564)[i % 3] for i in range(len(keys))]
    m.close()


def test_a_duplicate_across_two_calls_in_both_orders_of_validity(tree, fx):
    for first, second, want in ((b"x\tK\t562\n", b"x\tK\t564\n", 562), (b"x\tK\t55555\n", b"x\tK\t564\n", 564), (b"x\tK\t564\n", b"x\tK\t55555\n", 564),
                                (b"x\tK\t-1\n", b"x\tK\t666\n", 562)):
        m = api.AccMap(tree, pairs(), initial_slots=8).add_text(first, first_block=False).add_text(second, first_block=False)
        model = ce.Model(fx.nodes, fx.merged).add_text(first, first_block=False).add_text(second, first_block=False)
        check(m, model, [b"K", b"x"], (first, second))
        assert m.lookup([b"K"]) == [want]
        m.close()
    # in one block, far apart: the first line wins whatever lane got there first
    lines = [b"x\tK%d\t562\n" % (k % 50) for k in range(3000)] + [b"x\tK%d\t564\n" % (k % 50) for k in range(3000)]
    m = api.AccMap(tree, pairs(), initial_slots=8).add_text(b"x\tK7\t1423\n" + b"".join(lines), first_block=False)
    assert m.lookup([b"K%d" % k for k in range(50)]) == [1423 if k == 7 else 562 for k in range(50)]
    assert int(m.info()["duplicates"]) == 6001 - 50
    m.close()


def test_keys_only_the_excluded_set(gpu_lib, fx):
    m = api.AccMap(None).add_keys(ce.golden("excl.txt"), value=1)
    assert m.lookup([b"E1.1", b"A4.1", b"", b"E1.1 ", b"A4.1x"]) == [1, 1, ce.MISS, ce.MISS, ce.MISS]
    m.add_keys(b"x\ty\t562\r\nlast", value=9)
    assert m.lookup([b"x\ty\t562\r", b"last", b"y", b"E1.1"]) == [9, 9, ce.MISS, 1] and int(m.info()["entries"]) == 4
    m.close()


def test_the_device_pointer_form(tree, fx):
    hip = Hip()
    text = ce.golden("map.tsv")
    d = hip.malloc(len(text) + 64)
    hip.h2d(d, np.frombuffer(text, dtype=np.uint8))
    m = api.AccMap(tree, pairs(), initial_slots=8)
    m.add_text_device(d, len(text), first_block=True)
    check(m, fx.model, all_keys(text), "device")
    m.close()
    hip.free(d)


def test_refusals(gpu_lib, tree):
    L = gpu_lib.lib()
    h = C.c_void_p()
    assert L.kaiju_gpu_accmap_create(tree._h, 0, None, 0, 1, 2, 0, None) == -1
    assert L.kaiju_gpu_accmap_create(tree._h, 0, None, 3, 1, 2, 0, C.byref(h)) == -1
    assert L.kaiju_gpu_accmap_create(tree._h, 0, None, 0, 0, 2, 0, C.byref(h)) != 0 and b"column" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_accmap_create(tree._h, 0, None, 0, 1, 2, 1 << 41, C.byref(h)) == -1
    assert L.kaiju_gpu_accmap_create(tree._h, 1 if gpu_lib.device_count() == 1 else 7, None, 0, 1, 2, 0, C.byref(h)) == -1 and not h.value
    m = api.AccMap(tree, pairs())
    hip = Hip()
    d = hip.malloc(256)
    hip.memset(d, 256)
    assert L.kaiju_gpu_accmap_add_text(m._h, None, 5, 1) == -1 and L.kaiju_gpu_accmap_add_text(None, b"x", 1, 1) == -1
    assert L.kaiju_gpu_accmap_add_text_device(m._h, d + 4, 16, 0) == -1 and b"16-byte aligned" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_accmap_add_text_device(m._h, d, 0xfffffff1, 0) == -1 and b"2^32" in L.kaiju_gpu_last_error()
    assert L.kaiju_gpu_accmap_add_text_device(m._h, None, 16, 0) == -1
    n = C.c_uint64()
    assert L.kaiju_gpu_accmap_lookup(m._h, b"a\n", 2, None, 4, C.byref(n)) == -1 and L.kaiju_gpu_accmap_lookup(m._h, b"a\n", 2, None, 0, None) == -1
    assert L.kaiju_gpu_accmap_info(m._h, None) == -1
    assert L.kaiju_gpu_accmap_pass_ms(m._h, np.zeros(5, dtype=np.float32).ctypes.data, 5) != 0 and b"KAIJU_GPU_CONVERT_TIMES" in L.kaiju_gpu_last_error()
    keys_only = api.AccMap(None)
    assert L.kaiju_gpu_accmap_add_text(keys_only._h, b"a\tb\t1\n", 6, 0) == -1 and b"keys only" in L.kaiju_gpu_last_error()
    assert int(m.info()["entries"]) == 0
    for x in (m, keys_only):
        x.close()
    hip.free(d)


def test_pass_times(gpu_lib, tree, monkeypatch):
    monkeypatch.setenv("KAIJU_GPU_CONVERT_TIMES", "1")
    m = api.AccMap(tree, pairs())
    monkeypatch.delenv("KAIJU_GPU_CONVERT_TIMES")
    m.add_text(ce.golden("map.tsv"))
    ms = m.pass_ms()
    assert len(ms) == api.ACCMAP_PASSES and (ms >= 0).all() and ms.sum() > 0
    m.close()
