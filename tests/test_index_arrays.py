"""Every array of the HOST pack of an index (host_index.cpp: PackedIndex::build, build_kmer_table, build_klines, build_text,
build_text_wide - what the test emulation searches, and what a host-pack load uploads) against answers derived from the index
file and its FASTA alone (index_truth.py): rank blocks, SA sample, k-mer table and lines, text, text positions, the taxon of
every row.  The device's own arrays: test_gpu_index_arrays.py, with the same comparison."""
import ctypes as C
import os

import numpy as np
import pytest

import index_truth as it
import util


@pytest.fixture(scope="module")
def indexes(tmp_path_factory, oracle, golden, emu):
    """A: the golden index; B, D, C: index_truth.make_index_b / _c.  name -> (fmi, Truth), the reference computed once"""
    d = tmp_path_factory.mktemp("index_arrays")
    files = {"A": (golden.fmi, os.path.join(golden.dir, "db.faa")), "B": it.make_index_b(d), "C": it.make_index_c(d),
             "D": it.make_index_b(d, align64=True)}
    out = {}
    for name, (fmi, faa) in files.items():
        T = it.Truth(oracle, fmi, faa)
        h = emu.load(fmi)
        it.check_preconditions(name, T, emu.lib.emu_index_warnings(h))
        emu.lib.emu_index_free(h)
        out[name] = (fmi, T)
    return out


def test_reference_self_checks(indexes):
    """the reference against the oracle's own UpdateSI (2 000 words per k); its FASTA closure, ko_get_suffix and ko_initial_si
    checks ran when the fixture built it"""
    for name, (_, T) in indexes.items():
        for k in (2, 3, 4, 5):
            T.spot_check_kmers(k)
    assert indexes["A"][1].bwtlen % 64 != 0


def emu_arrays(emu, fmi, env, xmode=False):
    """load through the emulation with `env`; -> (layout, read(name))"""
    E = emu.lib
    E.emu_index_load_x.restype = C.c_void_p
    E.emu_index_load_x.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    E.emu_index_get_layout.argtypes = [C.c_void_p, C.POINTER(it.Layout)]
    E.emu_index_read_array.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: v for k, v in env.items() if v is not None})
    try:
        err = C.create_string_buffer(512)
        h = (E.emu_index_load_x if xmode else E.emu_index_load)(fmi.encode(), err, 512)
        assert h, err.value
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    lay = it.Layout()
    assert E.emu_index_get_layout(h, C.byref(lay)) == 0

    def read(name):
        w = it.ARRAYS.index(name)
        buf = np.empty(lay.size(name), dtype=np.uint8)
        assert E.emu_index_read_array(h, w, 0, len(buf), buf.ctypes.data) == 0
        assert E.emu_index_read_array(h, w, 1, len(buf), buf.ctypes.data) == -1          # (one byte beyond the array)
        return buf
    return h, lay, read


CONFIGS = [(ix, wide, k) for ix in "ABCD" for wide in (None, "16", "20") for k in ("2", "4", "5")]


@pytest.mark.parametrize("name,wide,k", CONFIGS)
def test_host_pack(indexes, emu, name, wide, k):
    fmi, T = indexes[name]
    h, lay, read = emu_arrays(emu, fmi, {"KAIJU_GPU_FORCE_WIDE": wide, "KAIJU_GPU_KMER": k})
    try:
        checked = it.compare_index(T, lay, read)
        assert checked == lay.present(), (sorted(lay.present() - checked), "reported but not compared")
        assert lay.kmer_k == int(k) and bool(lay.wide) == (wide is not None)
        want = {"rank_blocks", "sa_seq", "term_rows", "seq_taxid", "seq_valid", "kmer_table"}
        want |= {"count_bases"} if wide else {"sa_taxid", "kmer_lines", "text", "sa_full", "row_tax", "tax_of_dense"}
        if wide and name != "B":                              # (no text arrays on a wide index with the short sample array)
            want |= {"text", "sa_full", "row_tax", "tax_of_dense"}
        assert checked == want
    finally:
        emu.lib.emu_index_free(h)


@pytest.mark.parametrize("name", ["B", "C", "D"])
@pytest.mark.parametrize("tv", ["0", "1", "3"])
@pytest.mark.parametrize("row_tax", [True, False])
def test_host_pack_wide_text(indexes, emu, name, tv, row_tax):
    fmi, T = indexes[name]
    env = {"KAIJU_GPU_FORCE_WIDE": "16", "KAIJU_GPU_KMER": "3", "KAIJU_EMU_TV_SHIFT": tv,
           "KAIJU_EMU_NO_ROW_TAX": None if row_tax else "1"}
    h, lay, read = emu_arrays(emu, fmi, env)
    try:
        checked = it.compare_index(T, lay, read)
        assert checked == lay.present()
        if name != "B":
            assert lay.tv_shift == int(tv) and {"text", "sa_full"} <= checked and ("row_tax" in checked) == row_tax
        else:
            assert not ({"text", "sa_full", "row_tax"} & checked)
    finally:
        emu.lib.emu_index_free(h)


@pytest.mark.parametrize("wide", [None, "16"])
def test_host_pack_sequence_ids(indexes, emu, wide):
    """kaijux / kaijup ids: the id of a row is its sequence number, every name is usable"""
    fmi, T = indexes["C"]
    h, lay, read = emu_arrays(emu, fmi, {"KAIJU_GPU_FORCE_WIDE": wide, "KAIJU_GPU_KMER": "3"}, xmode=True)
    try:
        checked = it.compare_index(T, lay, read, ids_sequence=True)
        assert checked == lay.present() and "row_tax" in checked and lay.n_dense == T.nseq
    finally:
        emu.lib.emu_index_free(h)
