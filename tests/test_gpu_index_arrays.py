"""Every array the loader derives in HBM - k-mer table (k_kmer_extend, k_kmer_extend_wide), k-mer lines (k_kline_build), text,
suffix array and text positions (k_suffix_walk, k_text_build, k_seq_walk_len, k_seq_walk_fill), the taxon of every row
(k_row_tax), rank blocks and samples packed on the host or on the device (fmi_stream.hip) - read back with
kaiju_gpu_index_read_array and compared, element by element, with answers derived from the index file and its FASTA alone
(index_truth.py; test_index_arrays.py runs the same comparison on the host pack).
"""
import ctypes as C
import os

import numpy as np
import pytest

import index_truth as it

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def indexes(tmp_path_factory, oracle, golden):
    """A: the golden index; B, D, C: index_truth.make_index_b / _c.  name -> (fmi, Truth), the reference computed once"""
    d = tmp_path_factory.mktemp("index_arrays")
    files = {"A": (golden.fmi, os.path.join(golden.dir, "db.faa")), "B": it.make_index_b(d), "C": it.make_index_c(d),
             "D": it.make_index_b(d, align64=True)}
    return {name: (fmi, it.Truth(oracle, fmi, faa)) for name, (fmi, faa) in files.items()}


KNOBS = ("KAIJU_GPU_FORCE_WIDE", "KAIJU_GPU_FMI_STREAM", "KAIJU_GPU_STREAM_PIECE_KB", "KAIJU_GPU_KMER", "KAIJU_GPU_TV_SHIFT",
         "KAIJU_GPU_ROW_TAX", "KAIJU_GPU_NO_TEXT", "KAIJU_GPU_KEEP_KMER_TABLE")


def load_and_compare(api, name, fmi, T, env, id_mode=0):
    """one load in one configuration: preconditions from the reference, then every array; -> (layout, names compared)"""
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update({k: v for k, v in env.items() if v is not None})
    try:
        ix = api.Index(fmi, device=0, id_mode=id_mode)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    try:
        it.check_preconditions(name, T, ix.info.warnings)
        lay = it.Layout.from_buffer_copy(bytes(ix.layout()))
        with pytest.raises(api.KaijuGpuError):                      # (one byte beyond an array)
            ix.read_array("rank_blocks", 1, lay.size("rank_blocks"))
        checked = it.compare_index(T, lay, ix.read_array, ids_sequence=id_mode == api.IDS_SEQUENCE)
        assert checked == lay.present(), (sorted(lay.present() - checked), "reported but not compared")
        return lay, checked
    finally:
        ix.close()


SMALL = {"rank_blocks", "sa_seq", "term_rows", "seq_taxid", "seq_valid", "kmer_table"}
TEXT_NARROW = {"sa_taxid", "kmer_lines", "text", "sa_full", "row_tax", "tax_of_dense"}


@pytest.mark.parametrize("k", ["2", "4", "5"])
@pytest.mark.parametrize("stream", ["0", "1"])
@pytest.mark.parametrize("wide", [None, "16", "20"])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_device_arrays(gpu_lib, indexes, name, wide, stream, k):
    fmi, T = indexes[name]
    env = {"KAIJU_GPU_FORCE_WIDE": wide, "KAIJU_GPU_FMI_STREAM": stream, "KAIJU_GPU_KMER": k,
           "KAIJU_GPU_STREAM_PIECE_KB": "16" if stream == "1" else None}
    lay, checked = load_and_compare(gpu_lib, name, fmi, T, env)
    assert lay.kmer_k == int(k) and bool(lay.wide) == (wide is not None)
    want = SMALL | ({"count_bases"} if wide else TEXT_NARROW)
    if wide and name != "B":                                  # (no text arrays on a wide index with the short sample array)
        want |= {"text", "sa_full", "row_tax", "tax_of_dense"}
    assert checked == want


@pytest.mark.parametrize("stream", ["0", "1"])
def test_device_arrays_k6(gpu_lib, indexes, stream):
    """six-letter words on the golden index, narrow.  From the host pack the host builds the table and the device its 20^5
    lines; streamed, the device grows every level, keeps the five-letter table next to the lines and frees the deep one
    (the production shape).  410 MB of lines are read back: the lines that are not all zero are found with one reduction"""
    fmi, T = indexes["A"]
    lay, checked = load_and_compare(gpu_lib, "A", fmi, T, {"KAIJU_GPU_FMI_STREAM": stream, "KAIJU_GPU_KMER": "6",
                                                           "KAIJU_GPU_STREAM_PIECE_KB": "16" if stream == "1" else None})
    assert lay.kline_k == 6 and lay.kmer_k == (5 if stream == "1" else 6)
    assert checked == SMALL | TEXT_NARROW


@pytest.mark.parametrize("row_tax", ["1", "0"])
@pytest.mark.parametrize("tv", ["0", "1", "3", "-1"])
@pytest.mark.parametrize("name", ["B", "C", "D"])
def test_device_arrays_wide_text(gpu_lib, indexes, name, tv, row_tax):
    fmi, T = indexes[name]
    env = {"KAIJU_GPU_FORCE_WIDE": "16", "KAIJU_GPU_KMER": "3", "KAIJU_GPU_FMI_STREAM": "0", "KAIJU_GPU_TV_SHIFT": tv,
           "KAIJU_GPU_ROW_TAX": row_tax}
    lay, checked = load_and_compare(gpu_lib, name, fmi, T, env)
    want = SMALL | {"count_bases"}
    if name != "B":
        if tv != "-1":
            want |= {"text", "sa_full"}
            assert lay.tv_shift == int(tv)
        if row_tax == "1":
            want |= {"row_tax", "tax_of_dense"}
    assert checked == want


@pytest.mark.parametrize("wide", [None, "16"])
def test_device_arrays_sequence_ids(gpu_lib, indexes, wide):
    """KAIJU_GPU_IDS_SEQUENCE (kaijux / kaijup): the id of a row is its sequence number, every name is usable"""
    fmi, T = indexes["C"]
    lay, checked = load_and_compare(gpu_lib, "C", fmi, T, {"KAIJU_GPU_FORCE_WIDE": wide, "KAIJU_GPU_KMER": "3"},
                                    id_mode=gpu_lib.IDS_SEQUENCE)
    assert "row_tax" in checked and lay.n_dense == T.nseq
