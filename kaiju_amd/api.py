"""Python mirror of the host side of the seam, over the C-ABI (include/kaiju_gpu.h).

The names follow the reference: ``Config``-like parameters (Config.hpp:33-48), an index
loaded from a ``.fmi`` file (readFMI, util.cpp:265-276), a classifier that turns batches of
reads into per-read hit records (ConsumerThread::doWork, ConsumerThread.cpp:630-749) and the
taxonomy / LCA helpers (util.cpp:79-99, 194-263).  Everything numerical happens in
``libkaiju_gpu.so``; if that library or a HIP device is missing the calls raise — there is
no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

MAX_IDS = 21
MEM, GREEDY = 0, 1


class Params(C.Structure):
    _fields_ = [("mode", C.c_int32), ("min_fragment_length", C.c_uint32),
                ("mismatches", C.c_uint32), ("min_score", C.c_uint32),
                ("seed_length", C.c_uint32), ("seg", C.c_int32),
                ("use_evalue", C.c_int32), ("input_is_protein", C.c_int32), ("min_evalue", C.c_double),
                ("max_matches_SI", C.c_uint32), ("max_match_ids", C.c_uint32)]


class IndexInfo(C.Structure):
    _fields_ = [("bwtlen", C.c_int64), ("nseq", C.c_int32), ("alen", C.c_int32),
                ("chpt_exp", C.c_int32), ("db_length", C.c_double),
                ("device_bytes", C.c_uint64), ("warnings", C.c_uint32),
                ("alphabet", C.c_char * 64)]


class IndexFootprint(C.Structure):        # kaiju_gpu_index_footprint
    _fields_ = [(k, C.c_uint64) for k in ("rank_blocks", "count_bases", "sa_seq", "sa_taxid", "seq_tables", "kmer_table",
                                          "kmer_lines", "text", "sa_full", "other", "total")] + [("kmer_k", C.c_uint32), ("wide", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


INDEX_ARRAYS = ("rank_blocks", "count_bases", "sa_seq", "sa_taxid", "term_rows", "seq_taxid", "seq_valid", "kmer_table",
                "kmer_lines", "text", "sa_full", "row_tax", "tax_of_dense")      # KAIJU_GPU_ARR_*


class IndexLayout(C.Structure):           # kaiju_gpu_index_layout
    _fields_ = [("bytes", C.c_uint64 * len(INDEX_ARRAYS)), ("C", C.c_uint64 * 22), ("bwtlen", C.c_uint64), ("n_sa", C.c_uint64),
                ("sa_skip", C.c_uint64)] + [(k, C.c_uint32) for k in
                                            ("nseq", "chpt_exp", "mb_shift", "kmer_k", "kline_k", "tv_shift", "n_dense",
                                             "beyond_lo", "beyond_n", "beyond_row", "wide", "row_tax_shift")]


class Stats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_seg_fragments", C.c_uint64), ("n_overflow_retries", C.c_uint64),
                ("error_flags", C.c_uint64),
                ("ms_translate", C.c_double), ("ms_seg", C.c_double), ("ms_search", C.c_double),
                ("ms_retry", C.c_double), ("ms_total", C.c_double)]


HIT_DTYPE = np.dtype([("best", "<u4"), ("n_ids", "<u4"), ("flags", "<u4"), ("reserved", "<u4"),
                      ("taxid", "<u8", (MAX_IDS,))])
RESULT_DTYPE = np.dtype([("taxon", "<u8"), ("best", "<u4"), ("classified", "u1"), ("pad", "u1", (3,))])
VERBOSE_DTYPE = np.dtype([("n_acc", "<u4"), ("text_len", "<u4"), ("truncated", "<u4"), ("acc_iseq", "<u4", (20,))])  # kaiju_gpu_verbose
COMPACT_DTYPE = np.dtype([("lca", "<u8"), ("best", "<u4"), ("info", "<u4")])     # kaiju_gpu_compact
SEG_FRAGMENT_DTYPE = np.dtype([("read", "<u4"), ("start", "<u4"), ("len", "<u4"), ("flagged", "<u4"), ("n", "<u4"),
                               ("overflow", "<u4"), ("n_lr", "<u4"), ("reserved", "<u4"), ("first", "<u8")])   # kaiju_gpu_seg_fragment
SEG_LOST = 0xffffffff
NAME_SPAN_DTYPE = np.dtype([("pos", "<u4"), ("len", "<u4")])                                   # kaiju_gpu_name_span
PARSE_INFO_DTYPE = np.dtype([("n_records", "<u4"), ("n_records2", "<u4"), ("max_mate_len", "<u4"), ("name_mismatch", "<u4"),
                             ("seq_bytes", "<u8"), ("overflow", "<u4"), ("reserved", "<u4")])  # kaiju_gpu_parse_info
NO_MISMATCH = 0xffffffff
FORMAT_INFO_DTYPE = np.dtype([("text_bytes", "<u8"), ("n_records", "<u4"), ("n_classified", "<u4"), ("overflow", "<u4"),
                              ("n_inexact", "<u4")])                                           # kaiju_gpu_format_info
assert NAME_SPAN_DTYPE.itemsize == 8 and PARSE_INFO_DTYPE.itemsize == 32 and FORMAT_INFO_DTYPE.itemsize == 24
FORMAT_NAMES_INFO_DTYPE = np.dtype([("text_bytes", "<u8"), ("n_records", "<u4"), ("n_classified", "<u4"), ("overflow", "<u4"), ("n_inexact", "<u4"),
                                    ("n_unknown_taxon", "<u4"), ("n_unnamed_taxon", "<u4"), ("n_dropped", "<u4"), ("reserved", "<u4")])
assert FORMAT_NAMES_INFO_DTYPE.itemsize == 40
NAMES_NAME, NAMES_PATH, NAMES_RANKS = 0, 1, 2
ANNOTATE_INFO_DTYPE = np.dtype([("text_bytes", "<u8"), ("n_lines", "<u4"), ("n_c_lines", "<u4"), ("n_annotated", "<u4"), ("n_bad_id", "<u4"),
                                ("n_unknown_taxon", "<u4"), ("n_unnamed_taxon", "<u4"), ("n_dropped", "<u4"), ("n_empty", "<u4"), ("overflow", "<u4"),
                                ("reserved", "<u4")])
assert ANNOTATE_INFO_DTYPE.itemsize == 48
MERGE_INFO_DTYPE = np.dtype([("text_bytes", "<u8"), ("used1", "<u8"), ("used2", "<u8"), ("n_pairs", "<u8"), ("count", "<u8"), ("count_c1", "<u8"),
                             ("count_c2", "<u8"), ("count_c12", "<u8"), ("count_c3", "<u8"), ("count_c1_not_c2", "<u8"), ("count_c2_not_c1", "<u8"),
                             ("stop_pair", "<u8"), ("stop_why", "<u4"), ("more_in_2", "<u4"), ("overflow", "<u4"), ("reserved", "<u4")])   # kaiju_gpu_merge_info
assert MERGE_INFO_DTYPE.itemsize == 112
MERGE_FIRST, MERGE_SECOND, MERGE_LCA, MERGE_LOWEST = 0, 1, 2, 3
MERGE_MODES = {"1": MERGE_FIRST, "2": MERGE_SECOND, "lca": MERGE_LCA, "lowest": MERGE_LOWEST}
MERGE_STOP_SCORE_WIDE = 9
TALLY_INFO_DTYPE = np.dtype([("used", "<u8"), ("n_lines", "<u8"), ("n_total", "<u8"), ("n_unclassified", "<u8"), ("n_bad_id", "<u8"),
                             ("n_unknown_taxon", "<u8"), ("n_virus", "<u8")])   # kaiju_gpu_tally_info
TALLY_ENTRY_DTYPE = np.dtype([("taxon", "<u8"), ("direct", "<u8"), ("summed", "<u8"), ("virus", "<u4"), ("reserved", "<u4")])   # kaiju_gpu_tally_entry
assert TALLY_INFO_DTYPE.itemsize == 56 and TALLY_ENTRY_DTYPE.itemsize == 32
TALLY_PASSES = 3
KRONA_INFO_DTYPE = np.dtype([("text_bytes", "<u8"), ("written_bytes", "<u8"), ("n_lines", "<u8"), ("n_written", "<u8"), ("n_unnamed_taxa", "<u8"),
                             ("n_unnamed_reads", "<u8"), ("n_unclassified", "<u8"), ("overflow", "<u4"), ("reserved", "<u4")])   # kaiju_gpu_krona_info
assert KRONA_INFO_DTYPE.itemsize == 64
KRONA_MAX_TALLIES, KRONA_PASSES = 4, 5
ACCMAP_STATS_DTYPE = np.dtype([("entries", "<u8"), ("slots", "<u8"), ("arena_bytes", "<u8"), ("arena_cap", "<u8"), ("lines", "<u8"), ("lines_no_insert", "<u8"),
                               ("duplicates", "<u8"), ("rehashes", "<u8"), ("probe_hist", "<u8", (16,)), ("reserved", "<u8", (8,))])   # kaiju_gpu_accmap_stats
CONVERT_INFO_DTYPE = np.dtype([("text_bytes", "<u8"), ("written_bytes", "<u8"), ("n_records", "<u8"), ("n_kept", "<u8"), ("dropped_excluded", "<u8"),
                               ("dropped_no_taxon", "<u8"), ("dropped_not_included", "<u8"), ("dropped_no_lca", "<u8"), ("n_entries", "<u8"), ("n_hits", "<u8"),
                               ("n_lines", "<u8"), ("overflow", "<u4"), ("reserved0", "<u4"), ("reserved", "<u8", (4,))])   # kaiju_gpu_convert_info
assert ACCMAP_STATS_DTYPE.itemsize == 256 and CONVERT_INFO_DTYPE.itemsize == 128
ACCMAP_MISS, ACCMAP_PASSES, CONVERT_PASSES = 2 ** 64 - 1, 5, 7
GBK_INFO_DTYPE = np.dtype([("text_bytes", "<u8"), ("written_bytes", "<u8"), ("n_lines", "<u8"), ("lines_kind", "<u8", (5,)), ("n_records", "<u8"), ("letters_kept", "<u8"),
                           ("letters_dropped", "<u8"), ("no_taxon_line", "<u8"), ("overflow", "<u4"), ("reserved0", "<u4"), ("reserved", "<u8", (3,))])   # kaiju_gpu_gbk_info
assert GBK_INFO_DTYPE.itemsize == 128
GBK_PASSES = 6
TABLE_EXPAND_VIRUSES, TABLE_FILTER_UNCLASSIFIED, TABLE_FULL_PATH = 1, 2, 4
assert SEG_FRAGMENT_DTYPE.itemsize == 40
assert HIT_DTYPE.itemsize == 184 and RESULT_DTYPE.itemsize == 16 and COMPACT_DTYPE.itemsize == 16


FORMAT_VERBOSE_INFO_DTYPE = np.dtype([("text_bytes", "<u8"), ("n_records", "<u4"), ("n_classified", "<u4"), ("overflow", "<u4"),
                                      ("n_inexact", "<u4"), ("n_truncated", "<u4"), ("reserved", "<u4")])   # kaiju_gpu_format_verbose_info
assert FORMAT_VERBOSE_INFO_DTYPE.itemsize == 32


class TableOptions(C.Structure):          # kaiju_table_options
    _fields_ = [("rank", C.c_char_p), ("ranks_csv", C.c_char_p), ("min_percent", C.c_float), ("min_count", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class KaijuGpuError(RuntimeError):
    pass


_lib = None


def lib():
    """Load (building if necessary) libkaiju_gpu.so.  Raises if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("KAIJU_GPU_LIB") or _build.LIB      # (KAIJU_GPU_LIB: another build of the library, A/B measurements)
    if not os.path.exists(path):
        _build.build()
    L = C.CDLL(path)
    L.kaiju_gpu_strerror.restype = C.c_char_p
    L.kaiju_gpu_last_error.restype = C.c_char_p
    L.kaiju_gpu_index_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    L.kaiju_gpu_index_get_info.argtypes = [C.c_void_p, C.POINTER(IndexInfo)]
    L.kaiju_gpu_index_free.argtypes = [C.c_void_p]
    if hasattr(L, "kaiju_gpu_index_get_footprint"):        # (an older build loaded through KAIJU_GPU_LIB for an A/B run has none)
        L.kaiju_gpu_index_get_footprint.argtypes = [C.c_void_p, C.POINTER(IndexFootprint)]
    L.kaiju_gpu_default_params.argtypes = [C.POINTER(Params), C.c_int]
    L.kaiju_gpu_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(Params)]
    L.kaiju_gpu_destroy.argtypes = [C.c_void_p]
    L.kaiju_gpu_classify_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
    L.kaiju_gpu_classify_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                                  C.c_int, C.c_void_p, C.c_void_p]
    L.kaiju_gpu_set_max_read_length.argtypes = [C.c_void_p, C.c_uint32]
    L.kaiju_gpu_synchronize.argtypes = [C.c_void_p]
    L.kaiju_gpu_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.kaiju_taxonomy_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.kaiju_taxonomy_free.argtypes = [C.c_void_p]
    L.kaiju_taxonomy_lca.restype = C.c_uint64
    L.kaiju_taxonomy_lca.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.kaiju_finalize_hits.argtypes = [C.c_void_p, C.POINTER(Params), C.c_double, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_int, C.c_void_p]
    L.kaiju_gpu_taxonomy_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.kaiju_gpu_taxonomy_free.argtypes = [C.c_void_p]
    L.kaiju_gpu_lca_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.kaiju_gpu_classify_batch_device_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kaiju_gpu_classify_batch_verbose.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_uint32]
    L.kaiju_gpu_index_seq_name.restype = C.c_char_p
    L.kaiju_gpu_index_seq_name.argtypes = [C.c_void_p, C.c_uint32]
    L.kaiju_gpu_lca_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.kaiju_finalize_compact.argtypes = [C.POINTER(Params), C.c_double, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                         C.c_void_p]
    L.kaiju_gpu_classify_batch_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                                   C.c_void_p]
    L.kaiju_gpu_set_count_ops.argtypes = [C.c_void_p, C.c_int]
    L.kaiju_gpu_parse_block_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kaiju_gpu_parse_block.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kaiju_gpu_classify_text_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int,
                                                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kaiju_gpu_format_compact_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                                  C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.kaiju_gpu_format_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                           C.c_void_p, C.c_uint64, C.c_void_p]
    L.kaiju_gpu_format_bound.restype = C.c_uint64
    L.kaiju_gpu_format_bound.argtypes = [C.c_uint64, C.c_uint32]
    L.kaiju_gpu_format_evalue_table.argtypes = [C.c_void_p, C.c_uint32]
    L.kaiju_gpu_classify_text_to_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int,
                                                  C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    if hasattr(L, "kaiju_accession_ranks"):      # (a library linked from a source list of its own may lack accessions.cpp)
        L.kaiju_accession_ranks.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    if hasattr(L, "kaiju_gpu_index_upload_accessions"):       # (an older build loaded through KAIJU_GPU_LIB for an A/B run has none)
        L.kaiju_gpu_index_upload_accessions.argtypes = [C.c_void_p]
        L.kaiju_gpu_index_accession_bytes.restype = C.c_uint64
        L.kaiju_gpu_index_accession_bytes.argtypes = [C.c_void_p]
        L.kaiju_gpu_format_verbose_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                      C.c_uint64, C.c_void_p, C.c_void_p]
        L.kaiju_gpu_format_verbose.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                               C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_classify_batch_verbose_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64,
                                                            C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p]
    if hasattr(L, "kaiju_gpu_index_upload_seq_names"):        # (likewise)
        L.kaiju_gpu_index_upload_seq_names.argtypes = [C.c_void_p]
        L.kaiju_gpu_index_seq_name_bytes.restype = C.c_uint64
        L.kaiju_gpu_index_seq_name_bytes.argtypes = [C.c_void_p]
        L.kaiju_gpu_format_seq_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.kaiju_gpu_format_seq.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_classify_batch_seq_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64,
                                                        C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p]
    if hasattr(L, "kaiju_taxon_names_load"):                  # (likewise)
        L.kaiju_taxon_names_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_void_p]
        L.kaiju_taxon_names_free.argtypes = [C.c_void_p]
        L.kaiju_taxon_names_annotation.restype = C.c_int64
        L.kaiju_taxon_names_annotation.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        L.kaiju_taxon_names_count.restype = C.c_uint64
        L.kaiju_taxon_names_count.argtypes = [C.c_void_p, C.c_int]
        L.kaiju_gpu_taxon_names_upload.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.kaiju_gpu_taxon_names_free.argtypes = [C.c_void_p]
        L.kaiju_gpu_taxon_names_max_annotation.restype = C.c_uint64
        L.kaiju_gpu_taxon_names_max_annotation.argtypes = [C.c_void_p]
        L.kaiju_gpu_taxon_names_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_format_names_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                                    C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.kaiju_gpu_format_names.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_format_names_bound.restype = C.c_uint64
        L.kaiju_gpu_format_names_bound.argtypes = [C.c_uint64, C.c_uint32, C.c_void_p]
        L.kaiju_gpu_classify_text_to_text_names.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int,
                                                            C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    if hasattr(L, "kaiju_gpu_annotator_create"):              # (likewise)
        L.kaiju_gpu_annotator_create.argtypes = [C.c_void_p, C.c_void_p]
        L.kaiju_gpu_annotator_free.argtypes = [C.c_void_p]
        L.kaiju_gpu_annotate_text_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.kaiju_gpu_annotate_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_annotate_bound.restype = C.c_uint64
        L.kaiju_gpu_annotate_bound.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    if hasattr(L, "kaiju_gpu_merger_create"):                 # (likewise)
        L.kaiju_gpu_merger_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.kaiju_gpu_merger_free.argtypes = [C.c_void_p]
        L.kaiju_gpu_merge_text_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                                  C.c_void_p]
        L.kaiju_gpu_merge_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_merge_bound.restype = C.c_uint64
        L.kaiju_gpu_merge_bound.argtypes = [C.c_uint64, C.c_uint64]
    if hasattr(L, "kaiju_gpu_tally_create"):                  # (likewise)
        L.kaiju_gpu_tally_create.argtypes = [C.c_void_p, C.c_void_p]
        L.kaiju_gpu_tally_free.argtypes = [C.c_void_p]
        L.kaiju_gpu_tally_reset.argtypes = [C.c_void_p]
        L.kaiju_gpu_tally_add_text_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        L.kaiju_gpu_tally_add_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
        L.kaiju_gpu_tally_result.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.kaiju_gpu_tally_pass_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    if hasattr(L, "kaiju_gpu_krona_create"):                  # (likewise)
        L.kaiju_gpu_krona_create.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        L.kaiju_gpu_krona_free.argtypes = [C.c_void_p]
        L.kaiju_gpu_krona_text_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.kaiju_gpu_krona_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_krona_pass_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    if hasattr(L, "kaiju_gpu_accmap_create"):                 # (likewise)
        L.kaiju_gpu_accmap_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_accmap_free.argtypes = [C.c_void_p]
        L.kaiju_gpu_accmap_add_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        L.kaiju_gpu_accmap_add_text_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        L.kaiju_gpu_accmap_add_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]
        L.kaiju_gpu_accmap_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_accmap_info.argtypes = [C.c_void_p, C.c_void_p]
        L.kaiju_gpu_accmap_pass_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.kaiju_gpu_converter_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.kaiju_gpu_converter_free.argtypes = [C.c_void_p]
        L.kaiju_gpu_convert_text_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.kaiju_gpu_convert_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_convert_pass_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    if hasattr(L, "kaiju_gpu_accmap_create_rules"):           # (likewise)
        L.kaiju_gpu_accmap_create_rules.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_converter_create_rules.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "kaiju_gpu_gbk_create"):                    # (likewise)
        L.kaiju_gpu_gbk_create.argtypes = [C.c_int, C.c_void_p]
        L.kaiju_gpu_gbk_free.argtypes = [C.c_void_p]
        L.kaiju_gpu_gbk_reset.argtypes = [C.c_void_p]
        L.kaiju_gpu_gbk_text_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.kaiju_gpu_gbk_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.kaiju_gpu_gbk_pass_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    if hasattr(L, "kaiju_table_rows"):
        L.kaiju_table_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(TableOptions), C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.kaiju_gpu_get_op_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.kaiju_gpu_seg_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64,
                                        C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        L = lib()
        raise KaijuGpuError(f"{L.kaiju_gpu_strerror(rc).decode()} ({rc}): {L.kaiju_gpu_last_error().decode()}")


def default_params(mode="greedy", **kw) -> Params:
    p = Params()
    lib().kaiju_gpu_default_params(C.byref(p), GREEDY if mode in ("greedy", GREEDY) else MEM)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def device_count() -> int:
    return lib().kaiju_gpu_device_count()


CHAIN_WIN = 68                     # KAIJU_GPU_CHAIN_WIN
CHAIN_CASE_DTYPE = np.dtype([("win", "u1", (CHAIN_WIN,)), ("tx", "u1", (16,)), ("wq", "<i4"), ("pz", "<i4"), ("j", "<i4"), ("sc0", "<i4"),
                             ("thr", "<i4"), ("nmm", "<u4"), ("m", "<u4"), ("mismatches", "<u4")])   # kaiju_gpu_chain_case
assert CHAIN_CASE_DTYPE.itemsize == 116


def chain_hopeless_check(cases, device: int = 0) -> np.ndarray:
    """kaiju_gpu_chain_hopeless_check: the Greedy lane's pruning rule on the device, one answer byte per case (CHAIN_CASE_DTYPE)"""
    L = lib()
    L.kaiju_gpu_chain_hopeless_check.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    cases = np.ascontiguousarray(cases, dtype=CHAIN_CASE_DTYPE)
    out = np.zeros(len(cases), dtype=np.uint8)
    _check(L.kaiju_gpu_chain_hopeless_check(device, cases.ctypes.data, len(cases), out.ctypes.data))
    return out


IDS_TAXON, IDS_SEQUENCE = 0, 1     # kaiju_gpu_index_load_ex
U_RULE_NUCLEOTIDE, U_RULE_PROTEIN = 0, 1     # KAIJU_GPU_U_RULE_*: which unclassified reads of kaijux / kaijup get a third column


class Index:
    """FM-index resident in HBM (readFMI + Config::init of the reference)."""

    def __init__(self, fmi_path: str, device: int = 0, id_mode: int = 0):
        """id_mode IDS_SEQUENCE: hits collect database sequence numbers instead of taxon ids (kaijux / kaijup)"""
        self._h = C.c_void_p()
        L = lib()
        L.kaiju_gpu_index_load_ex.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        _check(L.kaiju_gpu_index_load_ex(fmi_path.encode(), device, id_mode, C.byref(self._h)))
        self.info = IndexInfo()
        _check(lib().kaiju_gpu_index_get_info(self._h, C.byref(self.info)))
        self.footprint = IndexFootprint()
        if hasattr(lib(), "kaiju_gpu_index_get_footprint"):
            _check(lib().kaiju_gpu_index_get_footprint(self._h, C.byref(self.footprint)))
        self.device = device

    @property
    def db_length(self):
        return self.info.db_length

    DIGEST_NAMES = ("rank_blocks", "count_bases", "sa_seq", "sa_taxid", "term_rows", "seq_taxid", "seq_valid", "kmer_table",
                    "kmer_lines", "text", "sa_full", "row_seq", "kmer_k", "C")

    def digest(self) -> dict:
        """kaiju_gpu_index_digest: a digest of every array this index holds in HBM (two loads of one index compare equal)"""
        L = lib()
        L.kaiju_gpu_index_digest.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        out = np.zeros(len(self.DIGEST_NAMES), dtype=np.uint64)
        _check(L.kaiju_gpu_index_digest(self._h, out.ctypes.data, len(out)))
        return {k: int(v) for k, v in zip(self.DIGEST_NAMES, out)}

    def seg_table_check(self):
        """kaiju_gpu_seg_table_check: (entries, mismatches) of the SEG window-probability table against the device's arithmetic"""
        L = lib()
        L.kaiju_gpu_seg_table_check.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        n, bad = C.c_uint64(), C.c_uint64()
        _check(L.kaiju_gpu_seg_table_check(self._h, C.byref(n), C.byref(bad)))
        return int(n.value), int(bad.value)

    def layout(self) -> IndexLayout:
        """kaiju_gpu_index_get_layout: bytes of every array this index holds in HBM (INDEX_ARRAYS order) and its scalars"""
        L = lib()
        L.kaiju_gpu_index_get_layout.argtypes = [C.c_void_p, C.POINTER(IndexLayout)]
        out = IndexLayout()
        _check(L.kaiju_gpu_index_get_layout(self._h, C.byref(out)))
        return out

    def read_array(self, name: str, offset: int = 0, n_bytes: int = None) -> np.ndarray:
        """kaiju_gpu_index_read_array: a slice (default: all) of one array of the index, as bytes"""
        L = lib()
        L.kaiju_gpu_index_read_array.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
        which = INDEX_ARRAYS.index(name)
        if n_bytes is None:
            n_bytes = int(self.layout().bytes[which]) - offset
        out = np.empty(n_bytes, dtype=np.uint8)
        _check(L.kaiju_gpu_index_read_array(self._h, which, offset, n_bytes, out.ctypes.data))
        return out

    @property
    def row_tax_shift(self) -> int:
        """0: the row -> taxon table of this index holds every row (or there is none); s = 1 .. 3: it holds every 2^s-th row
        (wide indexes too big for the full table, KAIJU_GPU_ROW_TAX_SHIFT)"""
        return int(self.layout().row_tax_shift)

    def upload_accessions(self) -> int:
        """kaiju_gpu_index_upload_accessions: the accession table of column 6 of kaiju -v to the device (explicit, idempotent);
        returns its bytes in HBM"""
        _check(lib().kaiju_gpu_index_upload_accessions(self._h))
        return int(lib().kaiju_gpu_index_accession_bytes(self._h))

    def upload_seq_names(self) -> int:
        """kaiju_gpu_index_upload_seq_names: the names of all sequences to the device, for the lines of kaijux / kaijup (explicit,
        idempotent); returns the table's bytes in HBM"""
        _check(lib().kaiju_gpu_index_upload_seq_names(self._h))
        return int(lib().kaiju_gpu_index_seq_name_bytes(self._h))

    def close(self):
        if self._h:
            lib().kaiju_gpu_index_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """The processes of a node, one per GPU (kaiju_gpu_comm_create): rank 0 leaves the communicator's id in `rendezvous_path`.
    gather_compact() = ONE RCCL gather of 16-byte records to `root` (kaiju_gpu_gather_compact), asynchronous on `stream`."""

    def __init__(self, rendezvous_path: str, rank: int, world: int, device: int = 0):
        L = lib()
        L.kaiju_gpu_comm_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.kaiju_gpu_comm_destroy.argtypes = [C.c_void_p]
        L.kaiju_gpu_gather_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
        L.kaiju_gpu_comm_last_error.restype = C.c_char_p
        self._h = C.c_void_p()
        rc = L.kaiju_gpu_comm_create(rendezvous_path.encode(), rank, world, device, C.byref(self._h))
        if rc != 0:
            raise KaijuGpuError(f"{L.kaiju_gpu_strerror(rc).decode()} ({rc}): {L.kaiju_gpu_comm_last_error().decode()}")
        self.rank, self.world = rank, world

    def gather_compact(self, d_send_ptr: int, n: int, d_recv_ptr: int, root: int = 0, stream: int = 0):
        L = lib()
        rc = L.kaiju_gpu_gather_compact(self._h, d_send_ptr, n, d_recv_ptr, root, stream)
        if rc != 0:
            raise KaijuGpuError(f"{L.kaiju_gpu_strerror(rc).decode()} ({rc}): {L.kaiju_gpu_comm_last_error().decode()}")

    def close(self):
        if self._h:
            lib().kaiju_gpu_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_index_image(fmi_path: str, image_path: str):
    """pack a .fmi once into the HBM layout and write it as a device image (loads with Index(image_path))"""
    L = lib()
    L.kaiju_gpu_index_write_image.argtypes = [C.c_char_p, C.c_char_p]
    _check(L.kaiju_gpu_index_write_image(fmi_path.encode(), image_path.encode()))


class Taxonomy:
    def __init__(self, nodes_dmp: str):
        self._h = C.c_void_p()
        _check(lib().kaiju_taxonomy_load(nodes_dmp.encode(), C.byref(self._h)))

    def lca(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.uint64)
        return int(lib().kaiju_taxonomy_lca(self._h, a.ctypes.data, len(a)))

    def close(self):
        if self._h:
            lib().kaiju_taxonomy_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceTaxonomy:
    """nodes.dmp in HBM for the LCA kernel (kaiju_gpu_taxonomy_upload)."""

    def __init__(self, tax: Taxonomy, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().kaiju_gpu_taxonomy_upload(tax._h, device, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().kaiju_gpu_taxonomy_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _names_mode(mode):
    """'name', 'path', 'ranks:<list>' (or a pair (mode, list)) -> (mode, list)"""
    if isinstance(mode, str):
        if mode.startswith("ranks:"):
            return NAMES_RANKS, mode[len("ranks:"):]
        return {"name": NAMES_NAME, "path": NAMES_PATH}[mode], None
    return mode


class TaxonNames:
    """nodes.dmp and names.dmp as kaiju-addTaxonNames reads them (kaiju_taxon_names_load; host only).  mode: "name", "path"
    (the tool's -p) or "ranks:<comma separated list>" (-r)."""

    def __init__(self, nodes_dmp: str, names_dmp: str, mode="name"):
        if not hasattr(lib(), "kaiju_taxon_names_load"):
            raise KaijuGpuError("this library was linked without taxon_names.cpp")
        m, ranks = _names_mode(mode)
        self.mode = m
        self._h = C.c_void_p()
        _check(lib().kaiju_taxon_names_load(nodes_dmp.encode(), names_dmp.encode(), m, ranks.encode() if ranks is not None else None, C.byref(self._h)))

    def annotation(self, taxon: int):
        """what the tool appends to a 'C' line of ``taxon`` (bytes), None: the line stays as it is"""
        n = lib().kaiju_taxon_names_annotation(self._h, taxon, None, 0)
        if n < 0:
            return None
        buf = np.zeros(n + 1, dtype=np.uint8)
        assert lib().kaiju_taxon_names_annotation(self._h, taxon, buf.ctypes.data, n) == n
        return buf[:n].tobytes()

    def count(self, named=False):
        return int(lib().kaiju_taxon_names_count(self._h, 1 if named else 0))

    def close(self):
        if self._h:
            lib().kaiju_taxon_names_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceTaxonNames:
    """TaxonNames in HBM, with the per-slot tables built there (kaiju_gpu_taxon_names_upload)."""
    TABLES = {"key": (0, "<u8"), "parent": (1, "<u4"), "name_pos": (2, "<u4"), "name_len": (3, "<u4"), "path_len": (4, "<u4"), "rank_len": (5, "<u4"),
              "rank_src": (6, "<u4"), "rank": (7, "u1")}

    def __init__(self, names: TaxonNames, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().kaiju_gpu_taxon_names_upload(names._h, device, C.byref(self._h)))

    @property
    def max_annotation(self):
        return int(lib().kaiju_gpu_taxon_names_max_annotation(self._h))

    def table(self, which: str, per_slot: int = 1):
        """a table as it lies on the device (for inspection); per_slot: words per slot (rank_src: the distinct ranks)"""
        k, dt = self.TABLES[which]
        cap = C.c_uint64()
        _check(lib().kaiju_gpu_taxon_names_read(self._h, k, None, 0, C.byref(cap)))
        out = np.zeros(cap.value * per_slot, dtype=dt)
        _check(lib().kaiju_gpu_taxon_names_read(self._h, k, out.ctypes.data, out.nbytes, None))
        return out

    def close(self):
        if self._h:
            lib().kaiju_gpu_taxon_names_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Annotator:
    """kaiju-addTaxonNames on the device of ``dnames`` (kaiju_gpu_annotator_create): text of output lines in, annotated text
    out.  It needs no index and no Classifier."""

    def __init__(self, dnames: DeviceTaxonNames):
        if not hasattr(lib(), "kaiju_gpu_annotator_create"):
            raise KaijuGpuError("this library was linked without annotate.hip")
        self._names = dnames                                  # (the tables must outlive the annotator)
        self._h = C.c_void_p()
        _check(lib().kaiju_gpu_annotator_create(dnames._h, C.byref(self._h)))

    def bound(self, text) -> int:
        return int(lib().kaiju_gpu_annotate_bound(len(text), bytes(text).count(b"\n") + 1, self._names._h))

    def annotate(self, text, drop_unclassified=False, out_cap=None, out=None):
        """Returns (bytes, info): the annotated lines and an ANNOTATE_INFO_DTYPE record.  out_cap: the capacity (default: one
        that cannot overflow); when the text overflows it, info["overflow"] is set and only whole lines in front of it are
        written.  out: a uint8 array of at least out_cap bytes to write into - the lines written change, nothing else does -;
        the first value returned is then None"""
        text = bytes(text)
        cap = int(out_cap) if out_cap is not None else self.bound(text)
        own = out is None
        if own:
            out = np.zeros(max(cap, 1), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.size >= cap
        info = np.zeros(1, dtype=ANNOTATE_INFO_DTYPE)
        _check(lib().kaiju_gpu_annotate_text(self._h, text, len(text), 1 if drop_unclassified else 0, out.ctypes.data, cap, info.ctypes.data))
        if not own:
            return None, info[0]
        written = min(int(info[0]["text_bytes"]), cap)
        if info[0]["overflow"]:                               # (the buffer was zeroed: behind the last line written lies no newline)
            written = bytes(out[:written]).rfind(b"\n") + 1
        return bytes(out[:written]), info[0]

    def annotate_device(self, d_text_ptr: int, nbytes: int, d_out_ptr: int, out_cap: int, d_info_ptr: int, drop_unclassified=False, stream: int = 0):
        """the same for device-resident buffers (raw pointers, both 16-byte aligned): kaiju_gpu_annotate_text_device,
        asynchronous on ``stream``"""
        _check(lib().kaiju_gpu_annotate_text_device(self._h, d_text_ptr or None, nbytes, 1 if drop_unclassified else 0, d_out_ptr or None, out_cap,
                                                    d_info_ptr or None, stream or None))

    def close(self):
        if self._h:
            lib().kaiju_gpu_annotator_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Merger:
    """kaiju-mergeOutputs on a device (kaiju_gpu_merger_create): two texts of output lines in, the merged text out.  ``dtax``: the
    tree of -t (None: the empty tree, which ``conflict="lca"`` refuses); ``conflict``: "1", "2", "lca" or "lowest" (-c);
    ``use_score``: -s.  It needs no index and no Classifier."""

    def __init__(self, dtax: DeviceTaxonomy | None = None, conflict="lca", use_score=False, device: int = 0):
        if not hasattr(lib(), "kaiju_gpu_merger_create"):
            raise KaijuGpuError("this library was linked without merge.hip")
        self._tax = dtax                                      # (the tree must outlive the merger)
        self._h = C.c_void_p()
        code = MERGE_MODES[conflict] if isinstance(conflict, str) else int(conflict)
        _check(lib().kaiju_gpu_merger_create(dtax._h if dtax is not None else None, device, code, 1 if use_score else 0, C.byref(self._h)))

    @staticmethod
    def bound(text1, text2) -> int:
        return int(lib().kaiju_gpu_merge_bound(len(text1), len(text2)))

    def merge(self, text1, text2, final=True, out_cap=None, out=None):
        """Returns (bytes, info): the merged lines and a MERGE_INFO_DTYPE record.  final=False: only lines a newline ends are
        paired and info["used1"] / info["used2"] say where the rest starts.  out_cap: the capacity (default: one that cannot
        overflow); when the text overflows it, info["overflow"] is set and only whole lines in front of it are written.  out: a
        uint8 array of at least out_cap bytes to write into - the lines written change, nothing else does -; the first value
        returned is then None"""
        text1, text2 = bytes(text1), bytes(text2)
        cap = int(out_cap) if out_cap is not None else self.bound(text1, text2)
        own = out is None
        if own:
            out = np.zeros(max(cap, 1), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.size >= cap
        info = np.zeros(1, dtype=MERGE_INFO_DTYPE)
        _check(lib().kaiju_gpu_merge_text(self._h, text1, len(text1), text2, len(text2), 1 if final else 0, out.ctypes.data, cap, info.ctypes.data))
        if not own:
            return None, info[0]
        written = min(int(info[0]["text_bytes"]), cap)
        if info[0]["overflow"]:                               # (the buffer was zeroed: behind the last line written lies no newline)
            written = bytes(out[:written]).rfind(b"\n") + 1
        return bytes(out[:written]), info[0]

    def merge_device(self, d_text1_ptr: int, nbytes1: int, d_text2_ptr: int, nbytes2: int, d_out_ptr: int, out_cap: int, d_info_ptr: int, final=True,
                     stream: int = 0):
        """the same for device-resident buffers (raw pointers, all 16-byte aligned): kaiju_gpu_merge_text_device, asynchronous
        on ``stream``"""
        _check(lib().kaiju_gpu_merge_text_device(self._h, d_text1_ptr or None, nbytes1, d_text2_ptr or None, nbytes2, 1 if final else 0, d_out_ptr or None,
                                                 out_cap, d_info_ptr or None, stream or None))

    def close(self):
        if self._h:
            lib().kaiju_gpu_merger_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tally:
    """kaiju2table's counts on the device of ``dnames`` (kaiju_gpu_tally_create): texts of output lines in, reads per taxon
    out.  It needs no index and no Classifier; ``dnames`` may be of any mode."""

    def __init__(self, dnames: DeviceTaxonNames):
        if not hasattr(lib(), "kaiju_gpu_tally_create"):
            raise KaijuGpuError("this library was linked without tally.hip")
        self._names = dnames                                  # (the tables must outlive the tally)
        self._h = C.c_void_p()
        _check(lib().kaiju_gpu_tally_create(dnames._h, C.byref(self._h)))

    def add(self, text, final=True):
        """counts the lines of ``text``; final=False: only lines a newline ends, info["used"] says where the rest starts.
        Returns the TALLY_INFO_DTYPE record of this call"""
        text = bytes(text)
        info = np.zeros(1, dtype=TALLY_INFO_DTYPE)
        _check(lib().kaiju_gpu_tally_add_text(self._h, text, len(text), 1 if final else 0, info.ctypes.data))
        return info[0]

    def add_device(self, d_text_ptr: int, nbytes: int, d_info_ptr: int, final=True, stream: int = 0):
        """the same for a device-resident text (raw pointer, 16-byte aligned): kaiju_gpu_tally_add_text_device, asynchronous
        on ``stream``"""
        _check(lib().kaiju_gpu_tally_add_text_device(self._h, d_text_ptr or None, nbytes, 1 if final else 0, d_info_ptr or None, stream or None))

    def reset(self):
        _check(lib().kaiju_gpu_tally_reset(self._h))

    def result(self, cap=None):
        """(entries, totals) since the last reset: a TALLY_ENTRY_DTYPE array sorted by taxon and a TALLY_INFO_DTYPE record.
        cap: room for that many entries (default: as many as there are)"""
        n = C.c_uint64()
        totals = np.zeros(1, dtype=TALLY_INFO_DTYPE)
        if cap is None:
            rc = lib().kaiju_gpu_tally_result(self._h, None, 0, C.byref(n), totals.ctypes.data)
            if rc == 0:
                return np.zeros(0, dtype=TALLY_ENTRY_DTYPE), totals[0]
            cap = n.value
            if not cap:
                _check(rc)
        entries = np.zeros(max(int(cap), 1), dtype=TALLY_ENTRY_DTYPE)
        _check(lib().kaiju_gpu_tally_result(self._h, entries.ctypes.data, int(cap), C.byref(n), totals.ctypes.data))
        entries = entries[:n.value]
        return entries[np.argsort(entries["taxon"], kind="stable")], totals[0]

    def pass_ms(self):
        """milliseconds of the last add call's passes (lines, count, finish); needs KAIJU_GPU_TALLY_TIMES=1 at creation"""
        ms = np.zeros(TALLY_PASSES, dtype=np.float32)
        _check(lib().kaiju_gpu_tally_pass_ms(self._h, ms.ctypes.data, TALLY_PASSES))
        return ms

    def close(self):
        if self._h:
            lib().kaiju_gpu_tally_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Krona:
    """kaiju2krona's text from the counts of tallies on the device of ``dnames`` (kaiju_gpu_krona_create): one line per taxon
    with reads, "<reads>\t<name>\t<name>...\n" with the lineage root first.  ranks: the text of the tool's -l (None: no
    list).  ``dnames`` may be of any mode."""

    def __init__(self, dnames: DeviceTaxonNames, ranks=None):
        if not hasattr(lib(), "kaiju_gpu_krona_create"):
            raise KaijuGpuError("this library was linked without krona.hip")
        self._names = dnames                                  # (the tables must outlive the object)
        self._h = C.c_void_p()
        if ranks is not None and not isinstance(ranks, bytes):
            ranks = ranks.encode()
        _check(lib().kaiju_gpu_krona_create(dnames._h, ranks, C.byref(self._h)))

    @staticmethod
    def _handles(tallies):
        tallies = [tallies] if isinstance(tallies, Tally) else list(tallies)
        return (C.c_void_p * max(len(tallies), 1))(*[t._h for t in tallies]), len(tallies)

    def text(self, tallies, unclassified=False, out_cap=None, out=None):
        """Returns (bytes, info): the lines of the counts of ``tallies`` (a Tally or up to KRONA_MAX_TALLIES of them, added per
        taxon) and a KRONA_INFO_DTYPE record.  unclassified: the tool's -u.  out_cap: the capacity (default: the size of the
        text, found by a call with none); when the text overflows it, info["overflow"] is set and only whole lines in front of
        it are written.  out: a uint8 array of at least out_cap bytes to write into; the first value returned is then None"""
        h, n = self._handles(tallies)
        info = np.zeros(1, dtype=KRONA_INFO_DTYPE)
        if out_cap is None:
            _check(lib().kaiju_gpu_krona_text(self._h, h, n, 1 if unclassified else 0, None, 0, info.ctypes.data))
            out_cap = int(info[0]["text_bytes"])
        cap = int(out_cap)
        own = out is None
        if own:
            out = np.zeros(max(cap, 1), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.size >= cap
        _check(lib().kaiju_gpu_krona_text(self._h, h, n, 1 if unclassified else 0, out.ctypes.data if cap else None, cap, info.ctypes.data))
        if not own:
            return None, info[0]
        return bytes(out[:int(info[0]["written_bytes"])]), info[0]

    def text_device(self, tallies, d_out_ptr: int, out_cap: int, d_info_ptr: int, unclassified=False, stream: int = 0):
        """the same into device memory (raw pointers, d_out 16-byte aligned): kaiju_gpu_krona_text_device, asynchronous on
        ``stream`` behind the calls of the tallies"""
        h, n = self._handles(tallies)
        _check(lib().kaiju_gpu_krona_text_device(self._h, h, n, 1 if unclassified else 0, d_out_ptr or None, out_cap, d_info_ptr or None, stream or None))

    def pass_ms(self):
        """milliseconds of the last call's passes (select, compact, len and offsets, write, finish); needs
        KAIJU_GPU_KRONA_TIMES=1 at creation"""
        ms = np.zeros(KRONA_PASSES, dtype=np.float32)
        _check(lib().kaiju_gpu_krona_pass_ms(self._h, ms.ctypes.data, KRONA_PASSES))
        return ms

    def close(self):
        if self._h:
            lib().kaiju_gpu_krona_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CONVERT_RULES = {"nr": 0, "refseq": 1}                        # KAIJU_GPU_CONVERT_RULES_NR, _REFSEQ


def _rules(rules):
    if rules not in CONVERT_RULES:
        raise KaijuGpuError("rules is 'nr' or 'refseq', not %r" % (rules,))
    if rules != "nr" and not hasattr(lib(), "kaiju_gpu_accmap_create_rules"):
        raise KaijuGpuError("this library has no rule sets (kaiju_gpu_accmap_create_rules)")
    return CONVERT_RULES[rules]


class AccMap:
    """The accession -> taxon map of kaiju-convertNR (rules="nr": kaiju_gpu_accmap_create) or of kaiju-convertRefSeq
    (rules="refseq": kaiju_gpu_accmap_create_rules) on the device.  dtax: the tree whose nodes decide which lines insert (None: a
    map for add_keys only, the excluded accessions); merged: (old id, new id) pairs of merged.dmp in file order."""

    def __init__(self, dtax=None, merged=(), device=0, initial_slots=0, key_col=1, taxon_col=2, rules="nr"):
        if not hasattr(lib(), "kaiju_gpu_accmap_create"):
            raise KaijuGpuError("this library was linked without accmap.hip")
        self._tax = dtax                                      # (the tree must outlive the map)
        self._h = C.c_void_p()
        self.rules = rules
        pairs = np.array([x for p in merged for x in p], dtype=np.uint64)
        tax, p = dtax._h if dtax is not None else None, pairs.ctypes.data if len(pairs) else None
        if _rules(rules):
            _check(lib().kaiju_gpu_accmap_create_rules(tax, device, p, len(pairs) // 2, CONVERT_RULES[rules], initial_slots, C.byref(self._h)))
        else:
            _check(lib().kaiju_gpu_accmap_create(tax, device, p, len(pairs) // 2, key_col, taxon_col, initial_slots, C.byref(self._h)))

    def add_text(self, text: bytes, first_block=True):
        """a block of the map file, cut behind a line end; first_block: its first line is the file's header line"""
        _check(lib().kaiju_gpu_accmap_add_text(self._h, text, len(text), 1 if first_block else 0))
        return self

    def add_text_device(self, d_text_ptr: int, nbytes: int, first_block=True):
        _check(lib().kaiju_gpu_accmap_add_text_device(self._h, d_text_ptr or None, nbytes, 1 if first_block else 0))

    def add_keys(self, text: bytes, value=1):
        """every non-empty line is a key with the value ``value``"""
        _check(lib().kaiju_gpu_accmap_add_keys(self._h, text, len(text), value))
        return self

    def lookup(self, keys):
        """the taxa of ``keys`` (a list of bytes without '\n'; ACCMAP_MISS: not in the map)"""
        keys = list(keys)
        if not keys:
            return []
        text = b"\n".join(keys) + b"\n"
        out = np.zeros(len(keys) + 1, dtype=np.uint64)
        n = C.c_uint64()
        _check(lib().kaiju_gpu_accmap_lookup(self._h, text, len(text), out.ctypes.data, len(out), C.byref(n)))
        assert n.value == len(keys), (n.value, len(keys))
        return [int(x) for x in out[:len(keys)]]

    def info(self):
        out = np.zeros(1, dtype=ACCMAP_STATS_DTYPE)
        _check(lib().kaiju_gpu_accmap_info(self._h, out.ctypes.data))
        return out[0]

    def pass_ms(self):
        """milliseconds of the last add call's passes (lines, parse, grow, insert, resolve); needs KAIJU_GPU_CONVERT_TIMES=1 at creation"""
        ms = np.zeros(ACCMAP_PASSES, dtype=np.float32)
        _check(lib().kaiju_gpu_accmap_pass_ms(self._h, ms.ctypes.data, ACCMAP_PASSES))
        return ms

    def close(self):
        if self._h:
            lib().kaiju_gpu_accmap_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Converter:
    """kaiju-convertNR on blocks of nr-style text (kaiju_gpu_converter_create): per kept record '>' [accession '_'] taxon '\n'
    letters '\n'.  include: the ids of -l that are nodes (None: 2, 2157, 10239); excluded: an AccMap built with add_keys.
    rules="refseq": kaiju-convertRefSeq (kaiju_gpu_converter_create_rules) - one accession per header, no LCA, no excluded
    map; amap must have been made with the same rules."""

    def __init__(self, dtax, amap: AccMap, excluded: AccMap = None, include=None, add_acc=False, rules="nr"):
        if not hasattr(lib(), "kaiju_gpu_converter_create"):
            raise KaijuGpuError("this library was linked without convert.hip")
        if _rules(rules) and excluded is not None:
            raise KaijuGpuError("the rules of kaiju-convertRefSeq have no excluded accessions")
        self._keep = (dtax, amap, excluded)                   # (they must outlive the converter)
        self._h = C.c_void_p()
        ids = np.array(list(include) if include is not None else [], dtype=np.uint64)
        if include is not None and not len(ids):
            ids = np.array([2 ** 64 - 1], dtype=np.uint64)   # an empty list keeps nothing: an id that is never a node
        p, n = (ids.ctypes.data, len(ids)) if include is not None else (None, 0)
        if _rules(rules):
            _check(lib().kaiju_gpu_converter_create_rules(dtax._h, p, n, amap._h, CONVERT_RULES[rules], 1 if add_acc else 0, C.byref(self._h)))
        else:
            _check(lib().kaiju_gpu_converter_create(dtax._h, p, n, amap._h, excluded._h if excluded is not None else None, 1 if add_acc else 0, C.byref(self._h)))

    def convert(self, text: bytes, out_cap=None):
        """Returns (bytes, info): the records of a block that starts at a header line (or is the start of the file) and a
        CONVERT_INFO_DTYPE record.  out_cap: the capacity (default: the size of the text, found by a call with none); when the
        text overflows it only whole records in front of it are written"""
        info = np.zeros(1, dtype=CONVERT_INFO_DTYPE)
        if out_cap is None:
            _check(lib().kaiju_gpu_convert_text(self._h, text, len(text), None, 0, info.ctypes.data))
            out_cap = int(info[0]["text_bytes"])
        cap = int(out_cap)
        out = np.full(cap + 32, 0x77, dtype=np.uint8)
        _check(lib().kaiju_gpu_convert_text(self._h, text, len(text), out.ctypes.data if cap else None, cap, info.ctypes.data))
        assert (out[cap:] == 0x77).all()
        return bytes(out[:int(info[0]["written_bytes"])]), info[0]

    def convert_device(self, d_text_ptr: int, nbytes: int, d_out_ptr: int, out_cap: int, d_info_ptr: int, stream: int = 0):
        """the same from and into device memory (raw pointers, 16-byte aligned): asynchronous on ``stream``"""
        _check(lib().kaiju_gpu_convert_text_device(self._h, d_text_ptr or None, nbytes, d_out_ptr or None, out_cap, d_info_ptr or None, stream or None))

    def convert_file(self, text: bytes, block_bytes=1 << 24) -> bytes:
        """a whole nr text, cut at "\n>" into blocks of about block_bytes: the tool's file, the '\n' of an empty one included"""
        out, at = [], 0
        while at < len(text):
            end = len(text)
            if end - at > block_bytes:
                end = text.rfind(b"\n>", at, at + block_bytes) + 1
                if end <= at:
                    raise KaijuGpuError("a record of more than %d bytes" % block_bytes)
            out.append(self.convert(text[at:end])[0])
            at = end
        got = b"".join(out)
        return got if got else b"\n"

    def pass_ms(self):
        """milliseconds of the last call's passes (lines, kinds, entries, decide, lengths and offsets, write, finish); needs
        KAIJU_GPU_CONVERT_TIMES=1 at creation"""
        ms = np.zeros(CONVERT_PASSES, dtype=np.float32)
        _check(lib().kaiju_gpu_convert_pass_ms(self._h, ms.ctypes.data, CONVERT_PASSES))
        return ms

    def close(self):
        if self._h:
            lib().kaiju_gpu_converter_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GbkNoTaxon(KaijuGpuError):
    """a /translation in front of which the file has no /db_xref="taxon:..": kaiju-gbk2faa.pl ends there with an empty file"""

    def __init__(self, line):
        super().__init__("No taxon id found in gbk file (line %d)" % line)
        self.line = line


class Gbk:
    """kaiju-gbk2faa on blocks of GenBank flat-file text (kaiju_gpu_gbk_create): per /translation a header '>' protein id '_' taxon
    and a line of filtered letters per line of the translation.  The object carries the taxon and the protein id seen last and
    whether a translation is open from block to block; reset() starts a new file."""

    def __init__(self, device=0):
        if not hasattr(lib(), "kaiju_gpu_gbk_create"):
            raise KaijuGpuError("this library was linked without gbk.hip")
        self._h = C.c_void_p()
        _check(lib().kaiju_gpu_gbk_create(device, C.byref(self._h)))

    def reset(self):
        _check(lib().kaiju_gpu_gbk_reset(self._h))
        return self

    def convert(self, text: bytes, out_cap=None, fill=0x77):
        """Returns (bytes, info): the output of a block that ends behind a line end (or is the end of the file) and a
        GBK_INFO_DTYPE record.  out_cap: the capacity; when the text overflows only whole lines in front of it are written and
        the carried state stays where it was.  Default: as much as the text has bytes, and the call is repeated with the
        size the first one reported if that was too little (a header may be longer than its line)"""
        info = np.zeros(1, dtype=GBK_INFO_DTYPE)
        cap = len(text) if out_cap is None else int(out_cap)
        while True:
            out = np.full(cap + 32, fill, dtype=np.uint8)
            _check(lib().kaiju_gpu_gbk_text(self._h, text, len(text), out.ctypes.data if cap else None, cap, info.ctypes.data))
            assert (out[cap:] == fill).all()
            if out_cap is not None or not info[0]["overflow"]:
                return bytes(out[:int(info[0]["written_bytes"])]), info[0]
            cap = int(info[0]["text_bytes"])

    def convert_device(self, d_text_ptr: int, nbytes: int, d_out_ptr: int, out_cap: int, d_info_ptr: int, stream: int = 0):
        """the same from and into device memory (raw pointers, 16-byte aligned): asynchronous on ``stream``"""
        _check(lib().kaiju_gpu_gbk_text_device(self._h, d_text_ptr or None, nbytes, d_out_ptr or None, out_cap, d_info_ptr or None, stream or None))

    def convert_file(self, text: bytes, block_bytes=1 << 24) -> bytes:
        """a whole flat file, cut behind line ends into blocks of at most block_bytes: the script's file.  GbkNoTaxon (with the
        line of the file) where the script dies"""
        self.reset()
        out, at, lines = [], 0, 0
        while at < len(text):
            end = len(text)
            if end - at > block_bytes:
                end = text.rfind(b"\n", at, at + block_bytes) + 1
                if end <= at:
                    raise KaijuGpuError("a line of more than %d bytes" % block_bytes)
            got, info = self.convert(text[at:end])
            if info["no_taxon_line"]:
                raise GbkNoTaxon(lines + int(info["no_taxon_line"]))
            out.append(got)
            lines += int(info["n_lines"])
            at = end
        return b"".join(out)

    def pass_ms(self):
        """milliseconds of the last call's passes (lines, kinds, scans, lengths and offsets, write, finish); needs
        KAIJU_GPU_CONVERT_TIMES=1 at creation"""
        ms = np.zeros(GBK_PASSES, dtype=np.float32)
        _check(lib().kaiju_gpu_gbk_pass_ms(self._h, ms.ctypes.data, GBK_PASSES))
        return ms

    def close(self):
        if self._h:
            lib().kaiju_gpu_gbk_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def table_text(names: TaxonNames, entries, totals, label, rank, ranks=None, min_percent=0.0, min_count=0, expand_viruses=False,
               filter_unclassified=False, full_path=False) -> bytes:
    """the rows kaiju2table prints for one input file (kaiju_table_rows; host only): ``entries`` and ``totals`` as
    Tally.result gives them, ``label`` for the file column; the other arguments are the tool's -r, -l, -m, -c, -e, -u, -p.
    Options the tool refuses raise KaijuGpuError.  No header row."""
    entries = np.ascontiguousarray(entries, dtype=TALLY_ENTRY_DTYPE)
    totals = np.array([totals], dtype=TALLY_INFO_DTYPE)
    flags = (TABLE_EXPAND_VIRUSES if expand_viruses else 0) | (TABLE_FILTER_UNCLASSIFIED if filter_unclassified else 0) | (TABLE_FULL_PATH if full_path else 0)
    opt = TableOptions(rank.encode(), ranks.encode() if ranks else None, float(min_percent), int(min_count), flags, 0)
    label = label if isinstance(label, bytes) else label.encode()
    n = C.c_uint64()
    args = (names._h, entries.ctypes.data if entries.size else None, entries.size, totals.ctypes.data, C.byref(opt), label)
    _check(lib().kaiju_table_rows(*args, None, 0, C.byref(n)))
    buf = np.zeros(n.value + 1, dtype=np.uint8)
    _check(lib().kaiju_table_rows(*args, buf.ctypes.data, n.value, C.byref(n)))
    return buf[:n.value].tobytes()


class Classifier:
    """One classification stream on one GPU (the ConsumerThread of the reference)."""

    def __init__(self, index: Index, params: Params):
        self.index = index
        self.params = params
        self._h = C.c_void_p()
        _check(lib().kaiju_gpu_create(C.byref(self._h), index._h, C.byref(params)))

    def classify(self, seqs: np.ndarray, off: np.ndarray, paired=False) -> np.ndarray:
        """Host buffers in, hit records out (blocking)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = (len(off) - 1) // 2
        hits = np.zeros(n, dtype=HIT_DTYPE)
        _check(lib().kaiju_gpu_classify_batch(self._h, seqs.ctypes.data, off.ctypes.data, n,
                                              1 if paired else 0, hits.ctypes.data))
        return hits

    def locate_intervals(self, lo, length, first) -> np.ndarray:
        """kaiju_gpu_locate_intervals (diagnostics): record r is given the suffix-array intervals first[r] .. first[r+1]-1 (rows
        lo[i] .. lo[i] + length[i] - 1, at most 16 a record) as pending matches; the locate this context's classification would
        run turns them into ids.  Returns the hit records (n_ids, taxid, KAIJU_HIT_ID_CAP in flags)."""
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        first = np.ascontiguousarray(first, dtype=np.uint32)
        n = len(first) - 1
        assert n >= 0 and len(lo) == len(length) and (n == 0 or int(first[-1]) <= len(lo))
        L = lib()
        L.kaiju_gpu_locate_intervals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        hits = np.zeros(n, dtype=HIT_DTYPE)
        _check(L.kaiju_gpu_locate_intervals(self._h, lo.ctypes.data, length.ctypes.data, first.ctypes.data, n, hits.ctypes.data))
        return hits

    def set_max_read_length(self, n: int):
        """upper bound of the read lengths given to classify_device (sizes scratch, picks the staged kernel)"""
        _check(lib().kaiju_gpu_set_max_read_length(self._h, int(n)))

    def classify_device(self, d_seqs_ptr: int, seq_bytes: int, d_off_ptr: int, n: int, d_out_ptr: int,
                        paired=False, stream: int = 0):
        """Device-resident buffers (raw pointers, e.g. torch ``data_ptr()``); asynchronous on ``stream``."""
        _check(lib().kaiju_gpu_classify_batch_device(self._h, d_seqs_ptr, seq_bytes, d_off_ptr, n,
                                                     1 if paired else 0, d_out_ptr, stream))

    def stream_handle(self) -> int:
        """the context's own HIP stream (hipStream_t as an integer): wrap it with torch.cuda.ExternalStream to queue
        torch work (a collective, a copy) behind a batch that was launched with stream=0"""
        h = C.c_void_p()
        lib().kaiju_gpu_get_stream.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        _check(lib().kaiju_gpu_get_stream(self._h, C.byref(h)))
        return int(h.value or 0)

    def synchronize(self):
        _check(lib().kaiju_gpu_synchronize(self._h))

    def stats(self) -> Stats:
        s = Stats()
        _check(lib().kaiju_gpu_get_stats(self._h, C.byref(s)))
        return s

    def finalize(self, tax: Taxonomy, hits: np.ndarray, off: np.ndarray, paired=False) -> np.ndarray:
        """E-value gate + LCA + C/U decision on the host (ConsumerThread.cpp:500-513,538,625,724-739)."""
        hits = np.ascontiguousarray(hits)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(hits)
        res = np.zeros(n, dtype=RESULT_DTYPE)
        _check(lib().kaiju_finalize_hits(tax._h, C.byref(self.params), self.index.db_length, hits.ctypes.data,
                                         off.ctypes.data, n, 1 if paired else 0, res.ctypes.data))
        return res

    def lca_device(self, dtax: "DeviceTaxonomy", d_hits_ptr: int, n: int, d_out_ptr: int, stream: int = 0):
        """hit records -> 16-byte compact records (LCA on the device); asynchronous on ``stream``."""
        _check(lib().kaiju_gpu_lca_batch_device(self._h, dtax._h, d_hits_ptr, n, d_out_ptr, stream))

    def classify_device_compact(self, dtax: "DeviceTaxonomy", d_seqs_ptr: int, seq_bytes: int, d_off_ptr: int, n: int,
                                d_hits_ptr: int, d_out_ptr: int, paired=False, stream: int = 0):
        """classify_device + lca_device in one call (kaiju_gpu_classify_batch_device_compact): the search's own post-search
        pass writes the 16-byte records where the configuration allows"""
        _check(lib().kaiju_gpu_classify_batch_device_compact(self._h, dtax._h, d_seqs_ptr, seq_bytes, d_off_ptr, n,
                                                             1 if paired else 0, d_hits_ptr, d_out_ptr, stream))

    def classify_verbose_raw(self, seqs: np.ndarray, off: np.ndarray, paired=False):
        """kaiju -v, the library call alone (kaiju_gpu_classify_batch_verbose): (hit records, kaiju_gpu_verbose records, the rows
        of column-7 text, their stride); the output arrays are kept between calls of the same size"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = (len(off) - 1) // 2
        maxpair = int((off[2::2] - off[0:-1:2]).max()) if n else 0
        lib().kaiju_gpu_verbose_text_stride.restype = C.c_uint32
        lib().kaiju_gpu_verbose_text_stride.argtypes = [C.c_uint32, C.c_int]
        stride = int(lib().kaiju_gpu_verbose_text_stride(maxpair, int(self.params.input_is_protein)))
        kept = getattr(self, "_vb_out", None)
        if kept is None or kept[0] != (n, stride):
            kept = ((n, stride), np.zeros(n, dtype=HIT_DTYPE), np.zeros(n, dtype=VERBOSE_DTYPE), np.zeros(n * stride, dtype=np.uint8))
            self._vb_out = kept
        _, hits, v, text = kept
        _check(lib().kaiju_gpu_classify_batch_verbose(self._h, seqs.ctypes.data, off.ctypes.data, n, 1 if paired else 0,
                                                      hits.ctypes.data, v.ctypes.data, text.ctypes.data, stride))
        return hits, v, text, stride

    def classify_verbose_packed(self, seqs: np.ndarray, off: np.ndarray, paired=False):
        """kaiju -v with column 7 of the batch as ONE string (kaiju_gpu_classify_batch_verbose_packed, what the command line
        programs call): (hit records, kaiju_gpu_verbose records, per read the position of its text, a COPY of the string -
        the library's own is valid until the context's next verbose call)"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = (len(off) - 1) // 2
        hits = np.zeros(n, dtype=HIT_DTYPE)
        v = np.zeros(n, dtype=VERBOSE_DTYPE)
        pos = np.zeros(n, dtype=np.uint64)
        text = C.c_void_p()
        nbytes = C.c_uint64()
        f = lib().kaiju_gpu_classify_batch_verbose_packed
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        f.restype = C.c_int
        _check(f(self._h, seqs.ctypes.data, off.ctypes.data, n, 1 if paired else 0, hits.ctypes.data, v.ctypes.data, pos.ctypes.data,
                 C.byref(text), C.byref(nbytes)))
        return hits, v, pos, (C.string_at(text.value, nbytes.value) if nbytes.value else b"")

    def verbose_columns(self, v, text, stride):
        """(per read the sorted accession list of column 6, the text of column 7) from what classify_verbose_raw returned"""
        n = len(v)
        accs, peps = [], []
        for r in range(n):
            names = set()
            for q in range(int(v[r]["n_acc"])):
                nm = lib().kaiju_gpu_index_seq_name(self.index._h, int(v[r]["acc_iseq"][q]))
                if nm and b"_" in nm:
                    names.add(nm[: nm.rindex(b"_")].decode())
            accs.append(sorted(names))
            peps.append(bytes(text[r * stride: r * stride + int(v[r]["text_len"])]).decode())
        return accs, peps

    def classify_verbose(self, seqs: np.ndarray, off: np.ndarray, paired=False):
        """kaiju -v: (hit records, per read the sorted accession list of column 6, the text of column 7)"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = (len(off) - 1) // 2
        hits = np.zeros(n, dtype=HIT_DTYPE)
        v = np.zeros(n, dtype=VERBOSE_DTYPE)
        maxpair = int((off[2::2] - off[0:-1:2]).max()) if n else 0
        lib().kaiju_gpu_verbose_text_stride.restype = C.c_uint32
        lib().kaiju_gpu_verbose_text_stride.argtypes = [C.c_uint32, C.c_int]
        stride = int(lib().kaiju_gpu_verbose_text_stride(maxpair, int(self.params.input_is_protein)))
        text = np.zeros(n * stride, dtype=np.uint8)
        _check(lib().kaiju_gpu_classify_batch_verbose(self._h, seqs.ctypes.data, off.ctypes.data, n, 1 if paired else 0,
                                                      hits.ctypes.data, v.ctypes.data, text.ctypes.data, stride))
        accs, peps = [], []
        for r in range(n):
            names = set()
            for q in range(int(v[r]["n_acc"])):
                nm = lib().kaiju_gpu_index_seq_name(self.index._h, int(v[r]["acc_iseq"][q]))
                if nm and b"_" in nm:
                    names.add(nm[: nm.rindex(b"_")].decode())
            accs.append(sorted(names))
            peps.append(bytes(text[r * stride: r * stride + int(v[r]["text_len"])]).decode())
        return hits, accs, peps

    def classify_compact(self, dtax: "DeviceTaxonomy", seqs: np.ndarray, off: np.ndarray, paired=False, out=None) -> np.ndarray:
        """Host buffers in, 16-byte records (LCA on the device) out; blocking (kaiju_gpu_classify_batch_compact).
        Arrays are used as they are (no copies): pass page-locked memory for full PCIe rates."""
        n = (len(off) - 1) // 2
        if out is None:
            out = np.zeros(n, dtype=COMPACT_DTYPE)
        assert seqs.dtype == np.uint8 and off.dtype == np.uint64 and seqs.flags.c_contiguous and off.flags.c_contiguous
        _check(lib().kaiju_gpu_classify_batch_compact(self._h, dtax._h, seqs.ctypes.data, off.ctypes.data, n,
                                                      1 if paired else 0, out.ctypes.data))
        return out

    def classify_text_compact(self, dtax: "DeviceTaxonomy", text1, text2=None, fastq=True, keep_names=False, rec_cap=None):
        """FASTQ / FASTA text in, 16-byte records out (kaiju_gpu_classify_text_compact): the records are extracted on the
        device.  Returns a dict: compact, off, names (n x 2 uint32: position and length in text1), info."""
        t1, t2, cap = _text_args(text1, text2, rec_cap)
        out = np.zeros(cap, dtype=COMPACT_DTYPE)
        off = np.zeros(2 * cap + 1, dtype=np.uint64)
        names = np.zeros(cap, dtype=NAME_SPAN_DTYPE)
        info = np.zeros(1, dtype=PARSE_INFO_DTYPE)
        _check(lib().kaiju_gpu_classify_text_compact(self._h, dtax._h, t1.ctypes.data, len(t1) - 1, t2.ctypes.data if t2 is not None else None,
                                                     len(t2) - 1 if t2 is not None else 0, 1 if fastq else 0, 1 if keep_names else 0, cap,
                                                     out.ctypes.data, off.ctypes.data, names.ctypes.data, info.ctypes.data))
        n = _reads_emitted(info[0], t2 is not None, cap)
        return {"compact": out[:n], "off": off[: 2 * n + 1], "names": names[:n].view("<u4").reshape(n, 2), "info": info[0]}

    def parse_block_device(self, d_text1_ptr: int, bytes1: int, d_text2_ptr: int, bytes2: int, rec_cap: int, d_seqs_ptr: int,
                           d_off_ptr: int, d_names_ptr: int, d_info_ptr: int, fastq=True, keep_names=False, stream: int = 0):
        """Device-resident text (raw pointers, 16-byte aligned; d_text2_ptr = 0: unpaired) to device-resident seqs / off /
        names / info (kaiju_gpu_parse_block_device); asynchronous on ``stream``."""
        _check(lib().kaiju_gpu_parse_block_device(self._h, d_text1_ptr or None, bytes1, d_text2_ptr or None, bytes2, 1 if fastq else 0,
                                                  1 if keep_names else 0, rec_cap, d_seqs_ptr or None, d_off_ptr or None,
                                                  d_names_ptr or None, d_info_ptr or None, stream or None))

    def parse_block_tensors(self, text1, text2=None, fastq=True, keep_names=False, rec_cap=None, stream: int = 0):
        """parse_block_device for torch uint8 tensors on the context's GPU; returns a dict of tensors (seqs uint8, off int64,
        names int32 n_cap x 2, info: 8 x int32 in the layout of kaiju_gpu_parse_info), nothing is synchronised"""
        import torch
        assert text1.dtype == torch.uint8 and text1.is_contiguous() and (text2 is None or (text2.dtype == torch.uint8 and text2.is_contiguous()))
        b1, b2 = text1.numel(), text2.numel() if text2 is not None else 0
        cap = int(rec_cap) if rec_cap is not None else b1 + 1
        dev = text1.device
        seqs = torch.empty(b1 + b2 + 64, dtype=torch.uint8, device=dev)
        off = torch.empty(2 * cap + 1, dtype=torch.int64, device=dev)
        names = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=dev)
        info = torch.empty(8, dtype=torch.int32, device=dev)
        self.parse_block_device(text1.data_ptr(), b1, text2.data_ptr() if text2 is not None else 0, b2, cap, seqs.data_ptr(), off.data_ptr(),
                                names.data_ptr(), info.data_ptr(), fastq=fastq, keep_names=keep_names, stream=stream)
        return {"seqs": seqs, "off": off, "names": names, "info": info}

    def format_compact(self, recs: np.ndarray, off: np.ndarray, text1, names: np.ndarray, paired=False, out_cap=None, out=None):
        """16-byte records, off[], the text the names lie in and the name spans (NAME_SPAN_DTYPE) to the lines of the output
        file (kaiju_gpu_format_compact): host buffers, blocking.  Returns (out, info): out is a uint8 array of out_cap bytes
        (default: kaiju_gpu_format_bound) of which the lines written have changed, info a FORMAT_INFO_DTYPE record."""
        recs = np.ascontiguousarray(recs, dtype=COMPACT_DTYPE)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        names = np.ascontiguousarray(names, dtype=NAME_SPAN_DTYPE)
        t1 = np.frombuffer(bytes(text1) + b"\0", dtype=np.uint8) if not isinstance(text1, np.ndarray) else np.concatenate([text1, np.zeros(1, dtype=np.uint8)])
        n = len(recs)
        assert len(off) == 2 * n + 1 and len(names) == n
        cap = int(out_cap) if out_cap is not None else format_bound(len(t1) - 1, n)
        if out is None:
            out = np.zeros(cap + 1, dtype=np.uint8)
        assert out.dtype == np.uint8 and len(out) >= cap
        info = np.zeros(1, dtype=FORMAT_INFO_DTYPE)
        _check(lib().kaiju_gpu_format_compact(self._h, recs.ctypes.data, off.ctypes.data, n, 1 if paired else 0, t1.ctypes.data, len(t1) - 1,
                                              names.ctypes.data, out.ctypes.data, cap, info.ctypes.data))
        return out, info[0]

    def format_compact_device(self, d_recs_ptr: int, d_off_ptr: int, n: int, d_text1_ptr: int, bytes1: int, d_names_ptr: int, d_out_ptr: int,
                              out_cap: int, d_info_ptr: int, paired=False, stream: int = 0):
        """the same for device-resident buffers (raw pointers; d_out 16-byte aligned): kaiju_gpu_format_compact_device,
        asynchronous on ``stream``"""
        _check(lib().kaiju_gpu_format_compact_device(self._h, d_recs_ptr or None, d_off_ptr or None, n, 1 if paired else 0, d_text1_ptr or None,
                                                     bytes1, d_names_ptr or None, d_out_ptr or None, out_cap, d_info_ptr or None, stream or None))

    def classify_text_to_text(self, dtax: "DeviceTaxonomy", text1, text2=None, fastq=True, keep_names=False, rec_cap=None, out_cap=None):
        """FASTQ / FASTA text in, the lines of the output file out (kaiju_gpu_classify_text_to_text).  Returns a dict: text
        (bytes), info (PARSE_INFO_DTYPE record), format_info (FORMAT_INFO_DTYPE record)."""
        t1, t2, cap = _text_args(text1, text2, rec_cap)
        ocap = int(out_cap) if out_cap is not None else format_bound(len(t1) - 1, cap)
        out = np.zeros(ocap + 1, dtype=np.uint8)
        info = np.zeros(1, dtype=PARSE_INFO_DTYPE)
        finfo = np.zeros(1, dtype=FORMAT_INFO_DTYPE)
        _check(lib().kaiju_gpu_classify_text_to_text(self._h, dtax._h, t1.ctypes.data, len(t1) - 1, t2.ctypes.data if t2 is not None else None,
                                                     len(t2) - 1 if t2 is not None else 0, 1 if fastq else 0, 1 if keep_names else 0, cap,
                                                     out.ctypes.data, ocap, info.ctypes.data, finfo.ctypes.data))
        return {"text": out[: int(finfo[0]["text_bytes"])].tobytes(), "info": info[0], "format_info": finfo[0]}

    def format_names(self, recs: np.ndarray, off: np.ndarray, text1, names: np.ndarray, dnames: "DeviceTaxonNames", paired=False, drop_unclassified=False,
                     out_cap=None, out=None):
        """format_compact with the column of kaiju-addTaxonNames (kaiju_gpu_format_names).  Returns (out, info): info is a
        FORMAT_NAMES_INFO_DTYPE record."""
        recs = np.ascontiguousarray(recs, dtype=COMPACT_DTYPE)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        names = np.ascontiguousarray(names, dtype=NAME_SPAN_DTYPE)
        t1 = np.frombuffer(bytes(text1) + b"\0", dtype=np.uint8) if not isinstance(text1, np.ndarray) else np.concatenate([text1, np.zeros(1, dtype=np.uint8)])
        n = len(recs)
        assert len(off) == 2 * n + 1 and len(names) == n
        cap = int(out_cap) if out_cap is not None else int(lib().kaiju_gpu_format_names_bound(len(t1) - 1, n, dnames._h))
        if out is None:
            out = np.zeros(cap + 1, dtype=np.uint8)
        assert out.dtype == np.uint8 and len(out) >= cap
        info = np.zeros(1, dtype=FORMAT_NAMES_INFO_DTYPE)
        _check(lib().kaiju_gpu_format_names(self._h, recs.ctypes.data, off.ctypes.data, n, 1 if paired else 0, t1.ctypes.data, len(t1) - 1,
                                            names.ctypes.data, dnames._h, 1 if drop_unclassified else 0, out.ctypes.data, cap, info.ctypes.data))
        return out, info[0]

    def format_names_device(self, d_recs_ptr: int, d_off_ptr: int, n: int, d_text1_ptr: int, bytes1: int, d_names_ptr: int, dnames: "DeviceTaxonNames",
                            d_out_ptr: int, out_cap: int, d_info_ptr: int, paired=False, drop_unclassified=False, stream: int = 0):
        """the same for device-resident buffers (raw pointers; d_out 16-byte aligned): kaiju_gpu_format_names_device,
        asynchronous on ``stream``"""
        _check(lib().kaiju_gpu_format_names_device(self._h, d_recs_ptr or None, d_off_ptr or None, n, 1 if paired else 0, d_text1_ptr or None, bytes1,
                                                   d_names_ptr or None, dnames._h, 1 if drop_unclassified else 0, d_out_ptr or None, out_cap,
                                                   d_info_ptr or None, stream or None))

    def classify_text_to_text_names(self, dtax: "DeviceTaxonomy", dnames: "DeviceTaxonNames", text1, text2=None, fastq=True, keep_names=False,
                                    drop_unclassified=False, rec_cap=None, out_cap=None):
        """classify_text_to_text with the column of kaiju-addTaxonNames (kaiju_gpu_classify_text_to_text_names).  Returns a dict:
        text (bytes), info (PARSE_INFO_DTYPE record), format_info (FORMAT_NAMES_INFO_DTYPE record)."""
        t1, t2, cap = _text_args(text1, text2, rec_cap)
        ocap = int(out_cap) if out_cap is not None else int(lib().kaiju_gpu_format_names_bound(len(t1) - 1, cap, dnames._h))
        out = np.zeros(ocap + 1, dtype=np.uint8)
        info = np.zeros(1, dtype=PARSE_INFO_DTYPE)
        finfo = np.zeros(1, dtype=FORMAT_NAMES_INFO_DTYPE)
        _check(lib().kaiju_gpu_classify_text_to_text_names(self._h, dtax._h, t1.ctypes.data, len(t1) - 1, t2.ctypes.data if t2 is not None else None,
                                                           len(t2) - 1 if t2 is not None else 0, 1 if fastq else 0, 1 if keep_names else 0, cap,
                                                           dnames._h, 1 if drop_unclassified else 0, out.ctypes.data, ocap, info.ctypes.data,
                                                           finfo.ctypes.data))
        return {"text": out[: int(finfo[0]["text_bytes"])].tobytes(), "info": info[0], "format_info": finfo[0]}

    def format_verbose(self, hits: np.ndarray, v: np.ndarray, text_pos: np.ndarray, text, recs: np.ndarray, off: np.ndarray, names_text,
                       names: np.ndarray, paired=False, text_cap=0xffffffff, out_cap=None, out=None):
        """what classify_verbose_packed returns (hit records, kaiju_gpu_verbose records, positions, the packed peptides), the
        compact records, off[], the text the names lie in and the name spans to the lines of kaiju -v
        (kaiju_gpu_format_verbose): host buffers, blocking.  Returns (out, info): out is a uint8 array of which the lines
        written have changed (out_cap bytes), info a FORMAT_VERBOSE_INFO_DTYPE record.  Index.upload_accessions() first."""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        v = np.ascontiguousarray(v, dtype=VERBOSE_DTYPE)
        text_pos = np.ascontiguousarray(text_pos, dtype=np.uint64)
        recs = np.ascontiguousarray(recs, dtype=COMPACT_DTYPE)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        names = np.ascontiguousarray(names, dtype=NAME_SPAN_DTYPE)
        pep = np.frombuffer(bytes(text) + b"\0", dtype=np.uint8)
        nt = np.frombuffer(bytes(names_text) + b"\0", dtype=np.uint8)
        n = len(recs)
        assert len(off) == 2 * n + 1 and len(names) == n and len(hits) == n and len(v) == n and len(text_pos) == n
        assert out_cap is not None or out is not None
        cap = int(out_cap) if out_cap is not None else len(out)
        if out is None:
            out = np.zeros(cap + 1, dtype=np.uint8)
        assert out.dtype == np.uint8 and len(out) >= cap
        info = np.zeros(1, dtype=FORMAT_VERBOSE_INFO_DTYPE)
        _check(lib().kaiju_gpu_format_verbose(self._h, hits.ctypes.data, v.ctypes.data, text_pos.ctypes.data, pep.ctypes.data, len(pep) - 1, int(text_cap),
                                              recs.ctypes.data, off.ctypes.data, n, 1 if paired else 0, nt.ctypes.data, len(nt) - 1, names.ctypes.data,
                                              out.ctypes.data, cap, info.ctypes.data))
        return out, info[0]

    def format_verbose_device(self, d_hits_ptr: int, d_recs_ptr: int, d_off_ptr: int, n: int, d_n_acc_ptr: int, d_acc_iseq_ptr: int,
                              d_text_pos_ptr: int, d_text_len_ptr: int, d_pep_ptr: int, text_cap: int, d_names_text_ptr: int, names_bytes: int,
                              d_names_ptr: int, d_out_ptr: int, out_cap: int, d_info_ptr: int, paired=False, stream: int = 0):
        """the same for device-resident buffers (raw pointers; d_out 16-byte aligned): kaiju_gpu_format_verbose_device,
        asynchronous on ``stream``"""
        _check(lib().kaiju_gpu_format_verbose_device(self._h, d_hits_ptr or None, d_recs_ptr or None, d_off_ptr or None, n, 1 if paired else 0,
                                                     d_n_acc_ptr or None, d_acc_iseq_ptr or None, d_text_pos_ptr or None, d_text_len_ptr or None,
                                                     d_pep_ptr or None, int(text_cap), d_names_text_ptr or None, names_bytes, d_names_ptr or None,
                                                     d_out_ptr or None, out_cap, d_info_ptr or None, stream or None))

    def classify_verbose_text(self, dtax: "DeviceTaxonomy", seqs: np.ndarray, off: np.ndarray, names_text, names: np.ndarray, paired=False):
        """reads in, the lines of kaiju -v out (kaiju_gpu_classify_batch_verbose_text).  Returns (text as bytes - a copy, the
        library's own is valid until the context's next verbose call -, a FORMAT_VERBOSE_INFO_DTYPE record)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        names = np.ascontiguousarray(names, dtype=NAME_SPAN_DTYPE)
        nt = np.frombuffer(bytes(names_text) + b"\0", dtype=np.uint8)
        n = (len(off) - 1) // 2
        assert len(names) == n
        text = C.c_void_p()
        nbytes = C.c_uint64()
        info = np.zeros(1, dtype=FORMAT_VERBOSE_INFO_DTYPE)
        _check(lib().kaiju_gpu_classify_batch_verbose_text(self._h, dtax._h, seqs.ctypes.data, off.ctypes.data, n, 1 if paired else 0, nt.ctypes.data,
                                                           len(nt) - 1, names.ctypes.data, C.byref(text), C.byref(nbytes), info.ctypes.data))
        return (C.string_at(text.value, nbytes.value) if nbytes.value else b""), info[0]

    def format_seq(self, hits: np.ndarray, off: np.ndarray, names_text, names: np.ndarray, paired=False, u_rule=U_RULE_NUCLEOTIDE, seqs=None,
                   v=None, text_pos=None, text=None, text_cap=0xffffffff, out_cap=None, out=None):
        """hit records of sequence numbers, off[], the text the names lie in and the name spans to the lines of kaijux / kaijup
        (kaiju_gpu_format_seq): host buffers, blocking.  seqs: the reads (U_RULE_PROTEIN only); text None: no peptide column, else
        v (kaiju_gpu_verbose records), text_pos and the packed peptides as classify_verbose_packed returns them.  Returns (out,
        info): out is a uint8 array of which the lines written have changed (out_cap bytes), info a FORMAT_VERBOSE_INFO_DTYPE
        record.  Index.upload_seq_names() first."""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        names = np.ascontiguousarray(names, dtype=NAME_SPAN_DTYPE)
        nt = np.frombuffer(bytes(names_text) + b"\0", dtype=np.uint8)
        n = len(hits)
        assert len(off) == 2 * n + 1 and len(names) == n
        sq = None if seqs is None else np.frombuffer(bytes(seqs) + b"\0", dtype=np.uint8)
        pep = None
        if text is not None:
            v = np.ascontiguousarray(v, dtype=VERBOSE_DTYPE)
            text_pos = np.ascontiguousarray(text_pos, dtype=np.uint64)
            pep = np.frombuffer(bytes(text) + b"\0", dtype=np.uint8)
            assert len(v) == n and len(text_pos) == n
        assert out_cap is not None or out is not None
        cap = int(out_cap) if out_cap is not None else len(out)
        if out is None:
            out = np.zeros(cap + 1, dtype=np.uint8)
        assert out.dtype == np.uint8 and len(out) >= cap
        info = np.zeros(1, dtype=FORMAT_VERBOSE_INFO_DTYPE)
        _check(lib().kaiju_gpu_format_seq(self._h, hits.ctypes.data, off.ctypes.data, n, 1 if paired else 0, int(u_rule), None if sq is None else sq.ctypes.data,
                                          None if pep is None else v.ctypes.data, None if pep is None else text_pos.ctypes.data,
                                          None if pep is None else pep.ctypes.data, 0 if pep is None else len(pep) - 1, int(text_cap), nt.ctypes.data,
                                          len(nt) - 1, names.ctypes.data, out.ctypes.data, cap, info.ctypes.data))
        return out, info[0]

    def format_seq_device(self, d_hits_ptr: int, d_off_ptr: int, n: int, d_seqs_ptr: int, d_text_pos_ptr: int, d_text_len_ptr: int, d_pep_ptr: int,
                          text_cap: int, d_names_text_ptr: int, names_bytes: int, d_names_ptr: int, d_out_ptr: int, out_cap: int, d_info_ptr: int,
                          paired=False, u_rule=U_RULE_NUCLEOTIDE, stream: int = 0):
        """the same for device-resident buffers (raw pointers; d_out 16-byte aligned; d_pep 0: no peptide column):
        kaiju_gpu_format_seq_device, asynchronous on ``stream``"""
        _check(lib().kaiju_gpu_format_seq_device(self._h, d_hits_ptr or None, d_off_ptr or None, n, 1 if paired else 0, int(u_rule), d_seqs_ptr or None,
                                                 d_text_pos_ptr or None, d_text_len_ptr or None, d_pep_ptr or None, int(text_cap), d_names_text_ptr or None,
                                                 names_bytes, d_names_ptr or None, d_out_ptr or None, out_cap, d_info_ptr or None, stream or None))

    def classify_seq_text(self, seqs: np.ndarray, off: np.ndarray, names_text, names: np.ndarray, paired=False, verbose=False, u_rule=U_RULE_NUCLEOTIDE):
        """reads in, the lines of kaijux / kaijup out (kaiju_gpu_classify_batch_seq_text).  Returns (text as bytes - a copy, the
        library's own is valid until the context's next verbose or text call -, a FORMAT_VERBOSE_INFO_DTYPE record)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        names = np.ascontiguousarray(names, dtype=NAME_SPAN_DTYPE)
        nt = np.frombuffer(bytes(names_text) + b"\0", dtype=np.uint8)
        n = (len(off) - 1) // 2
        assert len(names) == n
        text = C.c_void_p()
        nbytes = C.c_uint64()
        info = np.zeros(1, dtype=FORMAT_VERBOSE_INFO_DTYPE)
        _check(lib().kaiju_gpu_classify_batch_seq_text(self._h, seqs.ctypes.data, off.ctypes.data, n, 1 if paired else 0, 1 if verbose else 0, int(u_rule),
                                                       nt.ctypes.data, len(nt) - 1, names.ctypes.data, C.byref(text), C.byref(nbytes), info.ctypes.data))
        return (C.string_at(text.value, nbytes.value) if nbytes.value else b""), info[0]

    OP_COUNT_NAMES = ("kmer_lookups", "update_si", "update_si_lines", "lf_steps", "lf_lines", "sa_samples", "read_meta",
                      "frag_desc", "window_fills", "term_searches", "si_spills", "hits", "multi_letter_steps", "items_read",
                      "matches_read", "items_written", "matches_written", "wave_iterations", "lane_iterations", "record_bytes", "pruned_chains", "window_lines")

    def count_ops(self, on: bool):
        """accounting: the next batches run the counting instantiation of the search lane (never a timed launch)"""
        _check(lib().kaiju_gpu_set_count_ops(self._h, 1 if on else 0))

    def op_counts(self) -> dict:
        v = np.zeros(len(self.OP_COUNT_NAMES), dtype=np.uint64)
        _check(lib().kaiju_gpu_get_op_counts(self._h, v.ctypes.data, len(v)))
        return {k: int(x) for k, x in zip(self.OP_COUNT_NAMES, v)}

    def seg_regions(self, seqs: np.ndarray, off: np.ndarray, exact=False):
        """diagnostics (kaiju_gpu_seg_regions; protein contexts with seg): what the device SEG pass computed for every
        fragment of the batch - (kaiju_gpu_seg_fragment records, the (left, right) pairs they point into); exact: the SEG
        kernel of the exact pass instead of the SEG pass proper"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = (len(off) - 1) // 2
        fcap, lcap = 2 * n + 64, 16 * n + 1024
        while True:
            frags = np.zeros(fcap, dtype=SEG_FRAGMENT_DTYPE)
            lr = np.zeros((lcap, 2), dtype=np.int32)
            nf, nl = C.c_uint64(0), C.c_uint64(0)
            _check(lib().kaiju_gpu_seg_regions(self._h, seqs.ctypes.data, off.ctypes.data, n, 1 if exact else 0,
                                               frags.ctypes.data, fcap, C.byref(nf), lr.ctypes.data, lcap, C.byref(nl)))
            if nf.value <= fcap and nl.value <= lcap:
                return frags[: nf.value], lr[: nl.value]
            fcap, lcap = max(fcap, nf.value), max(lcap, nl.value)

    def lca(self, dtax: "DeviceTaxonomy", hits: np.ndarray) -> np.ndarray:
        """host hit records -> compact records through the LCA kernel (blocking)"""
        hits = np.ascontiguousarray(hits)
        out = np.zeros(len(hits), dtype=COMPACT_DTYPE)
        _check(lib().kaiju_gpu_lca_batch(self._h, dtax._h, hits.ctypes.data, len(hits), out.ctypes.data))
        return out

    def finalize_compact(self, recs: np.ndarray, off: np.ndarray, paired=False) -> np.ndarray:
        """E-value gate + C/U decision for compact records (their LCA was computed on the device)."""
        recs = np.ascontiguousarray(recs)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(recs)
        res = np.zeros(n, dtype=RESULT_DTYPE)
        _check(lib().kaiju_finalize_compact(C.byref(self.params), self.index.db_length, recs.ctypes.data,
                                            off.ctypes.data, n, 1 if paired else 0, res.ctypes.data))
        return res

    def close(self):
        if self._h:
            lib().kaiju_gpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


Context = Classifier


def _text_args(text1, text2, rec_cap):
    """texts as uint8 arrays with one byte of slack behind them (an empty text still has an address); the capacity: as many
    records as there are lines unless the caller knows better"""
    def arr(t):
        a = np.frombuffer(bytes(t), dtype=np.uint8) if not isinstance(t, np.ndarray) else np.ascontiguousarray(t, dtype=np.uint8)
        return np.concatenate([a, np.zeros(1, dtype=np.uint8)])
    t1 = arr(text1)
    t2 = arr(text2) if text2 is not None else None
    cap = int(rec_cap) if rec_cap is not None else int(np.count_nonzero(t1[:-1] == 10)) + 1
    return t1, t2, cap


def format_bound(bytes1: int, n: int) -> int:
    """an out_cap that cannot overflow for n records whose names are disjoint pieces of a text of bytes1 bytes"""
    return int(lib().kaiju_gpu_format_bound(bytes1, n))


def _reads_emitted(info, paired, cap):
    n = min(int(info["n_records"]), int(info["n_records2"])) if paired else int(info["n_records"])
    return min(n, cap)


def parse_block(ctx: Classifier, text1, text2=None, fastq=True, keep_names=False, rec_cap=None, names_fill=None):
    """Record extraction on the device (kaiju_gpu_parse_block): FASTQ / FASTA text (bytes or uint8 arrays; text2: the mates)
    to the buffers the classification entry points take.  Returns a dict: seqs (uint8), off (uint64, 2n + 1), names
    (n x 2 uint32: position and length of every name in text1), info (PARSE_INFO_DTYPE record) and names_all, the whole
    name buffer of rec_cap entries (pre-set to names_fill: what lies behind the reads emitted is not written)."""
    t1, t2, cap = _text_args(text1, text2, rec_cap)
    seqs = np.zeros(len(t1) + (len(t2) if t2 is not None else 0), dtype=np.uint8)
    off = np.zeros(2 * cap + 1, dtype=np.uint64)
    names = np.zeros(cap + 1, dtype=NAME_SPAN_DTYPE)
    if names_fill is not None:
        names.view("<u4")[:] = names_fill
    info = np.zeros(1, dtype=PARSE_INFO_DTYPE)
    _check(lib().kaiju_gpu_parse_block(ctx._h, t1.ctypes.data, len(t1) - 1, t2.ctypes.data if t2 is not None else None,
                                       len(t2) - 1 if t2 is not None else 0, 1 if fastq else 0, 1 if keep_names else 0, cap,
                                       seqs.ctypes.data, off.ctypes.data, names.ctypes.data, info.ctypes.data))
    n = _reads_emitted(info[0], t2 is not None, cap)
    return {"seqs": seqs[: int(info[0]["seq_bytes"])], "off": off[: 2 * n + 1], "names": names[:n].view("<u4").reshape(n, 2),
            "info": info[0], "names_all": names[:cap].view("<u4").reshape(cap, 2)}
