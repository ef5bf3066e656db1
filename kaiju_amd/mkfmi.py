"""Index construction: protein FASTA -> Kaiju ``.fmi`` (the off-line step of kaiju-makedb,
util/kaiju-makedb:373-375: ``kaiju-mkbwt -a ACDEFGHIKLMNPQRSTVWY -e 3`` + ``kaiju-mkfmi``).
The file is format-compatible with the reference, which can read it unchanged.

Test / benchmark infrastructure (csrc/mkfmi.h): a library of its own, kaiju_amd/libkaiju_mkfmi.so, not part of the product's
C-ABI - the GPU box has no network and no reference binaries, bench.py and the tests make their indexes with it.

``device=<n>`` sorts the suffixes on that GPU (csrc/kj_sufsort.h) and writes the same bytes; it loads a third library,
kaiju_amd/libkaiju_mkfmi_gpu.so.  With ``device=None`` (the default) that library is not touched."""
from __future__ import annotations

import ctypes as C

from . import api, build as _build

_LIB = None
_LIB_GPU = None


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(_build.build_mkfmi())
    return _LIB


class SufsortStats(C.Structure):
    """kaiju_sufsort_stats (csrc/mkfmi.h)"""
    _fields_ = [("rounds", C.c_uint32), ("reserved", C.c_uint32), ("active", C.c_uint64 * 16), ("ms_sort", C.c_float), ("reserved2", C.c_float)]


def _lib_gpu():
    global _LIB_GPU
    if _LIB_GPU is None:
        L = C.CDLL(_build.build_mkfmi_gpu())
        L.kaiju_build_fmi_error.restype = C.c_char_p
        L.kaiju_build_fmi_device.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        L.kaiju_build_fmi_replicated_device.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int]
        L.kaiju_suffix_sort_device.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(SufsortStats)]
        _LIB_GPU = L
    return _LIB_GPU


def suffix_sort(text, device: int = 0):
    """the suffix array of a text (uint8 codes 0 .. 20, a terminator 0 behind every sequence) sorted on a GPU: (sa, stats) with
    sa the positions of the letters in suffix order (uint32) and stats = {"rounds", "active": suffixes not final in front of
    each of the first 16 rounds, "ms_sort"}"""
    import numpy as np
    L = _lib_gpu()
    t = np.ascontiguousarray(text, dtype=np.uint8)
    sa = np.empty(max(1, int(np.count_nonzero(t))), dtype=np.uint32)
    n, st = C.c_uint64(0), SufsortStats()
    rc = L.kaiju_suffix_sort_device(t.ctypes.data, len(t), int(device), sa.ctypes.data, C.byref(n), C.byref(st))
    if rc != 0:
        raise api.KaijuGpuError(f"kaiju_suffix_sort_device failed ({rc}): {L.kaiju_build_fmi_error().decode()}")
    return sa[: n.value], {"rounds": int(st.rounds), "active": [int(a) for a in st.active], "ms_sort": float(st.ms_sort)}


def build_fmi(faa_path: str, out_fmi_path: str, threads: int = 0, exponent: int = 3, device=None) -> str:
    if device is not None:
        L = _lib_gpu()
        rc = L.kaiju_build_fmi_device(faa_path.encode(), out_fmi_path.encode(), threads, exponent, int(device))
        if rc != 0:
            raise api.KaijuGpuError(f"kaiju_build_fmi_device failed ({rc}): {L.kaiju_build_fmi_error().decode()}")
        return out_fmi_path
    L = _lib()
    L.kaiju_build_fmi.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.kaiju_build_fmi_error.restype = C.c_char_p
    rc = L.kaiju_build_fmi(faa_path.encode(), out_fmi_path.encode(), threads, exponent)
    if rc != 0:
        raise api.KaijuGpuError(f"kaiju_build_fmi failed ({rc}): {L.kaiju_build_fmi_error().decode()}")
    return out_fmi_path


def build_fmi_replicated(faa_path: str, out_fmi_path: str, copies: int, threads: int = 0, exponent: int = 3, copy_taxids=None, device=None) -> str:
    """the .fmi of the database in which every sequence of the FASTA occurs `copies` times in a row (kaiju_build_fmi_replicated:
    no second sort; test / benchmark infrastructure for indexes of 2^32 rows and more)"""
    import numpy as np
    L = _lib() if device is None else _lib_gpu()
    L.kaiju_build_fmi_replicated.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_uint32]
    L.kaiju_build_fmi_error.restype = C.c_char_p
    tx = np.ascontiguousarray(copy_taxids, dtype=np.uint64) if copy_taxids is not None and len(copy_taxids) else None
    args = (faa_path.encode(), out_fmi_path.encode(), threads, exponent, int(copies), tx.ctypes.data if tx is not None else None,
            len(tx) if tx is not None else 0)
    rc = L.kaiju_build_fmi_replicated(*args) if device is None else L.kaiju_build_fmi_replicated_device(*args, int(device))
    if rc != 0:
        raise api.KaijuGpuError(f"kaiju_build_fmi_replicated failed ({rc}): {L.kaiju_build_fmi_error().decode()}")
    return out_fmi_path
