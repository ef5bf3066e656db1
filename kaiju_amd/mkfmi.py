"""Index construction: protein FASTA -> Kaiju ``.fmi`` (the off-line step of kaiju-makedb,
util/kaiju-makedb:373-375: ``kaiju-mkbwt -a ACDEFGHIKLMNPQRSTVWY -e 3`` + ``kaiju-mkfmi``).
The file is format-compatible with the reference, which can read it unchanged.

Test / benchmark infrastructure (csrc/mkfmi.h): a library of its own, kaiju_amd/libkaiju_mkfmi.so, not part of the product's
C-ABI - the GPU box has no network and no reference binaries, bench.py and the tests make their indexes with it.

``device=<n>`` sorts the suffixes on that GPU (csrc/kj_sufsort.h) and writes the same bytes; it loads a third library,
kaiju_amd/libkaiju_mkfmi_gpu.so.  A file of 0xf0000000 bytes and more is sorted there with 64-bit positions (the wide instantiation
of the same sort), a smaller one with 32-bit positions; ``stages="device"`` is for the smaller ones.  With ``device=None`` (the default) that library is not touched.  ``stages="device"`` (with a
device; the default is ``"host"``) also runs the stages behind the sort there (csrc/kj_fmibuild.h): BWT, sequence ranks,
replication, samples, checkpoints and byte coding; the same bytes again.  ``fmi_arrays`` gives those arrays for a text without
writing a file, from the host stages or the device's."""
from __future__ import annotations

import ctypes as C

from . import api, build as _build

_LIB = None
_LIB_GPU = None


class FmiArrays(C.Structure):
    """kaiju_fmi_arrays (csrc/mkfmi.h)"""
    _fields_ = [("nseq", C.c_uint64), ("bwtlen", C.c_uint64), ("n_samples_bytes", C.c_uint64), ("n_index1", C.c_uint64), ("n_index2", C.c_uint64),
                ("ncheck", C.c_int64), ("nbytes", C.c_int32), ("sbits", C.c_int32), ("pbits", C.c_int32), ("N1", C.c_int32), ("N2", C.c_int32),
                ("reserved", C.c_int32), ("read_of_rank", C.c_void_p), ("samples", C.c_void_p), ("bwt", C.c_void_p), ("index1", C.c_void_p),
                ("index2", C.c_void_p), ("startLcode", C.c_int32 * 22)]


def _arrays_api(L):
    L.kaiju_build_fmi_error.restype = C.c_char_p
    L.kaiju_fmi_arrays_sizes.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(FmiArrays)]
    L.kaiju_fmi_arrays_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(FmiArrays)]
    return L


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = _arrays_api(C.CDLL(_build.build_mkfmi()))
    return _LIB


class SufsortStats(C.Structure):
    """kaiju_sufsort_stats (csrc/mkfmi.h)"""
    _fields_ = [("rounds", C.c_uint32), ("reserved", C.c_uint32), ("active", C.c_uint64 * 16), ("ms_sort", C.c_float), ("reserved2", C.c_float)]


class FmiBuildStats(C.Structure):
    """kaiju_fmi_build_stats (csrc/mkfmi.h)"""
    _fields_ = [("device_stages", C.c_uint32), ("reserved", C.c_uint32), ("ms_bwt", C.c_float), ("ms_ranks", C.c_float), ("ms_samples", C.c_float),
                ("ms_checkpoints", C.c_float), ("ms_recode", C.c_float), ("ms_download", C.c_float), ("device_bytes", C.c_uint64), ("sort", SufsortStats)]


STAGES = {"host": 0, "device": 1}                 # KAIJU_FMI_STAGES_*
STAGE_BITS = {"bwt": 1, "ranks": 2, "samples": 4, "checkpoints": 8, "recode": 16}      # KAIJU_FMI_STAGE_*


def _stats_dict(st):
    return {"device_stages": int(st.device_stages), "stages": [k for k, b in STAGE_BITS.items() if st.device_stages & b],
            "ms_bwt": float(st.ms_bwt), "ms_ranks": float(st.ms_ranks), "ms_samples": float(st.ms_samples), "ms_checkpoints": float(st.ms_checkpoints),
            "ms_recode": float(st.ms_recode), "ms_download": float(st.ms_download), "device_bytes": int(st.device_bytes),
            "sort": {"rounds": int(st.sort.rounds), "active": [int(a) for a in st.sort.active], "ms_sort": float(st.sort.ms_sort)}}


def _stages_value(stages):
    if stages not in STAGES:
        raise ValueError(f"stages = {stages!r}: 'host' or 'device'")
    return STAGES[stages]


def _lib_gpu():
    global _LIB_GPU
    if _LIB_GPU is None:
        L = C.CDLL(_build.build_mkfmi_gpu())
        L.kaiju_build_fmi_error.restype = C.c_char_p
        L.kaiju_build_fmi_device.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
        L.kaiju_build_fmi_replicated_device.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int]
        L.kaiju_suffix_sort_device.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(SufsortStats)]
        L.kaiju_suffix_sort_device_wide.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(SufsortStats), C.c_uint64]
        L.kaiju_build_fmi_device_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_int,
                                                C.POINTER(FmiBuildStats)]
        L.kaiju_fmi_arrays_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(FmiArrays), C.POINTER(FmiBuildStats)]
        _arrays_api(L)
        _LIB_GPU = L
    return _LIB_GPU


def suffix_sort(text, device: int = 0, wide: bool = False, rank_bias: int = 0):
    """the suffix array of a text (uint8 codes 0 .. 20, a terminator 0 behind every sequence) sorted on a GPU: (sa, stats) with
    sa the positions of the letters in suffix order (uint32) and stats = {"rounds", "active": suffixes not final in front of
    each of the first 16 rounds, "ms_sort"}.  wide: the instantiation of the sort with 64-bit positions (the one texts of
    0xf0000000 symbols and more take); sa is uint64 then.  rank_bias (wide only, a test hook): every rank inside the sort is that
    much higher, the result is the same."""
    import numpy as np
    if rank_bias and not wide:
        raise ValueError("rank_bias needs wide=True")
    L = _lib_gpu()
    t = np.ascontiguousarray(text, dtype=np.uint8)
    sa = np.empty(max(1, int(np.count_nonzero(t))), dtype=np.uint64 if wide else np.uint32)
    n, st = C.c_uint64(0), SufsortStats()
    if wide:
        rc = L.kaiju_suffix_sort_device_wide(t.ctypes.data, len(t), int(device), sa.ctypes.data, C.byref(n), C.byref(st), int(rank_bias))
    else:
        rc = L.kaiju_suffix_sort_device(t.ctypes.data, len(t), int(device), sa.ctypes.data, C.byref(n), C.byref(st))
    if rc != 0:
        raise api.KaijuGpuError(f"kaiju_suffix_sort_device{'_wide' if wide else ''} failed ({rc}): {L.kaiju_build_fmi_error().decode()}")
    return sa[: n.value], {"rounds": int(st.rounds), "active": [int(a) for a in st.active], "ms_sort": float(st.ms_sort)}


def fmi_arrays(text, copies: int = 1, exponent: int = 3, device=None, recode: bool = True, threads: int = 0):
    """the arrays of the .fmi of a text (uint8 codes 0 .. 20, a terminator 0 behind every sequence) without a file: (arrays, stats).
    arrays: read_of_rank (uint32), samples (uint8, ncheck entries of nbytes, big-endian), bwt (uint8; raw letters with recode=False),
    index1 (int64), index2 (uint16), startLcode (int32) and the scalars nseq, bwtlen, ncheck, nbytes, sbits, pbits, N1, N2.
    device=None: the host sort and the host stages (stats is None); device=<n>: the sort and all stages on that GPU."""
    import numpy as np
    L = _lib() if device is None else _lib_gpu()
    t = np.ascontiguousarray(text, dtype=np.uint8)
    a = FmiArrays()
    rc = L.kaiju_fmi_arrays_sizes(t.ctypes.data, len(t), int(copies), int(exponent), C.byref(a))
    if rc != 0:
        raise api.KaijuGpuError(f"kaiju_fmi_arrays_sizes failed ({rc}): {L.kaiju_build_fmi_error().decode()}")
    out = {"read_of_rank": np.zeros(max(1, a.nseq), dtype=np.uint32), "samples": np.full(max(1, a.n_samples_bytes), 0xee, dtype=np.uint8),
           "bwt": np.full(max(1, a.bwtlen), 0xee, dtype=np.uint8), "index1": np.full(max(1, a.n_index1), -1, dtype=np.int64),
           "index2": np.full(max(1, a.n_index2), 0xeeee, dtype=np.uint16)}
    for k, v in out.items():
        setattr(a, k, v.ctypes.data)
    st = None
    if device is None:
        rc = L.kaiju_fmi_arrays_host(t.ctypes.data, len(t), int(copies), int(exponent), int(threads), int(bool(recode)), C.byref(a))
    else:
        st = FmiBuildStats()
        rc = L.kaiju_fmi_arrays_device(t.ctypes.data, len(t), int(copies), int(exponent), int(device), int(bool(recode)), C.byref(a), C.byref(st))
    if rc != 0:
        raise api.KaijuGpuError(f"kaiju_fmi_arrays failed ({rc}): {L.kaiju_build_fmi_error().decode()}")
    sizes = {"read_of_rank": a.nseq, "samples": a.n_samples_bytes, "bwt": a.bwtlen, "index1": a.n_index1, "index2": a.n_index2}
    out = {k: v[: sizes[k]] for k, v in out.items()}
    out["startLcode"] = np.array(list(a.startLcode), dtype=np.int32)
    for k in ("nseq", "bwtlen", "ncheck", "nbytes", "sbits", "pbits", "N1", "N2"):
        out[k] = int(getattr(a, k))
    return out, (_stats_dict(st) if st is not None else None)


def build_fmi(faa_path: str, out_fmi_path: str, threads: int = 0, exponent: int = 3, device=None, stages: str = "host") -> str:
    """stages ("host" or "device", with a device only): where the stages behind the sort run; the same bytes either way"""
    sv = _stages_value(stages)
    if device is None and sv:
        raise ValueError("stages = 'device' needs a device")
    if device is not None and sv:
        L = _lib_gpu()
        rc = L.kaiju_build_fmi_device_ex(faa_path.encode(), out_fmi_path.encode(), threads, exponent, 1, None, 0, int(device), sv, None)
        if rc != 0:
            raise api.KaijuGpuError(f"kaiju_build_fmi_device_ex failed ({rc}): {L.kaiju_build_fmi_error().decode()}")
        return out_fmi_path
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


def build_fmi_replicated(faa_path: str, out_fmi_path: str, copies: int, threads: int = 0, exponent: int = 3, copy_taxids=None, device=None,
                         stages: str = "host") -> str:
    """the .fmi of the database in which every sequence of the FASTA occurs `copies` times in a row (kaiju_build_fmi_replicated:
    no second sort; test / benchmark infrastructure for indexes of 2^32 rows and more)"""
    import numpy as np
    sv = _stages_value(stages)
    if device is None and sv:
        raise ValueError("stages = 'device' needs a device")
    L = _lib() if device is None else _lib_gpu()
    L.kaiju_build_fmi_replicated.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_uint32]
    L.kaiju_build_fmi_error.restype = C.c_char_p
    tx = np.ascontiguousarray(copy_taxids, dtype=np.uint64) if copy_taxids is not None and len(copy_taxids) else None
    args = (faa_path.encode(), out_fmi_path.encode(), threads, exponent, int(copies), tx.ctypes.data if tx is not None else None,
            len(tx) if tx is not None else 0)
    if device is not None and sv:
        rc = L.kaiju_build_fmi_device_ex(*args, int(device), sv, None)
    else:
        rc = L.kaiju_build_fmi_replicated(*args) if device is None else L.kaiju_build_fmi_replicated_device(*args, int(device))
    if rc != 0:
        raise api.KaijuGpuError(f"kaiju_build_fmi_replicated failed ({rc}): {L.kaiju_build_fmi_error().decode()}")
    return out_fmi_path
