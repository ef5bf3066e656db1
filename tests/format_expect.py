"""What the format passes (kaiju_amd/csrc/format.hip, kj_format.h) must write, built without them: the decision per record is
taken from the library's host function kaiju_finalize_compact (the reference; it needs no device), the bytes are put together
here.  A case is a dict as tests/format_inputs.py makes them."""
import ctypes as C

import numpy as np

from kaiju_amd import api

FORMAT_INFO_DTYPE = np.dtype([("text_bytes", "<u8"), ("n_records", "<u4"), ("n_classified", "<u4"), ("overflow", "<u4"), ("n_inexact", "<u4")])
assert FORMAT_INFO_DTYPE.itemsize == 24
INFO_FIELDS = FORMAT_INFO_DTYPE.names
INEXACT = 0x80000000


def params_of(case):
    p = api.default_params(case["mode"], min_evalue=case["min_evalue"], input_is_protein=1 if case["protein"] else 0)
    return p


def finalize(params, db_length, recs, off, paired):
    """kaiju_finalize_compact: RESULT_DTYPE records"""
    n = len(recs)
    res = np.zeros(n, dtype=api.RESULT_DTYPE)
    if n:
        recs = np.ascontiguousarray(recs)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        assert api.lib().kaiju_finalize_compact(C.byref(params), float(db_length), recs.ctypes.data, off.ctypes.data, n, 1 if paired else 0,
                                                res.ctypes.data) == 0
    return res


def lines_of(res, names, text1):
    out = []
    for r in range(len(res)):
        p, l = int(names[r]["pos"]), int(names[r]["len"])
        name = bytes(text1[p:p + l])
        if res[r]["classified"]:
            out.append(b"C\t" + name + b"\t" + str(int(res[r]["taxon"])).encode() + b"\n")
        else:
            out.append(b"U\t" + name + b"\t0\n")
    return out


def expected(case, db_length, out_cap=None):
    """text: all lines; written: the whole lines that fit out_cap (None: everything fits); info: the fields of
    kaiju_gpu_format_info; line_off: where every line starts"""
    res = finalize(params_of(case), db_length, case["recs"], case["off"], case["paired"])
    lines = lines_of(res, case["names"], case["text1"])
    text = b"".join(lines)
    line_off = np.concatenate([[0], np.cumsum([len(l) for l in lines], dtype=np.int64)]).astype(np.int64)
    cap = len(text) if out_cap is None else out_cap
    fit = int(np.searchsorted(line_off, cap, side="right")) - 1
    info = {"text_bytes": len(text), "n_records": len(lines), "n_classified": int(np.count_nonzero(res["classified"])),
            "overflow": 1 if len(text) > cap else 0, "n_inexact": int(np.count_nonzero(case["recs"]["info"] & INEXACT))}
    return {"text": text, "written": text[: int(line_off[fit])], "info": info, "line_off": line_off, "res": res}
