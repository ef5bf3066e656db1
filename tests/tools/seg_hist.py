"""Workload statistics of s_Trim (host emulation built with -DKJ_SEG_HIST): the lengths of the raw segments seg_trim is called
with and of the sub-windows it evaluates, on reads made by the benchmark's recipe (synth.make_reads over synth.make_db), every
flagged fragment through the SEG pass (the Greedy flow; MEM's lazy flow sends a subset of the same fragments).  Says what share
of the windows the window-probability table (kj_core.h: kSegTabMax) serves.

    python tests/tools/seg_hist.py [reads] [database sequences] > profiles/<dir>/seg_hist.json
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import util  # noqa: E402
from kaiju_amd import mkfmi, synth  # noqa: E402

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
nseq = int(sys.argv[2]) if len(sys.argv) > 2 else 3001

so = os.path.join(util.EMU_DIR, "libkaiju_kernel_emu_seghist.so")
srcs = [os.path.join(util.EMU_DIR, f) for f in ("kernel_emu.cpp", "seg_hist_counters.cpp")] + \
       [os.path.join(util.CSRC, f) for f in ("host_index.cpp", "host_tables.cpp", "taxonomy.cpp")]
subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-pthread", "-DKJ_SEG_HIST", "-o", so] + srcs, check=True)
emu = util.Emu(so=so)

os.environ["KAIJU_EMU_LAZY_OFF"] = "1"          # every flagged fragment goes through the SEG pass
with tempfile.TemporaryDirectory() as W:
    lines, leaves = synth.make_taxonomy()
    db = synth.make_db(nseq=nseq, seed=12345, leaves=leaves)
    faa, fmi = os.path.join(W, "db.faa"), os.path.join(W, "db.fmi")
    synth.write_fasta(db, faa)
    mkfmi.build_fmi(faa, fmi, threads=4, exponent=3)
    h = emu.load(fmi)
    reads = synth.make_reads(db, n_reads, seed=777)
    seqs, off = synth.pack_reads(reads)
    hist = np.zeros((4, 64), dtype=np.uint64)
    emu.lib.emu_seg_hist(hist.ctypes.data_as(C.c_void_p), 1)
    emu.classify(h, util.gp("mem"), seqs, off)
    emu.lib.emu_seg_hist(hist.ctypes.data_as(C.c_void_p), 1)

raw, served, direct, other = (hist[k].astype(np.int64) for k in range(4))
windows = served + direct + other
cum = np.cumsum(windows)
out = {"reads": n_reads, "database_sequences": nseq, "seg_trim_calls": int(raw.sum()),
       "raw_segment_length_hist (index = residues, 63 = 63 and more)": raw.tolist(),
       "window_length_hist (index = residues, 63 = 63 and more)": windows.tolist(),
       "windows": int(windows.sum()), "windows_from_table": int(served.sum()), "windows_computed_prefix_path": int(direct.sum()),
       "windows_computed_other_paths": int(other.sum()),
       "share_of_windows_up_to": {str(m): round(float(cum[m]) / max(1, int(cum[-1])), 5) for m in (16, 20, 24, 32, 40, 48, 62)},
       "share_of_raw_segments_up_to": {str(m): round(float(np.cumsum(raw)[m]) / max(1, int(raw.sum())), 5) for m in (16, 20, 24, 32, 40, 48, 62)}}
print(json.dumps(out, indent=1))
