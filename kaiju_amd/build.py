"""Build the HIP library in-tree: kaiju_amd/libkaiju_gpu.so (gfx950).

hipcc cross-compiles without a GPU, so this runs in the build container as well as on the
GPU box.  The library is the product: kernels + C-ABI (include/kaiju_gpu.h)."""
from __future__ import annotations

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libkaiju_gpu.so")
SOURCES = ["capi.hip", "capi_index.hip", "capi_text.hip", "fmi_stream.hip", "exact_pass.hip", "ingest.hip", "format.hip", "format_verbose.hip", "format_seq.hip", "format_names.hip", "annotate.hip", "merge.hip", "tally.hip", "krona.hip", "accmap.hip", "convert.hip", "gbk.hip", "taxon_names.cpp", "accessions.cpp", "host_index.cpp", "host_tables.cpp", "taxonomy.cpp", "rccl_gather.cpp"]
HEADERS = ["capi_internal.h", "kj_core.h", "kj_flow.h", "kj_rowtax_plan.h", "kj_greedy3.h", "fmi_stream.h", "exact_pass.h", "kj_ingest.h", "kj_format.h", "kj_format_verbose.h", "kj_format_seq.h", "kj_format_names.h", "kj_annotate.h", "kj_merge.h", "kj_tally.h", "kj_krona.h", "kj_convert.h", "kj_gbk.h", "kj_textlines.h", os.path.join("host", "table_rows.h"), "taxon_names.h", "kj_scan.h", "kj_lines.h", "host_index.h", "host_tables.h", os.path.join("..", "..", "include", "kaiju_gpu.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-fno-gpu-rdc", "-Wno-unused-result"]


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the Kaiju GPU library cannot be built")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


MKFMI_LIB = os.path.join(HERE, "libkaiju_mkfmi.so")
MKFMI_SRC = [os.path.join(CSRC, "mkfmi.cpp"), os.path.join(CSRC, "mkfmi.h"), os.path.join(CSRC, "kj_fmibuild.h")]


def build_mkfmi(force=False, verbose=False):
    """the index builder: test / benchmark infrastructure in a library of its own (host only; csrc/mkfmi.h says why it exists)"""
    if force or not os.path.exists(MKFMI_LIB) or any(os.path.getmtime(d) > os.path.getmtime(MKFMI_LIB) for d in MKFMI_SRC):
        cmd = ["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-result", "-o", MKFMI_LIB, MKFMI_SRC[0], "-lpthread"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return MKFMI_LIB


MKFMI_GPU_LIB = os.path.join(HERE, "libkaiju_mkfmi_gpu.so")
MKFMI_GPU_SRC = [os.path.join(CSRC, f) for f in ("mkfmi.cpp", "sufsort.hip", "fmibuild.hip", "mkfmi.h", "kj_sufsort.h", "kj_fmibuild.h")]


def build_mkfmi_gpu(force=False, verbose=False):
    """the index builder with the suffix sort (csrc/kj_sufsort.h) and, asked to, the stages behind it (csrc/kj_fmibuild.h) on the
    device: the host builder's source with a define plus sufsort.hip and fmibuild.hip, a third library - libkaiju_mkfmi.so stays
    free of HIP and libkaiju_gpu.so free of the builder"""
    if force or not os.path.exists(MKFMI_GPU_LIB) or any(os.path.getmtime(d) > os.path.getmtime(MKFMI_GPU_LIB) for d in MKFMI_GPU_SRC):
        cmd = [hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fno-gpu-rdc", "-Wno-unused-result",
               "-DKAIJU_MKFMI_GPU", "-o", MKFMI_GPU_LIB] + MKFMI_GPU_SRC[:3] + ["-lpthread"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return MKFMI_GPU_LIB


def build(force=False, verbose=False):
    build_mkfmi(force=force, verbose=verbose)
    build_mkfmi_gpu(force=force, verbose=verbose)
    if force or needs_build():
        cmd = [hipcc_path()] + FLAGS + ["-o", LIB] + [os.path.join(CSRC, s) for s in SOURCES] + ["-lpthread", "-ldl"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    build_cli(force=force, verbose=verbose)
    build_annotate_cli(force=force, verbose=verbose)
    build_merge_cli(force=force, verbose=verbose)
    build_table_cli(force=force, verbose=verbose)
    build_krona_cli(force=force, verbose=verbose)
    build_convert_cli(force=force, verbose=verbose)
    build_refseq_cli(force=force, verbose=verbose)
    build_gbk_cli(force=force, verbose=verbose)
    return LIB


CLI_SRC = os.path.join(CSRC, "host", "kaiju_main.cpp")
CLI = os.path.join(HERE, "bin", "kaiju")


def build_cli(force=False, verbose=False):
    """the drop-in `kaiju` command (host C++ over the C-ABI)"""
    multi = os.path.join(os.path.dirname(CLI), "kaiju-multi")
    if (not force and os.path.exists(CLI) and os.path.exists(multi) and os.path.exists(os.path.join(os.path.dirname(CLI), "kaijux")) and
            os.path.exists(os.path.join(os.path.dirname(CLI), "kaijup")) and
            os.path.getmtime(CLI) >= max(os.path.getmtime(CLI_SRC), os.path.getmtime(LIB))):
        return CLI
    os.makedirs(os.path.dirname(CLI), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-o", CLI, CLI_SRC, "-L" + HERE, "-lkaiju_gpu", "-lz", "-lpthread",
           "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    # kaiju-multi is the same program (it looks at its name): comma separated file lists, one index load
    import shutil as _sh
    _sh.copy2(CLI, multi)
    _sh.copy2(CLI, os.path.join(os.path.dirname(CLI), "kaijux"))      # kaijux: database sequences instead of taxa
    _sh.copy2(CLI, os.path.join(os.path.dirname(CLI), "kaijup"))      # kaijup: kaijux for protein reads
    return CLI


ANNOTATE_SRC = [os.path.join(CSRC, "host", f) for f in ("annotate_main.cpp", "annotate_blocks.h")]
ANNOTATE_CLI = os.path.join(HERE, "bin", "kaiju-addTaxonNames")


def build_annotate_cli(force=False, verbose=False):
    """the drop-in `kaiju-addTaxonNames` command (host C++ over the C-ABI)"""
    if not force and os.path.exists(ANNOTATE_CLI) and os.path.getmtime(ANNOTATE_CLI) >= max([os.path.getmtime(LIB)] + [os.path.getmtime(s) for s in ANNOTATE_SRC]):
        return ANNOTATE_CLI
    os.makedirs(os.path.dirname(ANNOTATE_CLI), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-o", ANNOTATE_CLI, ANNOTATE_SRC[0], "-L" + HERE, "-lkaiju_gpu", "-lpthread", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return ANNOTATE_CLI


MERGE_SRC = [os.path.join(CSRC, "host", f) for f in ("merge_main.cpp", "merge_blocks.h")]
MERGE_CLI = os.path.join(HERE, "bin", "kaiju-mergeOutputs")


def build_merge_cli(force=False, verbose=False):
    """the drop-in `kaiju-mergeOutputs` command (host C++ over the C-ABI)"""
    if not force and os.path.exists(MERGE_CLI) and os.path.getmtime(MERGE_CLI) >= max([os.path.getmtime(LIB)] + [os.path.getmtime(s) for s in MERGE_SRC]):
        return MERGE_CLI
    os.makedirs(os.path.dirname(MERGE_CLI), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-o", MERGE_CLI, MERGE_SRC[0], "-L" + HERE, "-lkaiju_gpu", "-lpthread", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return MERGE_CLI


TABLE_SRC = [os.path.join(CSRC, "host", f) for f in ("table_main.cpp", "table_rows.h", "annotate_blocks.h")] + [os.path.join(CSRC, "kj_tally.h")]
TABLE_CLI = os.path.join(HERE, "bin", "kaiju2table")


def build_table_cli(force=False, verbose=False):
    """the drop-in `kaiju2table` command (host C++ over the C-ABI)"""
    if not force and os.path.exists(TABLE_CLI) and os.path.getmtime(TABLE_CLI) >= max([os.path.getmtime(LIB)] + [os.path.getmtime(s) for s in TABLE_SRC]):
        return TABLE_CLI
    os.makedirs(os.path.dirname(TABLE_CLI), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-o", TABLE_CLI, TABLE_SRC[0], "-L" + HERE, "-lkaiju_gpu", "-lpthread", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return TABLE_CLI


KRONA_SRC = [os.path.join(CSRC, "host", f) for f in ("krona_main.cpp", "annotate_blocks.h")]
KRONA_CLI = os.path.join(HERE, "bin", "kaiju2krona")


def build_krona_cli(force=False, verbose=False):
    """the drop-in `kaiju2krona` command (host C++ over the C-ABI)"""
    if not force and os.path.exists(KRONA_CLI) and os.path.getmtime(KRONA_CLI) >= max([os.path.getmtime(LIB)] + [os.path.getmtime(s) for s in KRONA_SRC]):
        return KRONA_CLI
    os.makedirs(os.path.dirname(KRONA_CLI), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-o", KRONA_CLI, KRONA_SRC[0], "-L" + HERE, "-lkaiju_gpu", "-lpthread", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return KRONA_CLI


CONVERT_SRC = [os.path.join(CSRC, "host", f) for f in ("convert_main.cpp", "convert_blocks.h", "refseq_options.h", "pargz.h")]
CONVERT_CLI = os.path.join(HERE, "bin", "kaiju-convertNR")


def build_convert_cli(force=False, verbose=False):
    """the drop-in `kaiju-convertNR` command (host C++ over the C-ABI)"""
    if not force and os.path.exists(CONVERT_CLI) and os.path.getmtime(CONVERT_CLI) >= max([os.path.getmtime(LIB)] + [os.path.getmtime(s) for s in CONVERT_SRC]):
        return CONVERT_CLI
    os.makedirs(os.path.dirname(CONVERT_CLI), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-o", CONVERT_CLI, CONVERT_SRC[0], "-L" + HERE, "-lkaiju_gpu", "-lz", "-lpthread", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return CONVERT_CLI


REFSEQ_CLI = os.path.join(HERE, "bin", "kaiju-convertRefSeq")


def build_refseq_cli(force=False, verbose=False):
    """the drop-in `kaiju-convertRefSeq` command: the source of `kaiju-convertNR` compiled for the other rule set"""
    if not force and os.path.exists(REFSEQ_CLI) and os.path.getmtime(REFSEQ_CLI) >= max([os.path.getmtime(LIB)] + [os.path.getmtime(s) for s in CONVERT_SRC]):
        return REFSEQ_CLI
    os.makedirs(os.path.dirname(REFSEQ_CLI), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-DKAIJU_CONVERT_REFSEQ", "-o", REFSEQ_CLI, CONVERT_SRC[0], "-L" + HERE, "-lkaiju_gpu", "-lz", "-lpthread", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return REFSEQ_CLI


GBK_SRC = [os.path.join(CSRC, "host", f) for f in ("gbk_main.cpp", "gbk_blocks.h", "pargz.h")]
GBK_CLI = os.path.join(HERE, "bin", "kaiju-gbk2faa")


def build_gbk_cli(force=False, verbose=False):
    """the drop-in `kaiju-gbk2faa` command (host C++ over the C-ABI)"""
    if not force and os.path.exists(GBK_CLI) and os.path.getmtime(GBK_CLI) >= max([os.path.getmtime(LIB)] + [os.path.getmtime(s) for s in GBK_SRC]):
        return GBK_CLI
    os.makedirs(os.path.dirname(GBK_CLI), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-o", GBK_CLI, GBK_SRC[0], "-L" + HERE, "-lkaiju_gpu", "-lz", "-lpthread", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return GBK_CLI


if __name__ == "__main__":
    build(force=True, verbose=True)
