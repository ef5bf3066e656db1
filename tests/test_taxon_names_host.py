"""The host side of the column of kaiju-addTaxonNames (kaiju_amd/csrc/taxon_names.cpp) through the library: the two parsers
on tests/golden/names/deep/ against tests/names_expect.py (the reference tool pins that file), the refusals, and the loader as
a stand-alone program under the address and undefined-behaviour sanitizers (tests/tools/taxon_names_san.cpp)."""
import ctypes as C
import os
import subprocess

import pytest

import names_expect
import names_inputs
import util
from kaiju_amd import api


def test_parser_on_deep():
    for mode in names_inputs.MODES:
        t = api.TaxonNames(names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, mode)
        e = names_inputs.deep_expect(mode)
        assert t.count() == len(e.nodes) and t.count(named=True) == sum(1 for i in e.nodes if i in e.names)
        for taxon in names_inputs.deep_taxa():
            assert t.annotation(taxon) == e.annotation(taxon), (mode, taxon)
        t.close()


def test_parser_on_golden(golden):
    e = names_expect.Names(names_inputs.read(golden.nodes), names_inputs.read(names_inputs.GOLDEN_NAMES), "path")
    t = api.TaxonNames(golden.nodes, names_inputs.GOLDEN_NAMES, "path")
    assert t.count() == len(e.nodes) == 65 and t.count(named=True) == 63
    for taxon in list(e.nodes) + [0, 2, 5]:
        assert t.annotation(taxon) == e.annotation(taxon)
    assert t.annotation(100005) is None and b"taxonid:1003; " in t.annotation(100012)


def test_rank_lists(tmp_path):
    e = names_inputs.deep_expect
    for ranks in ("genus", "species,,genus,", ",", "", "no rank,genus", "Genus,genus", "species group,embl", ",".join(["genus"] * 64),
                  ",".join("abcdefghijklmnop")):
        t = api.TaxonNames(names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, "ranks:" + ranks)
        want = e("ranks:" + ranks)
        for taxon in (1, 1039, 4001, 78, 5059, 12):
            assert t.annotation(taxon) == want.annotation(taxon), (ranks, taxon)
    with pytest.raises(api.KaijuGpuError, match="16 distinct ranks"):
        api.TaxonNames(names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, "ranks:" + ",".join("abcdefghijklmnopq"))
    with pytest.raises(api.KaijuGpuError, match="64 items"):
        api.TaxonNames(names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, "ranks:" + ",".join(["genus"] * 65))


def test_cycle_is_refused(tmp_path):
    nodes = tmp_path / "nodes.dmp"
    nodes.write_bytes(b"1\t|\t1\t|\tno rank\t|\n5\t|\t1\t|\tgenus\t|\n20\t|\t21\t|\tgenus\t|\n21\t|\t22\t|\tgenus\t|\n22\t|\t20\t|\tgenus\t|\n23\t|\t22\t|\tspecies\t|\n")
    with pytest.raises(api.KaijuGpuError) as err:
        api.TaxonNames(str(nodes), names_inputs.DEEP_NAMES, "path")
    assert "(-1)" in str(err.value) and "cycle" in str(err.value) and any(" %d" % i in str(err.value) for i in (20, 21, 22))
    # two nodes that are each other's parent
    nodes.write_bytes(b"1\t|\t1\t|\tno rank\t|\n30\t|\t31\t|\tgenus\t|\n31\t|\t30\t|\tgenus\t|\n")
    with pytest.raises(api.KaijuGpuError, match="cycle"):
        api.TaxonNames(str(nodes), names_inputs.DEEP_NAMES, "name")
    # the self-parent is none, wherever it stands
    nodes.write_bytes(b"40\t|\t40\t|\tgenus\t|\n41\t|\t40\t|\tspecies\t|\n")
    assert api.TaxonNames(str(nodes), names_inputs.DEEP_NAMES, "path").count() == 2


def test_missing_files_and_arguments(tmp_path):
    for nodes, names in ((str(tmp_path / "none"), names_inputs.DEEP_NAMES), (names_inputs.DEEP_NODES, str(tmp_path / "none"))):
        with pytest.raises(api.KaijuGpuError, match=r"\(-2\)"):
            api.TaxonNames(nodes, names)
    h = C.c_void_p()
    L = api.lib()
    assert L.kaiju_taxon_names_load(None, None, 0, None, C.byref(h)) == -1
    assert L.kaiju_taxon_names_load(names_inputs.DEEP_NODES.encode(), names_inputs.DEEP_NAMES.encode(), 3, None, C.byref(h)) == -1 and not h
    assert L.kaiju_taxon_names_annotation(None, 1, None, 0) == -1
    # empty files: a table without nodes
    (tmp_path / "empty").write_bytes(b"")
    t = api.TaxonNames(str(tmp_path / "empty"), str(tmp_path / "empty"), "path")
    assert t.count() == 0 and t.annotation(1) is None


def test_entry_points_exist_and_need_a_device():
    L = api.lib()
    for sym in ("kaiju_gpu_taxon_names_upload", "kaiju_gpu_taxon_names_free", "kaiju_gpu_format_names", "kaiju_gpu_format_names_device",
                "kaiju_gpu_format_names_bound", "kaiju_gpu_classify_text_to_text_names", "kaiju_gpu_taxon_names_read"):
        assert hasattr(L, sym), sym
    assert L.kaiju_gpu_format_names_bound(1000, 17, None) == 1000 + 17 * 25
    if api.device_count() > 0:
        return            # (a HIP device is visible: the answer without one cannot be seen here)
    t = api.TaxonNames(names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, "path")
    with pytest.raises(api.KaijuGpuError, match=r"\(-4\)"):
        api.DeviceTaxonNames(t, 0)
    assert L.kaiju_gpu_format_names_device(None, None, None, 0, 0, None, 0, None, None, 0, None, 0, None, None) == -4


def test_loader_under_the_sanitizers(tmp_path, golden):
    """a plain executable of its own: nothing is loaded into this process"""
    exe = str(tmp_path / "taxon_names_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(util.ROOT, "tests", "tools", "taxon_names_san.cpp"), os.path.join(util.ROOT, "kaiju_amd", "csrc", "taxon_names.cpp")], check=True)
    env = dict(os.environ, TMPDIR=str(tmp_path))
    r = subprocess.run([exe, names_inputs.DEEP_NODES, names_inputs.DEEP_NAMES, golden.nodes, names_inputs.GOLDEN_NAMES], env=env, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout.rstrip().endswith(b" ok"), (r.returncode, r.stdout[-300:], r.stderr[-2000:])
