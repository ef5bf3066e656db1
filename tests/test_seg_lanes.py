"""The SEG code of kj_core.h (seg_trim, seg_classes, seg_scan, seg_regions) run by W real lanes on the host - one context per
lane, a hand-over where the device has a barrier, the butterfly of the device's reduce_min (tests/emu/kernel_emu.cpp: CoopLanes,
emu_seg_lanes) - against the oracle's regions.  The rest of the host suite runs this code with one lane, where the strided
loops are plain loops, the reduction is empty and no barrier matters; here the distribution of s_Trim's sub-windows over the
lanes, the (probability, visiting order) tie-break, the prefix counts and window classes shared between lanes and "every lane
computes the same values" are under test without a GPU.  tests/test_gpu_seg_regions.py runs the same inputs on the device."""
import pytest

import seg_inputs as si

WIDTHS = (8, 16, 32, 64)
# what the device's k_seg / k_seg_teams do (prefix counts, window classes), and the other branches of seg_trim and seg_scan
VARIANTS = {"prefix+cls": (), "noprefix": ("KAIJU_EMU_NO_SEG_PREFIX",), "nocls": ("KAIJU_EMU_SEG_NOCLS",),
            "noprefix+nocls": ("KAIJU_EMU_NO_SEG_PREFIX", "KAIJU_EMU_SEG_NOCLS")}
# The work grows with the width (every lane scans the whole peptide; only s_Trim's sub-windows are shared), so the sets
# shrink with it (repeat lengths 12, 12 + step, ...; fuzzed peptides), and the three variants besides the device's
# configuration run thinned sets.  The lanes run in one thread: the file takes about 17 s (measured, one core; the emulation library already built).
TIE_STEP = {8: 1, 16: 2, 32: 3, 64: 4}
FUZZ = {8: 1000, 16: 600, 32: 400, 64: 300}


@pytest.fixture(scope="module")
def handle(emu, golden):
    return emu.load(golden.fmi)


@pytest.fixture(scope="module")
def seg_oracle(oracle):
    return si.SegOracle(oracle)


def check(emu, h, seg_oracle, width, peptides, what):
    """regions by `width` lanes == the oracle's; the scan lists overflow exactly where they do with one lane"""
    overflows = 0
    for aa in peptides:
        want = seg_oracle(aa)
        got = emu.seg_lanes(h, aa, width)
        one_lane_ov = emu.lib.emu_seg(h, aa, len(aa), *_scratch()) < 0
        assert (got is None) == one_lane_ov, (what, width, aa)
        if got is None:
            overflows += 1
            continue
        assert got == want, f"{what}, {width} lanes, peptide {aa.decode()}\n  lanes  {got}\n  oracle {want}\n  1 lane {emu.seg_rec(h, aa)[0]}"
    return overflows


def _scratch():
    import ctypes as C
    return (C.c_int32 * 64)(), (C.c_int32 * 64)()


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_lanes_equal_the_oracle(emu, handle, seg_oracle, monkeypatch, variant, width):
    for name in VARIANTS[variant]:
        monkeypatch.setenv(name, "1")
    full = variant == "prefix+cls"
    step = TIE_STEP[width] if full else 8
    ties = si.tie_cases(step=step)
    assert len(ties) == 20 * len(range(12, 141, step))
    assert check(emu, handle, seg_oracle, width, ties, "ties") == 0
    assert check(emu, handle, seg_oracle, width, si.tie_witnesses(seg_oracle), "tied minimum of s_Trim") == 0
    limits = si.limit_cases()
    assert {62, 63, 64, 65} <= {si.first_raw_segment(aa) for aa in limits}          # both sides of kSegPacked
    if not full:
        limits = limits[::2] + [aa for aa in limits if si.first_raw_segment(aa) in (62, 63, 64, 65)]
    assert check(emu, handle, seg_oracle, width, limits, "limits") == 0
    assert check(emu, handle, seg_oracle, width, si.window_cases(), "window") == 0
    fuzz = si.fuzz_cases(FUZZ[width] if full else 100)
    assert sum(1 for aa in fuzz if seg_oracle(aa)) > len(fuzz) * 2 // 3
    assert check(emu, handle, seg_oracle, width, fuzz, "fuzz") == 0
    for aa, regs in si.kat_cases():
        assert emu.seg_lanes(handle, aa, width) == regs, (width, aa)


@pytest.mark.parametrize("width", WIDTHS)
def test_lanes_at_the_record_limits(emu, handle, seg_oracle, width):
    """fragments with 14 .. 43 regions: the lists of the lanes equal the oracle's as long as the scan lists (32 segments) hold
    them, and overflow beyond"""
    cases = si.record_cases()
    for want, aa in cases.items():
        assert len(seg_oracle(aa)) == want
    assert sorted(cases) == [14, 15, 16, 31, 32, 33, 43]
    fit = [aa for want, aa in cases.items() if want <= 32]
    assert check(emu, handle, seg_oracle, width, fit, "record limits") == 0
    assert check(emu, handle, seg_oracle, width, [cases[33], cases[43]], "beyond the scan lists") == 2
