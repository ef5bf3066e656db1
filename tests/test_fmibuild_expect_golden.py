"""The numpy expectation of the builder's arrays (tests/fmibuild_expect.py) against a file the reference's binaries wrote: for
the golden database at exponent 3 it must equal the sections of tests/golden/db.fmi - sequence order, samples, coded BWT, index1,
index2 and startLcode.  This pins the expectation, which every check of the device stages is made against, to the reference."""
import numpy as np

import fmibuild_expect as fe


def test_expectation_equals_the_sections_of_the_golden_file(golden):
    ref = fe.read_fmi(golden.fmi)
    assert ref["exponent"] == 3 and ref["alphabet"] == b"*ACDEFGHIKLMNPQRSTVWY"
    want = fe.expected("golden_db", 1, 3)
    assert fe.first_difference(want, ref) is None
    assert ref["mask"] == (1 << want["pbits"]) - 1 and ref["check"] == 7
    # the lengths of the file are those of the sequences in sorted order
    t = fe.text("golden_db")
    term = np.flatnonzero(t == 0)
    lens = term - np.concatenate(([0], term[:-1] + 1))
    assert np.array_equal(ref["lengths"], lens[want["read_of_rank"]])


def test_first_difference_names_the_element():
    want = fe.expected("iid_257", 1, 3)
    got = dict(want)
    got["bwt"] = want["bwt"].copy()
    got["bwt"][200] ^= 1
    assert fe.first_difference(got, want) == ("bwt", 200, int(got["bwt"][200]), int(want["bwt"][200]))
    assert fe.first_difference(want, want) is None and fe.first_difference(dict(want, bwt=want["bwt_raw"]), want, recode=False) is None
