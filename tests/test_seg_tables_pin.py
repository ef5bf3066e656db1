"""The ln(n!) table of SEG (blast_seg.c:52-1308, 10 001 entries printed with six decimals) is DERIVED - from lgamma, rounded to
six decimals - in the product (kaiju_amd/csrc/host_tables.cpp: build_seg_tables) and in the oracle (oracle/kaiju_oracle.c:
init_lnfact) alike: a shared assumption.  The printed table, parsed into tests/golden/seg_lnfact.npy (make_golden_lnfact.py),
is compared entry by entry, bit for bit, with both, and the two derivations with each other."""
import ctypes as C
import os

import numpy as np

import pyoracle as po

PRINTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_lnfact.npy")


def _tables(emu, golden):
    h = emu.load(golden.fmi)
    emu.lib.emu_lnfact.restype = C.c_double
    emu.lib.emu_lnfact.argtypes = [C.c_void_p, C.c_uint32]
    emu.lib.emu_lnfact_n.restype = C.c_uint32
    emu.lib.emu_lnfact_n.argtypes = [C.c_void_p]
    product = [emu.lib.emu_lnfact(h, n) for n in range(emu.lib.emu_lnfact_n(h))]
    O = po.Oracle()
    O.lib.ko_lnfact.restype = C.c_double
    O.lib.ko_lnfact.argtypes = [C.c_int]
    oracle = [O.lib.ko_lnfact(n) for n in range(O.lib.ko_lnfact_n())]
    return product, oracle


def test_product_and_oracle_derive_the_same_table(emu, golden):
    product, oracle = _tables(emu, golden)
    assert len(product) == len(oracle) == 10001
    assert product == oracle                      # doubles compared exactly
    assert product[0] == 0.0 and product[2] == 0.693147 and product[20] == 42.335616


def test_table_equals_the_one_printed_in_blast_seg_c(emu, golden):
    printed = np.load(PRINTED).tolist()
    product, oracle = _tables(emu, golden)
    assert len(printed) == 10001
    assert printed == product and printed == oracle
