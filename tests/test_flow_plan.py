"""Which kernels a classification call runs: the product's flow plan (kaiju_amd/csrc/kj_flow.h: plan_flow, which launch_batch
executes and the emulation takes over), row by row against a table written by hand from the documented behaviour (README.md,
DESIGN.md 3, the layouts and switches of test_gpu_postsearch.py).  A row names only the fields it is about."""
import ctypes as C

import pytest

# the enums of kj_flow.h
OK, PROTEIN_PAIRED, PROTEIN_TOO_LONG, TOO_MANY_FRAG_SLOTS = range(4)
S1_PROTEIN, S1_OLD, S1_FAST, S1_FAST_TRIG, S1_LONG, S1_LONG_TRIG, S1_TEAM = range(7)
SEG_OFF, SEG_EAGER, SEG_LAZY = range(3)
MEM_V1, MEM_WIDE_V1, MEM2, MEM_WIDE2, GREEDY_V1, GREEDY2, GREEDY2_WIDE, GREEDY3 = range(8)
PLAIN, COUNTING, XORDER, VERBOSE = range(4)
IN_LANE, ROW_TAX, ROW_TAX_WIDE, TEAM, WIDE_WALK, FUSED = range(6)
DEFER, LAZY, X_ORDER, PROTEIN = 8, 4, 1, 2          # Params::flags (kj_core.h)

IX_FIELDS = ("blocks64", "kline", "kline_k", "kmer64", "kmer_k", "wide", "row_tax")
SW_FIELDS = ("mode", "m", "seed_length", "seg", "flags", "verbose", "verbose_v1", "mem_v1", "stage1_old", "stage1_lane", "lazy_seg",
             "fused_post", "exact_pass", "greedy2", "greedy3", "count_ops", "blocks_retry")
CALL_FIELDS = ("n", "paired", "max_read_len", "seq_bytes", "records16")
PLAN_FIELDS = ("status", "run", "stage1", "seg", "seg_apply", "lane", "inst", "inst_second", "mem_second", "flags_lane", "flags_second",
               "fused", "trigcheck", "mem_verbose", "locate", "exact_pass", "lca", "clear_out", "max_read_len", "max_pair", "pep_bytes",
               "n_frag_slots", "seg_cap", "max_frag", "si_cap_retry", "per_lane", "blocks_retry")

# a narrow index as the device builds it (k-mer lines of seven letters, the text arrays and with them the row -> taxon table) and
# a wide one (64-bit positions: a k-mer table, no lines)
NARROW = dict(blocks64=1, kline=1, kline_k=7, kmer64=0, kmer_k=5, wide=0, row_tax=1)
WIDE = dict(blocks64=1, kline=0, kline_k=0, kmer64=1, kmer_k=6, wide=1, row_tax=1)
# a context's defaults: MEM, m = 11, SEG; greedy2 = 2: as creation sets it (flow_greedy2)
SW = dict(mode=0, m=11, seed_length=7, seg=1, flags=0, verbose=0, verbose_v1=0, mem_v1=0, stage1_old=0, stage1_lane=0, lazy_seg=1,
          fused_post=1, exact_pass=1, greedy2=2, greedy3=0, count_ops=0, blocks_retry=16)
GREEDY = dict(SW, mode=1, blocks_retry=4)
# 1000 single-end reads of 150 nt, the 16-byte records wanted
CALL = dict(n=1000, paired=0, max_read_len=150, seq_bytes=150000, records16=1)

V1_MEM = dict(lane=MEM_V1, inst=PLAIN, flags_lane=0, flags_second=0, locate=IN_LANE, mem_verbose=0, fused=0, seg=SEG_EAGER, seg_apply=1)
V1_GREEDY = dict(lane=GREEDY_V1, inst=PLAIN, flags_lane=0, locate=IN_LANE, mem_verbose=0)

ROWS = [
    # ---- narrow, default switches, MEM, SEG, single-end
    ("default", NARROW, SW, CALL,
     dict(status=OK, run=1, stage1=S1_TEAM, seg=SEG_LAZY, seg_apply=0, lane=MEM2, inst=PLAIN, inst_second=PLAIN, mem_second=1,
          flags_lane=DEFER | LAZY, flags_second=DEFER, fused=1, trigcheck=0, mem_verbose=0, locate=FUSED, exact_pass=1, lca=0, clear_out=0)),
    ("default_184_byte_records_only", NARROW, SW, dict(CALL, records16=0), dict(fused=1, lca=0, clear_out=1)),
    ("paired", NARROW, SW, dict(CALL, paired=1, seq_bytes=300000), dict(stage1=S1_FAST, seg=SEG_LAZY, fused=1, max_pair=300)),
    ("stage1_lane", NARROW, dict(SW, stage1_lane=1), CALL, dict(stage1=S1_FAST, fused=1)),
    ("no_row_tax", dict(NARROW, row_tax=0), SW, CALL,
     dict(stage1=S1_TEAM, seg=SEG_LAZY, lane=MEM2, flags_lane=DEFER | LAZY, fused=0, trigcheck=1, locate=TEAM, mem_second=1, lca=1, clear_out=1)),
    ("wide_row_tax", WIDE, SW, CALL,
     dict(stage1=S1_TEAM, seg=SEG_LAZY, lane=MEM_WIDE2, inst=PLAIN, inst_second=PLAIN, mem_second=0, flags_lane=DEFER | LAZY, fused=0,
          trigcheck=1, locate=ROW_TAX_WIDE, lca=1)),
    ("wide_no_row_tax", dict(WIDE, row_tax=0), SW, CALL, dict(lane=MEM_WIDE2, fused=0, locate=WIDE_WALK, lca=1)),
    # ---- switches
    ("lazy_seg_off", NARROW, dict(SW, lazy_seg=0), CALL,
     dict(stage1=S1_FAST_TRIG, seg=SEG_EAGER, seg_apply=1, lane=MEM2, flags_lane=DEFER, fused=0, trigcheck=0, locate=ROW_TAX, lca=1, clear_out=1)),
    ("fused_post_off", NARROW, dict(SW, fused_post=0), CALL,
     dict(stage1=S1_TEAM, seg=SEG_LAZY, lane=MEM2, flags_lane=DEFER | LAZY, mem_second=1, fused=0, trigcheck=1, locate=ROW_TAX, lca=1, clear_out=1)),
    ("mem_lane_v1", NARROW, dict(SW, mem_v1=1), CALL, dict(V1_MEM, stage1=S1_FAST_TRIG, trigcheck=0, mem_second=0, lca=1)),
    ("mem_lane_v1_wide", WIDE, dict(SW, mem_v1=1), CALL, dict(V1_MEM, lane=MEM_WIDE_V1)),
    ("seg_off", NARROW, dict(SW, seg=0), CALL,
     dict(stage1=S1_TEAM, seg=SEG_OFF, seg_apply=0, lane=MEM2, flags_lane=DEFER, mem_second=0, fused=1, trigcheck=0, locate=FUSED,
          exact_pass=0, lca=0, seg_cap=1)),
    ("exact_pass_off", NARROW, dict(SW, exact_pass=0), CALL, dict(exact_pass=0, fused=1)),
    ("count_ops", NARROW, dict(SW, count_ops=1), CALL, dict(lane=MEM2, inst=COUNTING, inst_second=PLAIN, mem_second=1)),
    ("count_ops_wide", WIDE, dict(SW, count_ops=1), CALL, dict(lane=MEM_WIDE2, inst=COUNTING, inst_second=PLAIN, mem_second=0)),
    # ---- read length: short / long units of the fast stage 1, then the old one; m likewise
    ("mate_191", NARROW, SW, dict(CALL, max_read_len=191), dict(stage1=S1_TEAM, seg=SEG_LAZY, fused=1)),
    ("mate_192", NARROW, SW, dict(CALL, max_read_len=192), dict(stage1=S1_LONG, seg=SEG_LAZY, fused=1)),
    ("mate_191_trigger", NARROW, dict(SW, lazy_seg=0), dict(CALL, max_read_len=191), dict(stage1=S1_FAST_TRIG, seg=SEG_EAGER)),
    ("mate_192_trigger", NARROW, dict(SW, lazy_seg=0), dict(CALL, max_read_len=192), dict(stage1=S1_LONG_TRIG, seg=SEG_EAGER)),
    ("mate_287", NARROW, SW, dict(CALL, max_read_len=287), dict(stage1=S1_LONG, seg=SEG_LAZY, fused=1)),
    ("mate_288", NARROW, SW, dict(CALL, max_read_len=288),
     dict(stage1=S1_OLD, seg=SEG_EAGER, seg_apply=1, lane=MEM2, flags_lane=DEFER, fused=0, locate=ROW_TAX, lca=1)),
    ("stage1_old", NARROW, dict(SW, stage1_old=1), CALL, dict(stage1=S1_OLD, seg=SEG_EAGER, fused=0, locate=ROW_TAX)),
    ("max_read_len_0_is_1024", NARROW, SW, dict(CALL, max_read_len=0), dict(stage1=S1_OLD, max_read_len=1024, max_pair=1024)),
    ("m_64", NARROW, dict(SW, m=64), CALL, dict(stage1=S1_TEAM, seg=SEG_LAZY, fused=1)),
    ("m_65", NARROW, dict(SW, m=65), CALL, dict(stage1=S1_OLD, seg=SEG_EAGER, lane=MEM2, fused=0, locate=ROW_TAX)),
    # ---- k against m
    ("kline_k_eq_m", dict(NARROW, kline_k=11), SW, CALL, dict(lane=MEM2, seg=SEG_LAZY, fused=1)),
    ("kline_k_eq_m_plus_1", dict(NARROW, kline_k=12), SW, CALL, dict(V1_MEM, stage1=S1_FAST_TRIG)),
    ("kline_k_1", dict(NARROW, kline_k=1), SW, CALL, dict(V1_MEM)),
    ("kmer_k_eq_m_wide", dict(WIDE, kmer_k=11), SW, CALL, dict(lane=MEM_WIDE2, seg=SEG_LAZY)),
    ("kmer_k_eq_m_plus_1_wide", dict(WIDE, kmer_k=12), SW, CALL, dict(V1_MEM, lane=MEM_WIDE_V1)),
    ("no_lines", dict(NARROW, kline=0), SW, CALL, dict(V1_MEM)),
    # ---- -v
    ("verbose", NARROW, dict(SW, verbose=1), CALL,
     dict(stage1=S1_TEAM, seg=SEG_LAZY, lane=MEM2, inst=VERBOSE, inst_second=VERBOSE, mem_second=0, flags_lane=DEFER | LAZY, fused=0,
          trigcheck=1, mem_verbose=1, locate=ROW_TAX, lca=1)),
    ("verbose_wide", WIDE, dict(SW, verbose=1), CALL, dict(lane=MEM_WIDE2, inst=VERBOSE, mem_verbose=1, fused=0, locate=ROW_TAX_WIDE)),
    ("verbose_v1", NARROW, dict(SW, verbose=1, verbose_v1=1), CALL, dict(V1_MEM)),
    # (positions in 16 bits: max_read_len / 3 + 4 < 65536, and in MEM mode 2 * max_pair / (m + 1) + 8 < 65536)
    ("verbose_196595", NARROW, dict(SW, verbose=1), dict(CALL, max_read_len=196595), dict(lane=MEM2, inst=VERBOSE, mem_verbose=1, stage1=S1_OLD)),
    ("verbose_196596", NARROW, dict(SW, verbose=1), dict(CALL, max_read_len=196596), dict(V1_MEM)),
    ("verbose_paired_196583", NARROW, dict(SW, verbose=1), dict(CALL, paired=1, max_read_len=196583), dict(lane=MEM2, inst=VERBOSE, mem_verbose=1)),
    ("verbose_paired_196584", NARROW, dict(SW, verbose=1), dict(CALL, paired=1, max_read_len=196584), dict(V1_MEM)),
    ("plain_196596", NARROW, SW, dict(CALL, max_read_len=196596), dict(lane=MEM2, inst=PLAIN, locate=ROW_TAX)),
    ("greedy_verbose_196595", NARROW, dict(GREEDY, verbose=1), dict(CALL, max_read_len=196595), dict(lane=GREEDY2, inst=VERBOSE, mem_verbose=1)),
    ("greedy_verbose_196596", NARROW, dict(GREEDY, verbose=1), dict(CALL, max_read_len=196596), dict(V1_GREEDY)),
    ("greedy_verbose_paired_196584", NARROW, dict(GREEDY, verbose=1), dict(CALL, paired=1, max_read_len=196584), dict(lane=GREEDY2, inst=VERBOSE)),
    # ---- Greedy: never lazy, never fused, no k_seg_apply
    ("greedy", NARROW, GREEDY, CALL,
     dict(stage1=S1_FAST_TRIG, seg=SEG_EAGER, seg_apply=0, lane=GREEDY2, inst=PLAIN, flags_lane=DEFER, fused=0, trigcheck=0, mem_second=0,
          mem_verbose=0, locate=ROW_TAX, exact_pass=1, lca=1, clear_out=1, blocks_retry=4)),
    ("greedy_seg_off", NARROW, dict(GREEDY, seg=0), CALL, dict(stage1=S1_TEAM, seg=SEG_OFF, lane=GREEDY2, fused=0, exact_pass=0)),
    ("greedy_lazy_seg_switch_is_mem_only", NARROW, dict(GREEDY, lazy_seg=1), CALL, dict(seg=SEG_EAGER, stage1=S1_FAST_TRIG)),
    ("greedy_k_eq_seed", dict(NARROW, kline_k=7), dict(GREEDY, seed_length=7), CALL, dict(lane=GREEDY2)),
    ("greedy_k_eq_seed_plus_1", dict(NARROW, kline_k=8), dict(GREEDY, seed_length=7), CALL, dict(V1_GREEDY)),
    ("greedy_seed_3", dict(NARROW, kline_k=3), dict(GREEDY, seed_length=3), CALL, dict(lane=GREEDY2)),
    ("greedy_seed_2", dict(NARROW, kline_k=2), dict(GREEDY, seed_length=2), CALL, dict(V1_GREEDY)),
    ("greedy_k_1", dict(NARROW, kline_k=1), GREEDY, CALL, dict(V1_GREEDY)),
    ("greedy_lane_v1", NARROW, dict(GREEDY, greedy2=0), CALL, dict(V1_GREEDY, stage1=S1_FAST_TRIG, seg=SEG_EAGER)),
    ("greedy_no_row_tax", dict(NARROW, row_tax=0), GREEDY, CALL, dict(lane=GREEDY2, locate=TEAM)),
    ("greedy_wide", WIDE, GREEDY, CALL, dict(lane=GREEDY2_WIDE, inst=PLAIN, flags_lane=DEFER, locate=ROW_TAX_WIDE)),
    ("greedy_wide_no_row_tax", dict(WIDE, row_tax=0), GREEDY, CALL, dict(lane=GREEDY2_WIDE, locate=WIDE_WALK)),
    ("greedy_wide_k_eq_seed_plus_1", dict(WIDE, kmer_k=8), GREEDY, CALL, dict(V1_GREEDY)),
    ("greedy_wide_no_table", dict(WIDE, kmer64=0), GREEDY, CALL, dict(V1_GREEDY)),
    ("greedy_count_ops", NARROW, dict(GREEDY, count_ops=1), CALL, dict(lane=GREEDY2, inst=COUNTING)),
    ("greedy_wide_count_ops", WIDE, dict(GREEDY, count_ops=1), CALL, dict(lane=GREEDY2_WIDE, inst=COUNTING)),
    ("greedy_verbose", NARROW, dict(GREEDY, verbose=1, count_ops=1), CALL, dict(lane=GREEDY2, inst=VERBOSE, mem_verbose=1, locate=ROW_TAX)),
    ("greedy_verbose_v1", NARROW, dict(GREEDY, verbose=1, verbose_v1=1), CALL, dict(V1_GREEDY)),
    ("greedy_row_pool_lane", NARROW, dict(GREEDY, greedy3=1), CALL, dict(lane=GREEDY3, inst=PLAIN, flags_lane=DEFER, locate=ROW_TAX)),
    ("greedy_row_pool_lane_count_ops", NARROW, dict(GREEDY, greedy3=1, count_ops=1), CALL, dict(lane=GREEDY3, inst=COUNTING)),
    ("greedy_row_pool_lane_verbose", NARROW, dict(GREEDY, greedy3=1, verbose=1), CALL, dict(lane=GREEDY2, inst=VERBOSE)),
    # ---- protein reads
    ("protein", NARROW, dict(SW, flags=PROTEIN), dict(CALL, max_read_len=100, seq_bytes=100000),
     dict(status=OK, stage1=S1_PROTEIN, seg=SEG_EAGER, seg_apply=1, lane=MEM2, fused=0, locate=ROW_TAX, max_read_len=300, max_pair=300, max_frag=100)),
    ("protein_seg_off", NARROW, dict(SW, flags=PROTEIN, seg=0), dict(CALL, max_read_len=100), dict(stage1=S1_PROTEIN, seg=SEG_OFF, fused=1)),
    ("protein_greedy", NARROW, dict(GREEDY, flags=PROTEIN), dict(CALL, max_read_len=100), dict(stage1=S1_PROTEIN, lane=GREEDY2, max_frag=100)),
    ("protein_paired", NARROW, dict(SW, flags=PROTEIN), dict(CALL, paired=1), dict(status=PROTEIN_PAIRED)),
    ("protein_2_28", NARROW, dict(SW, flags=PROTEIN), dict(CALL, max_read_len=1 << 28), dict(status=OK, max_read_len=3 << 28, max_frag=1 << 28)),
    ("protein_over_2_28", NARROW, dict(SW, flags=PROTEIN), dict(CALL, max_read_len=(1 << 28) + 1), dict(status=PROTEIN_TOO_LONG)),
    # ---- other
    ("kaijux", NARROW, dict(SW, flags=X_ORDER), CALL,
     dict(lane=MEM2, inst=XORDER, inst_second=XORDER, mem_second=0, seg=SEG_LAZY, fused=1, locate=FUSED)),
    ("kaijux_wide", WIDE, dict(SW, flags=X_ORDER), CALL, dict(lane=MEM_WIDE2, inst=XORDER, inst_second=XORDER, mem_second=0)),
    ("kaijux_count_ops", NARROW, dict(SW, flags=X_ORDER, count_ops=1), CALL, dict(inst=COUNTING, inst_second=XORDER, mem_second=0)),
    ("n_0", NARROW, SW, dict(CALL, n=0, seq_bytes=0), dict(status=OK, run=0, fused=0, exact_pass=0, lca=0, clear_out=0)),
    ("n_0_greedy", NARROW, GREEDY, dict(CALL, n=0, seq_bytes=0), dict(status=OK, run=0, exact_pass=0, lca=0, clear_out=0)),
    # 2 * (2 * seq_bytes / (m + 1) + 7 n) + 8 fragment slots must stay below 2^32 - 1
    ("frag_slots_below_limit", NARROW, SW, dict(CALL, n=1, seq_bytes=6 * 2147483636), dict(status=OK, n_frag_slots=(1 << 32) - 2)),
    ("frag_slots_at_limit", NARROW, SW, dict(CALL, n=1, seq_bytes=6 * 2147483637), dict(status=TOO_MANY_FRAG_SLOTS)),
    # ---- the sizes that launch_batch and kaiju_gpu_seg_regions share
    ("sizes", NARROW, SW, CALL,
     dict(max_read_len=150, max_pair=150, pep_bytes=2 * 150000 + 208 * 1000 + 288, n_frag_slots=2 * (300000 // 12 + 7000) + 8, seg_cap=32012,
          max_frag=52, si_cap_retry=364, per_lane=320, blocks_retry=16)),
    ("sizes_paired", NARROW, SW, dict(CALL, paired=1, seq_bytes=300000), dict(max_pair=300, si_cap_retry=664, per_lane=624, max_frag=52)),
    # (LDS staging of the old stage 1: 64 lanes * per_lane <= 60000 bytes; the retry pass's scratch: halved down to 1 GB)
    ("sizes_per_lane_last", NARROW, SW, dict(CALL, max_read_len=454), dict(per_lane=928)),
    ("sizes_per_lane_in_place", NARROW, SW, dict(CALL, max_read_len=462), dict(per_lane=0)),
    ("sizes_retry_blocks_halved", NARROW, SW, dict(CALL, max_read_len=20000), dict(si_cap_retry=40064, blocks_retry=4)),
    ("sizes_retry_blocks_one", NARROW, SW, dict(CALL, max_read_len=196596), dict(si_cap_retry=393256, blocks_retry=1, per_lane=0)),
    ("sizes_si_cap_retry_capped", NARROW, SW, dict(CALL, max_read_len=1 << 24), dict(si_cap_retry=1 << 24, blocks_retry=1)),
    ("sizes_greedy_retry_blocks_kept", NARROW, GREEDY, dict(CALL, max_read_len=196596), dict(blocks_retry=4)),
    ("sizes_seg_cap_capped", NARROW, SW, dict(CALL, n=1, seq_bytes=6 * 100000000), dict(seg_cap=0x00ffffff)),
]


@pytest.fixture(scope="module")
def flow_plan(emu):
    lib = emu.lib
    lib.emu_flow_plan.restype = None
    lib.emu_flow_plan.argtypes = [C.POINTER(C.c_uint64)] * 4

    def plan(ix, sw, call):
        a = (C.c_uint64 * len(IX_FIELDS))(*[ix[k] for k in IX_FIELDS])
        b = (C.c_uint64 * len(SW_FIELDS))(*[sw[k] for k in SW_FIELDS])
        c = (C.c_uint64 * len(CALL_FIELDS))(*[call[k] for k in CALL_FIELDS])
        out = (C.c_uint64 * len(PLAN_FIELDS))()
        lib.emu_flow_plan(a, b, c, out)
        return dict(zip(PLAN_FIELDS, [int(x) for x in out]))
    return plan


@pytest.mark.parametrize("name,ix,sw,call,want", ROWS, ids=[r[0] for r in ROWS])
def test_flow_plan(flow_plan, name, ix, sw, call, want):
    got = flow_plan(ix, sw, call)
    assert {k: got[k] for k in want} == want


def test_row_names_are_unique():
    assert len({r[0] for r in ROWS}) == len(ROWS)
