"""Pairs of calls for the tests of call history (test_call_history_emu.py on the host, test_gpu_call_history.py on the device):
a call A that leaves residue in a context's buffers (or in the caller's) and a call B whose records must not depend on it.

Every case names the buffer it dirties.  The expectation of B is always the oracle's and B's own result on fresh memory.
Two worlds: 'golden' (tests/golden: db.fmi and its reads, util.long_reads, util.many_region_reads) and 'motif' (the planted
motifs of postsearch_inputs.py, whose reads are known to enter the lazy-SEG listing, the second search, the retry pass and the
many-rows locate).

The continuation cases put stale letters directly behind the LAST frame string of B's last read, where B's stage 1 writes
nothing.  The fast stage 1 (kj_core.h: s1_mate) stores six strings of u = len / 48 + 1 units of 16 bytes per mate, the three
reverse strings right-aligned: the last one ends exactly at byte 96 * u of the mate's area.  B's last read is two
nucleotides and the reverse complement of a back-translated stretch of a database protein, so its match ends at that byte.
  'mate': A is B with a second mate for its last read, the back-translation of the residues that follow in the protein: the
          mate's first string starts at byte 96 * u.  B is A without its last mate.
  'read': single reads (the team kernel).  The area of read r is 2 * len + 208 bytes and the next read starts behind it, at
          least 112 bytes behind the strings of a single read: no other read of A reaches it (two mates of 144 nt leave 16
          bytes, still no direct neighbour).  So A keeps n and swaps the last read for a longer one: B's has u = 1, A's u = 3,
          whose forward string of frame 2 starts at byte 96 - A's read is two nucleotides and the residues that follow.
The general stage 1 (build_fragments) closes every string with a stop of its own and copies whole 16-byte words out of its
staging area: there the stale letters lie behind that stop, within the 64 bytes a window loads, never directly behind.
continuation_armed() proves all this on the memory B's lanes see: the emulation's peptide area carried over from A to B."""
from __future__ import annotations

import functools
import os

import numpy as np

import postsearch_inputs as P
import util

COMP = bytes.maketrans(b"ACGT", b"TGCA")
STAGE1 = {0: "Protein", 1: "Old", 2: "Fast", 3: "FastTrig", 4: "Long", 5: "LongTrig", 6: "Team"}     # kj_flow.h: FlowStage1


class Env:
    """environment variables set for a block (the switches a context or an index reads when it is created)"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def specified_equal(a, b):
    """best, n_ids, flags and the announced ids of every record: what include/kaiju_gpu.h specifies where the hit records are
    not cleared (the id slots behind n_ids are the caller's memory as it stood)"""
    if len(a) != len(b) or not all((a[f] == b[f]).all() for f in ("best", "n_ids", "flags")):
        return False
    k = np.arange(21)[None, :] < a["n_ids"][:, None]
    return bool((np.where(k, a["taxid"], 0) == np.where(k, b["taxid"], 0)).all())


class Call:
    """one classification call: a batch in the layout of include/kaiju_gpu.h and the read-length bound its context is told"""

    def __init__(self, name, reads1, reads2=None, max_len=None, too_long=()):
        self.name, self.reads1, self.reads2 = name, list(reads1), None if reads2 is None else list(reads2)
        self.seqs, self.off = util.pack(self.reads1, self.reads2)
        self.paired = reads2 is not None
        self.n = len(self.reads1)
        longest = max([1] + [len(x) for x in self.reads1 if x is not None] + [len(x) for x in (self.reads2 or [])])
        self.max_len = max_len or longest          # kaiju_gpu_set_max_read_length of the device-resident entry points
        # reads with a mate longer than max_len: kErrReadTooLong (error flag 16), the read gets an empty record
        self.too_long = tuple(too_long)
        assert all(len(self.reads1[i]) > self.max_len or (self.reads2 and len(self.reads2[i]) > self.max_len) for i in self.too_long)
        assert longest <= self.max_len or self.too_long

    def oracle_batch(self):
        """what the oracle is asked: the batch with the over-long reads emptied"""
        if not self.too_long:
            return self.seqs, self.off
        r1 = [b"" if i in self.too_long else x for i, x in enumerate(self.reads1)]
        r2 = None if self.reads2 is None else [b"" if i in self.too_long else x for i, x in enumerate(self.reads2)]
        return util.pack(r1, r2)


class Case:
    """calls: run in this order on ONE context; the last one is the victim, the others leave the residue.  chain: the calls
    are also run back and forth on one context, and the first again at the end.  dirties: the buffers the case is about"""

    def __init__(self, name, world, calls, dirties, m=11, modes=("mem", "greedy"), segs=(1, 0), protein=False, chain=False, device=True, host=True):
        self.name, self.world, self.calls, self.dirties, self.m = name, world, calls, dirties, m
        self.modes, self.segs, self.protein, self.chain, self.device, self.host = modes, segs, protein, chain, device, host

    @property
    def victim(self):
        return self.calls[-1]

    def __repr__(self):
        return self.name


def rc(s: bytes):
    return s[::-1].translate(COMP)


def nt(pep: str):
    return "".join(util.BACK[c] for c in pep).encode()


@functools.lru_cache(maxsize=None)
def golden_proteins():
    with open(os.path.join(util.GOLD, "db.faa")) as f:
        return [line.strip() for line in f if not line.startswith(">")]


def nothing_reads(n, m=11, seed=41):
    """reads that can have no record: empty, shorter than 3 * m, only N, no hit (random: a chance match of m residues in a
    database of 80 000 has a probability below 1e-8 a position)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = i % 4
        if k == 0:
            out.append(b"")
        elif k == 1:
            out.append(bytes(rng.choice(list(b"ACGT"), 3 * m - 1 - i % 7).astype(np.uint8)))
        elif k == 2:
            out.append(b"N" * (100 + i % 50))
        else:
            out.append(bytes(rng.choice(list(b"ACGT"), 150).astype(np.uint8)))
    return out


def interleave(a, b):
    """a[0], b[1], a[2], b[3], ...: both kinds share every wavefront"""
    return [(a if i % 2 == 0 else b)[i] for i in range(min(len(a), len(b)))]


def continuation(name, q, e, kind, n_front=5, a=10):
    """see the module's docstring; n_front golden reads in front (with 30-nt mates, no fragment, in the 'mate' kind)"""
    g = util.Golden()
    prot = max(golden_proteins(), key=len)
    match, follows = prot[a: a + q], prot[a + q: a + q + e]
    front = [r for r in g.reads if 100 <= len(r) <= 150][:n_front]
    last_b = b"GC" + rc(nt(match))
    if kind == "mate":
        mates = [x[:30] for x in front]
        calls = [Call("with mate", front + [last_b], mates + [nt(follows)]), Call("without", front + [last_b], mates + [b""])]
    else:
        calls = [Call("longer", front + [b"GC" + nt(follows)]), Call("short", front + [last_b])]
    c = Case(name, "golden", calls, "peptide area behind the last frame string")
    c.match, c.follows = match, follows
    return c


def continuation_armed(emu, h, case, mode, seg, want_stage1):
    """A, then B on the peptide area as A left it (everything else a pattern).  Asserts that both took stage 1 `want_stage1`
    and that the case is armed AFTER B's stage 1 and search: the bytes directly behind the fragment that ends B's match are
    stale residue codes equal to the database text that follows the match (the general stage 1: behind the stop it writes,
    a run of at least eight of them within a window's 64 bytes).  Returns B's records of that run"""
    import ctypes as C
    emu.lib.emu_alphabet.restype = C.c_char_p
    emu.lib.emu_alphabet.argtypes = [C.c_void_p]
    alpha = emu.lib.emu_alphabet(h).decode()
    A, B = case.calls
    try:
        emu.set_fill(b"\xee")
        emu.set_carry(False)
        emu.classify(h, util.gp(mode, m=case.m, seg=seg), A.seqs, A.off, paired=A.paired)
        assert STAGE1[emu.lib.emu_last_stage1()] == want_stage1, (case.name, STAGE1[emu.lib.emu_last_stage1()])
        emu.set_carry(True)
        got, _ = emu.classify(h, util.gp(mode, m=case.m, seg=seg), B.seqs, B.off, paired=B.paired)
        assert STAGE1[emu.lib.emu_last_stage1()] == want_stage1, (case.name, STAGE1[emu.lib.emu_last_stage1()])
    finally:
        emu.set_carry(False)
        emu.set_fill(b"")
    pep = emu.pep_read(0, 1 << 24)
    base, frags = emu.frags_read(B.n - 1)
    ends = [base + s + ln for s, ln in frags if "".join(alpha[c] if c < 21 else "?" for c in pep[base + s: base + s + ln]).endswith(case.match)]
    assert len(ends) == 1, (case.name, frags)
    behind = "".join(alpha[c] if c < 21 else "?" for c in pep[ends[0]: ends[0] + 64])
    if want_stage1 != "Old":
        assert behind.startswith(case.follows) and "*" not in case.follows, (case.name, behind)
    else:
        runs = [k for k in range(len(case.follows) - 7) if case.follows[k: k + 8] in behind]
        assert behind[0] == "*" and runs, (case.name, behind)
    return got


# (name, residues of B's match, residues that follow in A, kind, mode, seg, the stage 1 both calls must take, environment)
CONTINUATION = (("continuation_team", 14, 32, "read", "mem", 1, "Team", {}),
                ("continuation_team_noseg", 14, 32, "read", "mem", 0, "Team", {}),
                ("continuation_fast", 40, 20, "mate", "mem", 1, "Fast", {}),
                ("continuation_fasttrig", 40, 20, "mate", "greedy", 1, "FastTrig", {}),
                ("continuation_long", 70, 20, "mate", "mem", 1, "Long", {}),
                ("continuation_longtrig", 70, 20, "mate", "greedy", 1, "LongTrig", {}),
                ("continuation_old", 100, 30, "mate", "mem", 1, "Old", {}),
                ("continuation_old_short", 40, 20, "mate", "greedy", 1, "Old", {"KAIJU_EMU_STAGE1_OLD": "1", "KAIJU_GPU_STAGE1": "old"}))


@functools.lru_cache(maxsize=None)
def golden_cases():
    g = util.Golden()
    short = [r for r in g.reads if len(r) <= 150]                 # 666 reads of 100 and 150 nt: the fast stage 1, lazy SEG
    mid = [r for r in g.reads if 191 < len(r) <= 287]             # 250 nt: the instantiation with six units a frame string
    _, many_nt = util.many_region_reads()                         # 12 reads for the exact pass (more than 15 SEG regions a fragment)
    many_p, _ = util.many_region_reads()
    longs = util.long_reads(n=60)
    out = []
    # every slot of the hit buffer holds a valid record - of its neighbour
    out.append(Case("records_rotated", "golden", [Call("rotated", short[1:] + short[:1]), Call("golden", short)], "hit records"))
    out.append(Case("records_rotated_pairs", "golden", [Call("rotated", g.p1[1:] + g.p1[:1], g.p2[1:] + g.p2[:1]), Call("pairs", g.p1, g.p2)], "hit records"))
    # records with as many ids as there are under reads that can have no record
    nothing = interleave(short, nothing_reads(len(short)))
    out.append(Case("records_on_nothing", "golden", [Call("golden", short), Call("nothing", nothing)], "hit records, fragment lists"))
    over = list(nothing)
    over[3] = short[3] + short[4]                                 # 300 nt under a bound of 150
    out.append(Case("records_on_nothing_too_long", "golden", [Call("golden", short), Call("nothing+long", over, max_len=150, too_long=(3,))],
                    "hit records, fragment lists", host=False))
    # the exact pass (and the general stage 1, the eager SEG pass) under plain reads, and back
    exact = [many_nt[i // 8 % len(many_nt)] if i % 8 == 5 else short[i] for i in range(96)]
    out.append(Case("routes_exact", "golden", [Call("exact", exact), Call("plain", short[:96])], "redo bitmap and lists, SegRecs, region pool", chain=True))
    # n_A > n_B: the exact-pass reads of A behind B's end; n_B = 333 is no multiple of 32, 64 or 256
    nb = 333
    big = short[:nb] + [many_nt[i % len(many_nt)] if i % 3 == 0 else short[nb + i] for i in range(90)]
    out.append(Case("shrink", "golden", [Call("large", big), Call("small", short[:nb])], "every list and bitmap behind n_B"))
    out.append(Case("shrink_by_one", "golden", [Call("large", short[:nb] + [many_nt[0]]), Call("small", short[:nb])], "the word of read n_B"))
    out.append(Case("shrink_empty_between", "golden", [Call("large", big), Call("empty", []), Call("small", short[:nb])], "every list and bitmap behind n_B"))
    # who writes the peptide area, and how
    ns = len(g.p1)
    out.append(Case("layout_paired_single", "golden", [Call("pairs", g.p1, g.p2), Call("single", short[:ns])], "peptide area, fragment lists", chain=True))
    out.append(Case("layout_long_short", "golden", [Call("long", longs), Call("short", short[:len(longs)])], "peptide area, staging", chain=True))
    out.append(Case("layout_mid_short", "golden", [Call("mid", mid + short[:24]), Call("short", short[100: 100 + len(mid) + 24])], "peptide area", chain=True))
    out.append(Case("layout_max_read_length", "golden", [Call("bound1024", short[:200], max_len=1024), Call("bound150", short[:200])],
                    "per_lane, si_cap_retry, scratch sizes", chain=True, host=False))
    out.append(Case("layout_protein", "golden", [Call("long proteins", many_p), Call("proteins", g.prot_reads[:len(many_p)])],
                    "peptide area", protein=True, chain=True))
    for name, q, e, kind, mode, seg, _, _ in CONTINUATION:
        c = continuation(name, q, e, kind)
        c.modes, c.segs = (mode,), (seg,)                         # (the configuration that takes the case's stage 1)
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def motif_cases():
    """m = 8 (the short pairs and singles: the fast stage 1, lazy SEG) and m = 11 (the long reads of sets 1 and 2)"""
    I = P.inputs()
    enc = lambda reads: ([r.nt1.encode() for r in reads], [r.nt2.encode() for r in reads] if any(r.nt2 for r in reads) else None)
    out = []
    # pairs: every rung of set 3 but the plain ones is a side route - a lazy-SEG listing ('lc', 'multi', more than 16 matches:
    # kWinForce), the second search behind it, the retry pass (more than 16 matches), more than kLocDeferRows rows ('pairrows')
    pairs = I.kept["pairs"]
    side = [r for r in pairs if r.rung[0] in ("lc", "multi", "pairrows") or r.k > 2]
    plain = [r for r in pairs if r.rung[0] == "pair" and r.k <= 2]
    plain = [plain[i % len(plain)] for i in range(len(side))]
    out.append(Case("routes_pairs", "motif", [Call("side", *enc(side)), Call("plain", *enc(plain))], "hit records, seglist, retry list, loc list",
                    m=8, modes=("mem",), chain=True))
    single = I.kept["short"]
    s_side = [r for r in single if r.rung[0] == "force"]
    s_plain = [r for r in single if r.rung[0] == "single"]
    s_plain = [s_plain[i % len(s_plain)] for i in range(len(s_side))]
    out.append(Case("routes_single", "motif", [Call("forced", *enc(s_side)), Call("plain", *enc(s_plain))], "hit records, seglist, retry list",
                    m=8, modes=("mem",), chain=True))
    # long reads: three to sixteen matches or more than eight rows (the list of k_mem_locate / k_mem_post1), the retry pass
    rows = [r for r in I.kept["rows"] + I.kept["ladder"] if P.list_bound(r) or r.k > 16]
    fill = I.kept["fill"][:len(rows)]
    out.append(Case("routes_rows", "motif", [Call("listed", *enc(rows)), Call("plain", *enc(fill))], "hit records, loc list, retry list", chain=True))
    greedy = I.kept["greedy"]
    out.append(Case("routes_greedy", "motif", [Call("many best", *enc([r for r in greedy if r.k >= 12])), Call("few", *enc([r for r in greedy if r.k <= 2] * 4))],
                    "hit records, match scratch", modes=("greedy",), chain=True))
    return out


def by_name(cases):
    return {c.name: c for c in cases}
