"""Inputs of the post-search tests (test_postsearch_emu.py on the host, test_gpu_postsearch.py on the device), built from seeds:
one tiny database of planted motifs, its taxonomy, the read sets that put a read on either side of every threshold between
a finished search and a finished record (kj_core.h: mem_lane2's BK_LOC_INIT, mem_locate_read, mem_locate_read_team; capi.hip:
k_mem_post1 / _post2, k_mem_locate*, the lazy-SEG hand-off, the retry pass) - and a census of every read that knows nothing of
that code: six-frame translation, the k-mers of the fragments looked up in the set of the database's k-mers.

A motif of 12 residues (8 for the short pairs) lies in c sequences; the residue in front of and behind every copy is never a
spacer letter (W, C), the reads put nothing but spacers, stops and read ends next to a motif: no match extends past a motif,
every occurrence is one longest match of c rows."""
from __future__ import annotations

import functools
import os

import numpy as np

import util

AA = "ACDEFGHIKLMNPQRSTVWY"
SPACER = "WC"                                   # the letters of the reads' spacers; no copy's flank is one of them
FLANK = [c for c in AA if c not in SPACER]
DIAG = dict(zip("ARNDCQEGHILKMFPSTWYV", (4, 5, 6, 6, 9, 5, 5, 6, 8, 4, 4, 5, 5, 6, 7, 4, 5, 11, 7, 4)))   # BLOSUM62's diagonal
COPIES = (1, 2, 3, 4, 5, 7, 8, 9, 10, 16, 20, 24, 40)
MISSING = (900001, 900002, 900003, 900004)      # taxon ids that nodes.dmp does not have
UNITS = ("DEGHIKLMN", "PQRSTVYDE")               # the periods of the periodic reads: nine different letters, neither A nor F
SEED = 20240611
COMP = str.maketrans("ACGT", "TGCA")

_B = "TCAG"
CODON = {a + b + c: aa for (a, b, c), aa in zip(((a, b, c) for a in _B for b in _B for c in _B),
                                                "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG")}


def translate(nt: str):
    return "".join(CODON.get(nt[i: i + 3], "X") for i in range(0, len(nt) - 2, 3))


def six_frames(nt: str):
    rc = nt[::-1].translate(COMP)
    return [translate(s[f:]) for s in (nt, rc) for f in (0, 1, 2)]


def fragments(nt: str):
    """the stretches of amino acids between the stops (and letters that are none) of the six frame strings"""
    out = []
    for fs in six_frames(nt):
        for piece in fs.replace("X", "*").split("*"):
            if piece:
                out.append(piece)
    return out


def back(pep: str):
    """the fixed codon table of the suite (util.BACK); '*' = a stop"""
    return "".join("TAA" if c == "*" else util.BACK[c] for c in pep)


# ---------------------------------------------------------------------------------------------------------------------------
# the database
# ---------------------------------------------------------------------------------------------------------------------------
class Motif:
    def __init__(self, name, seq, taxa):
        self.name, self.seq, self.taxa = name, seq, list(taxa)      # taxa: one entry per copy

    @property
    def copies(self):
        return len(self.taxa)


def _rand(rng, n, letters=AA):
    return "".join(letters[int(i)] for i in rng.integers(0, len(letters), size=n))


def _motif(rng, n, min_score, seen):
    """n random residues, at least 8 different ones in 12 (nothing SEG would flag), a BLOSUM62 score of its own of at least
    min_score (Greedy's default -s 65 lets every 12-residue motif through)"""
    while True:
        s = _rand(rng, n)
        if len(set(s)) >= min(8, n - 2) and sum(DIAG[c] for c in s) >= min_score and s not in seen:
            seen.add(s)
            return s


def taxonomy():
    """four families of four genera of four species: the LCA of a motif's taxa is a species, a genus, a family or the root"""
    from kaiju_amd import synth
    return synth.make_taxonomy(4, 4, 4)


def _leaf(leaves, f, g, s):
    return int(leaves[(f % 4) * 16 + (g % 4) * 4 + s % 4])


def _taxa_sets(leaves, c, k):
    """variant -> the taxa of the c copies of the k-th copy count"""
    out = {"one": [_leaf(leaves, k, k // 4, k // 2)]}
    if c >= 2:
        nt = min(c, 5)
        if nt <= 4 and k % 3 == 0:
            few = [_leaf(leaves, k, k + 1, s) for s in range(nt)]                    # one genus
        elif k % 3 == 1:
            few = [_leaf(leaves, k, q, q + k) for q in range(4)] + [_leaf(leaves, k, 0, k + 1)]   # one family
            few = few[:nt]
        else:
            few = [_leaf(leaves, q, k + q, k) for q in range(4)] + [_leaf(leaves, 1, k + 2, k + 1)]   # several families
            few = few[:nt]
        out["five" if c >= 24 else "few"] = few
    if c >= 16:
        out["many"] = [int(leaves[(5 * k + 3 * q) % 64]) for q in range(c)]           # c different species (3 and 64 are coprime)
    return {v: [t[j % len(t)] for j in range(c)] for v, t in out.items()}


class Inputs:
    pass


def build_db(seed=SEED):
    rng = np.random.default_rng(seed)
    lines, leaves = taxonomy()
    seen = set()
    motifs = {}

    def add(name, seq, taxa):
        motifs[name] = Motif(name, seq, taxa)

    # single copies under species of their own (26 of them: 21 and 22 ids in one read)
    for i in range(26):
        add(f"s{i}", _motif(rng, 12, 66, seen), [int(leaves[(7 * i) % 64])])
    for k, c in enumerate(COPIES[1:], start=1):
        for v, taxa in _taxa_sets(leaves, c, k).items():
            add(f"c{c}{v}", _motif(rng, 12, 66, seen), taxa)
    # five species that c16many does not have: 21 ids in a record without the cap's flag
    add("c5far", _motif(rng, 12, 66, seen), [int(t) for t in leaves if int(t) not in motifs["c16many"].taxa][:5])
    # taxon ids that nodes.dmp does not have: alone, next to a known one, two of them
    add("x1", _motif(rng, 12, 66, seen), [MISSING[0]])
    add("x2", _motif(rng, 12, 66, seen), [MISSING[1], _leaf(leaves, 2, 1, 3)])
    add("x3", _motif(rng, 12, 66, seen), [MISSING[2], MISSING[3]])
    # Greedy: equal scores come from one motif repeated
    for i in range(4):
        add(f"g1_{i}", _motif(rng, 12, 70, seen), [_leaf(leaves, i, i + 1, i + 2)])
        add(f"g9_{i}", _motif(rng, 12, 70, seen), [_leaf(leaves, i, q % 3, q) for q in range(9)])
    # the second set: 8 residues, for the short pairs
    for i in range(24):
        add(f"h{i}", _motif(rng, 8, 0, seen), [int(leaves[(11 * i + 5) % 64])])
    for i in range(3):
        add(f"h2_{i}", _motif(rng, 8, 0, seen), [_leaf(leaves, i, 2, 0), _leaf(leaves, i, 2, 1 + i)])
        add(f"h3_{i}", _motif(rng, 8, 0, seen), [_leaf(leaves, i, 0, 0), _leaf(leaves, i, 1, 0), _leaf(leaves, i + 1, 0, 0)])
    add("h9", _motif(rng, 8, 0, seen), [_leaf(leaves, 3, q % 3, q) for q in range(9)])
    # the nine 8-residue windows of a string of period nine, each in a sequence of its own (the flanks of a first copy are A
    # and F: no window extends): a periodic read is ONE fragment with a longest match at every position - the only way to more
    # than 16 matches without a second fragment.  (A pair's matches lie in two fragments at least, kWinMulti: such a pair is
    # listed for SEG if ANY of its fragments trips the trigger, and the shifted frames of a back-translation nearly always do.)
    for u, unit in enumerate(UNITS):
        for i in range(9):
            add(f"p{u}_{i}", (unit * 2)[i: i + 8], [_leaf(leaves, u + 2, i, i // 4)])
    # low-complexity motifs: a read holds them in the middle of a run of their main letter, SEG cuts them out
    add("lcq", "QAQQAQQA", [_leaf(leaves, 0, 3, 3)])
    add("lcs", "SGSSGSGS", [_leaf(leaves, 2, 3, 3)])
    seqs = []                                     # (name, taxon, residues)
    for m in motifs.values():
        lc = m.name.startswith("lc")
        for j, tax in enumerate(m.taxa):
            a, b = int(rng.integers(21, 54)), int(rng.integers(21, 54))
            lf = "L" if lc else FLANK[j % 18]
            rf = "K" if lc else FLANK[(7 * j + 3) % 18]
            seqs.append((f"{m.name}n{j}", tax, _rand(rng, a) + lf + m.seq + rf + _rand(rng, b)))
    while len(seqs) % 8 == 0 or len(seqs) < 500:  # (nseq % 8 == 0 is the reference's short sample array: no row -> taxon table)
        seqs.append((f"r{len(seqs)}", int(leaves[len(seqs) % 64]), _rand(rng, int(rng.integers(50, 121)))))
    order = rng.permutation(len(seqs))            # copies of a motif do not stand next to each other
    return lines, leaves, motifs, [seqs[int(i)] for i in order]


# ---------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------
class Census:
    """how often every k-mer (and whether a (k+1)-mer) occurs in the database: set lookups, nothing else"""

    def __init__(self, seqs):
        self.count = {8: {}, 12: {}}
        self.longer = {8: set(), 12: set()}
        for _, _, s in seqs:
            for k in (8, 12):
                cnt = self.count[k]
                for i in range(len(s) - k + 1):
                    w = s[i: i + k]
                    cnt[w] = cnt.get(w, 0) + 1
                lg = self.longer[k]
                for i in range(len(s) - k):
                    lg.add(s[i: i + k + 1])

    def read(self, k, *mates):
        """(longest matches, their rows, a (k+1)-mer matched) of a read or pair whose longest matches should have k residues"""
        cnt, lg = self.count[k], self.longer[k]
        n = rows = 0
        ext = False
        for nt in mates:
            for fr in fragments(nt):
                for i in range(len(fr) - k + 1):
                    c = cnt.get(fr[i: i + k])
                    if c:
                        n += 1
                        rows += c
                for i in range(len(fr) - k):
                    ext = ext or fr[i: i + k + 1] in lg
        return n, rows, ext


# ---------------------------------------------------------------------------------------------------------------------------
# the reads
# ---------------------------------------------------------------------------------------------------------------------------
class Read:
    __slots__ = ("name", "rung", "nt1", "nt2", "k", "rows", "mlen")

    def __init__(self, name, rung, nt1, nt2, k, rows, mlen):
        self.name, self.rung, self.nt1, self.nt2, self.k, self.rows, self.mlen = name, rung, nt1, nt2, k, rows, mlen


class Builder:
    def __init__(self, motifs, seed):
        self.m, self.rng, self.n = motifs, np.random.default_rng(seed), 0
        self.reads = []

    def spacer(self, n=None):
        n = int(self.rng.integers(1, 4)) if n is None else n
        return _rand(self.rng, n, SPACER)

    def join(self, names, stops=(), one_spacer=False):
        """the motifs `names` in a row, a spacer behind each (stops: positions behind which a stop follows the spacer)"""
        pep = ""
        for i, nm in enumerate(names):
            pep += self.m[nm].seq + self.spacer(1 if one_spacer else None)
            if i in stops:
                pep += "*"
        return pep

    def nt(self, pep, pad_to=0):
        """back-translated, padded behind a stop with random residues to at least pad_to nucleotides, a frame shift of 0 - 2
        nucleotides in front, every second read on the other strand"""
        if pad_to and 3 * len(pep) + 5 < pad_to:
            pep += "*" + _rand(self.rng, (pad_to - 3 * len(pep)) // 3 + 1)
        s = "ACGT"[: self.n % 3] + back(pep)
        if self.n % 2:
            s = s[::-1].translate(COMP)
        return s

    def add(self, rung, pep1, pep2=None, k=0, rows=0, mlen=12, pad_to=0):
        nt1 = self.nt(pep1, pad_to)
        nt2 = self.nt(pep2, pad_to) if pep2 is not None else ""
        self.reads.append(Read(f"{'.'.join(str(x) for x in rung)}#{self.n}", rung, nt1, nt2, k, rows, mlen))
        self.n += 1

    def rows_of(self, names):
        return sum(self.m[n].copies for n in names)


LONG = 300                                       # sets 1, 2, 5: longer than 287 nt - the general stage 1, SEG eagerly


def ladder_reads(motifs, seed=SEED + 1):
    """set 1: k motif occurrences, k = 1 .. 18, 21, 22, in one fragment and spread over fragments by stops"""
    b = Builder(motifs, seed)
    pool = [f"s{i}" for i in range(26)] + ["c2one", "c2few", "c3one", "c3few", "x1", "x2"]
    singles = [f"s{i}" for i in range(26)]
    for k in list(range(1, 19)) + [21, 22]:
        for q in range(4):
            names = singles[q: q + k] if q == 0 else [pool[int(i)] for i in b.rng.integers(0, len(pool), size=k)]
            b.add(("k", k, "one"), b.join(names), k=k, rows=b.rows_of(names), pad_to=LONG)
            stops = set(range(k - 1)) if q < 2 else set(range(2, k - 1, 3)) | {0}
            if k == 1:
                stops = {0}
            b.add(("k", k, "spread"), b.join(names, stops), k=k, rows=b.rows_of(names), pad_to=LONG)
    return b.reads


ROW_RUNGS = {1: [("s0",), ("x1",)], 2: [("c2one",), ("c2few",), ("s1", "s2"), ("x3",), ("x2",)],
             7: [("c7one",), ("c7few",), ("c3few", "c4few"), ("c5few", "c2few"), ("c5one", "c2one")],
             8: [("c8one",), ("c8few",), ("c4few", "c4one"), ("c7few", "s3"), ("c4one", "c4one")],
             9: [("c9one",), ("c9few",), ("c4few", "c5few"), ("c8few", "s4"), ("c5one", "c4one")],
             10: [("c10one",), ("c10few",), ("c5few", "c5one"), ("c9few", "s5"), ("c9one", "x1")],
             16: [("c16one",), ("c16few",), ("c16many",), ("c8few", "c8one"), ("c9few", "c7few")],
             40: [("c40one",), ("c40five",), ("c40many",), ("c20few", "c20one"), ("c24many", "c16few"), ("c24five", "c16many")],
             80: [("c40five", "c40many"), ("c40many", "c40one"), ("c40one", "c40five"), ("c40many", "c40many")],
             # ids: 20 and 21 different ones without the cap's flag, the cap itself, ids that nodes.dmp does not have
             20: [("c16many", "c4few"), ("c20one",), ("c20few",)], 21: [("c16many", "c5far")], 24: [("c24many",), ("c24five",), ("c24one",)]}


def row_reads(motifs, seed=SEED + 2):
    """set 2: one or two matches whose rows sum to 1 .. 80 (kLocDeferRows = 8 from both sides for one and for two matches, the
    many-rows instantiation with and without the id cap); two matches in one fragment and in two"""
    b = Builder(motifs, seed)
    for total, combos in ROW_RUNGS.items():
        for names in combos:
            assert b.rows_of(names) == total, names
            reps = 2 if len(names) == 2 or len(combos) >= 4 else 4
            for q in range(reps):
                stops = {0} if (len(names) == 2 and q % 2) else ()
                for nm in (names, names[::-1])[: len(names)]:
                    b.add(("rows", total, len(names)), b.join(nm, stops), k=len(names), rows=total, pad_to=LONG)
    return b.reads


def _short_names(b, k):
    pool = [f"h{i}" for i in range(24)] + ["h2_0", "h2_1", "h2_2", "h3_0", "h3_1", "h3_2"]
    return [pool[int(i)] for i in b.rng.permutation(len(pool))[:k]]


def lazy_reads(motifs, seed=SEED + 3):
    """set 3: pairs of mates of at most 287 nt (8-residue motifs, one spacer residue, at most 9 a mate), for
    min_fragment_length = 8: the fast stage 1 and, with SEG, the lazy flow; and single short reads"""
    b = Builder(motifs, seed)
    fill = lambda: _rand(b.rng, int(b.rng.integers(20, 40)))
    splits = {1: [(1, 0), (0, 1)], 2: [(1, 1), (2, 0)], 3: [(2, 1), (3, 0), (0, 3)], 8: [(4, 4), (8, 0)], 16: [(8, 8), (9, 7)],
              17: [(9, 8), (8, 9)], 18: [(9, 9)]}
    for k, sp in splits.items():
        for q in range((4 if len(sp) == 1 else 2) * (2 if k > 16 else 1)):
            for a, c in sp:
                names = _short_names(b, k)
                p1 = b.join(names[:a], one_spacer=True) if a else fill()
                p2 = b.join(names[a:], one_spacer=True) if c else fill()
                b.add(("pair", k), p1, p2, k=k, rows=b.rows_of(names), mlen=8)
    for q in range(4):
        # the longest matches of a pair in two fragments: of two mates, of one mate
        n2 = _short_names(b, 3)
        b.add(("multi", "mates"), b.join(n2[:1], one_spacer=True), b.join(n2[1:2], one_spacer=True), k=2, rows=b.rows_of(n2[:2]), mlen=8)
        b.add(("multi", "stop"), b.join(n2, {0}, one_spacer=True), fill(), k=3, rows=b.rows_of(n2), mlen=8)
        # more than kLocDeferRows rows under the lazy flow
        b.add(("pairrows", 9), b.join(["h9"], one_spacer=True), fill(), k=1, rows=9, mlen=8)
        b.add(("pairrows", 10), b.join(["h9"], one_spacer=True), b.join(n2[:1], one_spacer=True), k=2, rows=9 + b.rows_of(n2[:1]), mlen=8)
        # a low-complexity run of 14 residues and more in the fragment of a longest match: beside the motif (SEG cuts the run,
        # the match stays) and across it (the motif is cut out with the run: the second search changes the answer)
        nm = _short_names(b, 2)
        run = "QA"[q % 2] * (14 + q)
        b.add(("lc", "beside"), b.m[nm[0]].seq + b.spacer(1) + run, b.join(nm[1:], one_spacer=True) if q % 2 else fill(),
              k=1 + q % 2, rows=b.rows_of(nm[: 1 + q % 2]), mlen=8)
        lc, ch = (("lcq", "Q"), ("lcs", "S"))[q % 2]
        # (q >= 2: the other mate's fragment is the longer one and searched first - the fragment noted in the record is clean,
        #  only kWinMulti makes anybody look at the flagged one)
        others = nm[:1] if q < 2 else _short_names(b, 3)
        b.add(("lc", "across"), ch * (4 + q) + b.m[lc].seq + ch * 4, b.join(others, one_spacer=True), k=1 + len(others),
              rows=1 + b.rows_of(others), mlen=8)
    # no match at all: a pair that nobody lists (the record's note is 0) - the filling of the pair layouts
    for q in range(4):
        b.add(("pair", 0), fill(), fill(), k=0, rows=0, mlen=8)
    single = Builder(motifs, seed + 100)
    for k in (1, 2, 3):
        for q in range(4):
            names = _short_names(single, k)
            single.add(("single", k), single.join(names, {0} if q % 2 else (), one_spacer=True), k=k, rows=single.rows_of(names), mlen=8)
    # more than 16 longest matches in ONE fragment, nothing in it for SEG: without kWinForce nobody lists such a read
    for n in (17, 18, 40):
        for q in range(4):
            # (a spacer in front: a search that reaches residue 1 of its fragment ends the fragment, bwt.c:376 - a match
            #  from residue 0 directly behind one from residue 1 is never looked for, and the census does not know that)
            single.add(("force", n), "W" + (UNITS[q % 2] * 8)[q: q + 8 + n - 1], k=n, rows=n, mlen=8)
    return b.reads, single.reads


def greedy_reads(motifs, seed=SEED + 4):
    """set 4: one motif k times in a read, k = 1 .. 22: k best matches of one score (max_matches_SI = 20 from both sides)"""
    b = Builder(motifs, seed)
    for k in range(1, 23):
        for kind in ("g1", "g9"):
            for i in range(4):
                nm = f"{kind}_{i}"
                stops = set(range(1, k, 4)) if i % 2 else ()
                b.add(("greedy", k, kind), b.join([nm] * k, stops), k=k, rows=k * motifs[nm].copies)
    return b.reads


def filler_reads(motifs, n=760, seed=SEED + 5):
    """set 5's plain reads: no, one or two matches of few rows (mem_locate_read's two registers, at most kLocDeferRows rows)"""
    b = Builder(motifs, seed)
    pool = [f"s{i}" for i in range(26)] + ["c2one", "c2few", "c3few", "c4few", "x1"]
    for q in range(n):
        k = (1, 1, 2, 0, 1, 2, 1, 1)[q % 8]
        names = [pool[int(i)] for i in b.rng.integers(0, len(pool), size=k)]
        if b.rows_of(names) > 8:
            names = names[:1]
        pep = b.join(names, {0} if q % 3 == 0 else ()) if names else _rand(b.rng, 40)
        b.add(("fill", len(names)), pep, k=len(names), rows=b.rows_of(names), pad_to=LONG)
    return b.reads


def list_bound(r):
    """a read that k_mem_locate / k_mem_post1 hand on: three to sixteen matches (the list), or more than eight rows"""
    return 3 <= r.k <= 16 or (r.k <= 2 and r.rows > 8)


# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs():
    """everything, built once per process: .db (sequences), .motifs, .nodes_lines, .designed / .kept per set"""
    I = Inputs()
    I.nodes_lines, I.leaves, I.motifs, I.db = build_db()
    I.census = cs = Census(I.db)
    short_pairs, short_single = lazy_reads(I.motifs)
    I.designed = {"ladder": ladder_reads(I.motifs), "rows": row_reads(I.motifs), "pairs": short_pairs, "short": short_single,
                  "greedy": greedy_reads(I.motifs), "fill": filler_reads(I.motifs)}
    I.kept, I.dropped = {}, {}
    for name, reads in I.designed.items():
        keep, drop = [], []
        for r in reads:
            got = cs.read(r.mlen, *((r.nt1, r.nt2) if r.nt2 else (r.nt1,)))
            (keep if got == (r.k, r.rows, False) else drop).append(r)
        I.kept[name], I.dropped[name] = keep, drop
    return I


def pack(reads):
    paired = any(r.nt2 for r in reads)
    return util.pack([r.nt1.encode() for r in reads], [r.nt2.encode() for r in reads] if paired else None)


def layout_orders(I, seed=SEED + 6):
    """set 5: the reads of sets 1 and 2 and the plain ones as ONE base list (about 1000 reads); index lists into it -
    'front': the list-bound reads first; 'one_per_64': a list-bound read at the head of every wavefront of 64, plain ones
    behind it; 'perm': a permutation; and prefixes of 1, 63, 64, 65 and 257 reads of 'front' and of 'perm'"""
    base = I.kept["ladder"] + I.kept["rows"] + I.kept["fill"]
    lb = [i for i, r in enumerate(base) if list_bound(r)]
    rest = [i for i, r in enumerate(base) if not list_bound(r)]
    plain = [i for i in rest if base[i].k <= 2]
    orders = {"front": lb + rest}
    per = []
    for w in range(16):
        per.append(lb[(w * 7) % len(lb)])
        per += [plain[(w * 63 + q) % len(plain)] for q in range(63)]
    orders["one_per_64"] = per[:-30]                                   # (a partial last block)
    orders["perm"] = [int(i) for i in np.random.default_rng(seed).permutation(len(base))]
    for n in (1, 63, 64, 65, 257):
        orders[f"front{n}"] = orders["front"][:n]
        orders[f"perm{n}"] = orders["perm"][:n]
    return base, orders


def pair_orders(I, seed=SEED + 7):
    """the short pairs in the orders that the ballot of k_mem_post1's seglist sees: index lists into I.kept["pairs"], reads
    repeated.  A pair with more than 16 matches is listed whatever its fragments look like (kWinForce), a pair without a match
    never is: 'front' - 70 forced pairs, 70 that are never listed, then every pair once (wavefronts with 64, a few and no
    listed lanes, a partial last block); 'one_per_64' - a forced pair at the head of every wavefront of never-listed ones;
    'perm' - 'front' permuted"""
    pairs = I.kept["pairs"]
    forced = [i for i, r in enumerate(pairs) if r.k > 16]
    never = [i for i, r in enumerate(pairs) if r.k == 0]
    front = [forced[q % len(forced)] for q in range(70)] + [never[q % len(never)] for q in range(70)] + list(range(len(pairs)))
    per = []
    for w in range(4):
        per += [forced[(3 * w) % len(forced)]] + [never[(w + q) % len(never)] for q in range(63)]
    rng = np.random.default_rng(seed)
    return {"front": front, "one_per_64": per[:-20], "perm": [front[int(i)] for i in rng.permutation(len(front))]}


def write_db(I, workdir):
    """db.faa, db.fmi and nodes.dmp of the inputs in workdir"""
    from kaiju_amd import mkfmi, synth
    faa, fmi, nodes = (os.path.join(workdir, f) for f in ("db.faa", "db.fmi", "nodes.dmp"))
    with open(faa, "w") as f:
        for name, tax, s in I.db:
            f.write(f">{name}_{tax}\n{s}\n")
    synth.write_nodes_dmp(nodes, I.nodes_lines)
    mkfmi.build_fmi(faa, fmi, threads=2, exponent=3)
    return faa, fmi, nodes
