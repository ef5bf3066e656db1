"""Inputs of the chain-pruning tests (test_chain_prune_emu.py on the host, test_gpu_chain_prune.py on the device), built from
seeds.  Two layers: cases for the rule alone (kj_chain_hopeless against chain_expect.walk), and a designed database with reads
whose variant chains sit on a chosen side of one threshold of the rule (greedy_lane2 against the oracle).

Layer 1 - the domain of kj_chain_hopeless, read off its two call sites in greedy_lane2 (kj_core.h, the narrow and the wide
lane's G_VMULTI step):
  - the variant substitutes the letter at pz = m_qi - 1 of a recorded match [m_qi, m_qi + m_ql - 1]; its own match is [pz, j]
    with j = m_qi + m_ql - 1 >= pz, l0 = j - pz + 1 = m_ql + 1 letters; GB_VAR_MATCH needs m_qi > 0, so pz >= 0;
  - GB_VAR_MATCH fills the window until pz is in it: wq <= pz <= wq + kWin - 1, so a = pz - wq is 0 .. 63.  A window fill
    puts the position asked for at the window's END (wq = max(0, top - 63)), a window carried by a popped item starts where
    the item's did, and a fragment with several recorded matches asks about one in the window another one's fill left
    behind: wq is 0 or anything up to pz.  a == 0 (`a <= 0` in the code) happens at the fragment's start (pz == wq == 0)
    and with wq == pz > 0, where the window shows nothing in front of pz;
  - win[0 .. 63] are the fragment's letters wq .. wq + 63 (what lies behind the fragment's end is whatever the row held), the
    row has four bytes of slack behind them (kGWinStride = 17 words);
  - letters are codes 1 .. 20 of the index alphabet; a text byte may be 0 (a sequence's terminator, the padding in front of
    the first sequence: the lane only looks when tp >= 16 + kTextPad, so the sixteen bytes exist);
  - nmm = t_nmm + 1 is 1 .. mismatches in the lane; the rule itself takes 0 .. mismatches, and so does the sweep;
  - sc0 = m_dsum + t_diff + bos is a small integer of either sign, thr = max(min_score, best) a positive one;
  - p.m = min_fragment_length, p.mismatches <= kMaxMismatch = 8 are the only parameters read."""
from __future__ import annotations

import functools

import numpy as np

import chain_expect as X

SEED = 20241021
WIN, ROW = 64, 68                                # kWin, KAIJU_GPU_CHAIN_WIN
A_SWEEP = tuple(range(0, 21)) + (60, 61, 62, 63)
WQ_SWEEP = (0, 37)
MISMATCHES = (0, 1, 3, 5)
# classes of a = pz - wq (the paths of the rule): the census counts per class
CLASSES = ("a0_pz0", "a0_wq", "lt16_wq0", "lt16_wq", "eq16", "gt16_sh0", "gt16_sh1", "gt16_sh2", "gt16_sh3")
# where the window shows all sixteen letters in front of pz (or the fragment's start): the rule is meant to be exact there
EXACT_CLASSES = ("a0_pz0", "lt16_wq0", "eq16", "gt16_sh0", "gt16_sh1", "gt16_sh2", "gt16_sh3")


def class_of(a, wq):
    a, wq = np.asarray(a), np.asarray(wq)
    c = np.where(a == 0, np.where(wq == 0, 0, 1), np.where(a < 16, np.where(wq == 0, 2, 3), np.where(a == 16, 4, 5 + ((a - 16) & 3))))
    return c.astype(np.int64)


def _popcount16(x):
    x = np.asarray(x, dtype=np.int64)
    return sum((x >> k) & 1 for k in range(16))


def _design_end(dmask, pz, left):
    """the designer's aim (the truth is chain_expect's): distance e of the (left + 1)-th difference, counting everything in front
    of the fragment's start as one; -1 where sixteen letters hold fewer; and the differences within e"""
    full = (dmask | ((0xffff << np.minimum(pz, 16)) & 0xffff)).astype(np.int64)
    m = full.copy()
    for q in range(8):
        m = np.where(q < left, m & (m - 1), m)
    e = np.full(len(m), -1, dtype=np.int64)
    for k in range(15, -1, -1):
        e = np.where((m >> k) & 1, k, e)
    nsub = _popcount16(full & ((1 << np.maximum(e, 0)) - 1))
    return e, nsub


def _masks(rng):
    """difference masks with 0 .. 5 bits set whose highest bit stands at every distance 0 .. 15"""
    out = [0]
    for nbits in range(1, 6):
        for d in range(nbits - 1, 16):
            low = rng.permutation(d)[: nbits - 1]
            out.append((1 << d) | sum(1 << int(b) for b in low))
    return np.array(out, dtype=np.int64)


# (l0 + e - m, what thr is): the score bound at thr - 1, thr and thr + 1 is the designer's reading of the rule's bound - eleven
# a letter gained, four a substitution; "low" = a threshold that every chain of the length reaches
COMBOS = ((-1, 0), (0, 1), (0, 0), (0, -1), (1, 1), (1, 0), (1, -1), (-1, "low"), (0, "low"), (1, "low"))


def _assemble(rng, a, wq, mm, nmm, dmask, zmask, l0, sc0, thr, m, all_w=None):
    """the arrays of a set of cases from the designer's choices: fragment and text letters, window rows, classes"""
    n = len(a)
    pz = wq + a
    front = rng.integers(1, 21, size=(n, 16))
    if all_w is not None:
        front = np.where(all_w[:, None], X.ALPHABET.index("W") + 1, front)
    k = np.arange(16)[None, :]
    other = (front - 1 + rng.integers(1, 20, size=(n, 16))) % 20 + 1            # a letter that differs
    text = np.where((dmask[:, None] >> k) & 1, other, front)
    text = np.where(k >= pz[:, None], rng.integers(0, 21, size=(n, 16)), text)   # in front of the fragment's start: anything
    text = np.where((zmask[:, None] >> k) & 1, 0, text)
    front = np.where(k < pz[:, None], front, 0)
    # the window row: fragment letters wq .. wq + 63, four bytes of whatever behind them
    i = np.arange(WIN)[None, :]
    dist = a[:, None] - 1 - i                                                    # distance of window byte i in front of pz
    near = (dist >= 0) & (dist < 16)
    win = rng.integers(1, 21, size=(n, WIN))
    win = np.where(near, np.take_along_axis(front, np.clip(dist, 0, 15), axis=1), win)
    behind = i > (a + l0)[:, None] + rng.integers(0, 40, size=(n, 1))            # behind the fragment's end: what the row held
    win = np.where(behind, rng.integers(0, 256, size=(n, WIN)), win)
    row = np.concatenate([win, rng.integers(0, 256, size=(n, ROW - WIN))], axis=1).astype(np.uint8)
    return {"a": a, "wq": wq, "pz": pz, "j": pz + l0 - 1, "l0": l0, "mismatches": mm, "nmm": nmm, "sc0": sc0, "thr": thr, "m": m,
            "front": front, "nfront": np.where(pz > 16, 17, np.minimum(pz, 16)), "text": text, "win": row,
            "tx": text[:, ::-1].astype(np.uint8), "cls": class_of(a, wq)}


def sweep_cases(seed=SEED):
    """every a of A_SWEEP (all byte shifts of the window load twice), wq == 0 and wq > 0, every (mismatches, nmm), every mask of
    _masks, and around each the length and the score bound on both sides of their thresholds (COMBOS)"""
    rng = np.random.default_rng(seed)
    masks = _masks(rng)
    mmn = np.array([(mm, q) for mm in MISMATCHES for q in range(mm + 1)], dtype=np.int64)
    g = np.meshgrid(np.array(A_SWEEP), np.array(WQ_SWEEP), np.arange(len(mmn)), np.arange(len(masks)), np.arange(len(COMBOS)), indexing="ij")
    a, wq, mi, ki, ci = (x.ravel().astype(np.int64) for x in g)
    mm, nmm, dmask = mmn[mi, 0], mmn[mi, 1], masks[ki]
    n = len(a)
    m = np.full(n, 11, dtype=np.int64)
    e, nsub = _design_end(dmask, wq + a, mm - nmm)
    dl = np.array([c[0] for c in COMBOS], dtype=np.int64)[ci]
    low = np.array([c[1] == "low" for c in COMBOS])[ci]
    ds = np.array([0 if c[1] == "low" else c[1] for c in COMBOS], dtype=np.int64)[ci]
    l0 = np.where(e >= 0, np.maximum(1, m + dl - e), np.array([3, 10, 11])[dl + 1])
    sc0 = rng.integers(20, 91, size=n)
    bound = sc0 + np.where(e >= 0, 11 * (e - nsub) + 4 * nsub, 0)
    thr = np.where(low, sc0 - 40, bound - ds)
    # a third of the cases gain nothing but W, the letter whose diagonal entry is the largest: the bound is met exactly
    all_w = rng.integers(0, 3, size=n) == 0
    return _assemble(rng, a, wq, mm, nmm, dmask, np.zeros(n, dtype=np.int64), l0, sc0, thr, m, all_w)


def random_cases(n=60000, seed=SEED + 1):
    """on top: everything drawn - a, wq, m, difference density, text bytes that are no letters, realistic scores (the diagonal
    sum of l0 letters against min_score 65 and 50 and against thresholds near the match's own score)"""
    rng = np.random.default_rng(seed)
    a = np.where(rng.integers(0, 4, size=n) == 0, rng.integers(0, 18, size=n), rng.integers(0, 64, size=n))
    wq = np.where(rng.integers(0, 5, size=n) < 2, 0, rng.integers(1, 400, size=n))
    mm = np.array(MISMATCHES + (2, 4))[rng.integers(0, 6, size=n)]
    nmm = (rng.random(n) * (mm + 1)).astype(np.int64)
    m = np.array([11, 11, 15, 8])[rng.integers(0, 4, size=n)]
    dens = np.array([0.08, 0.3, 0.6])[rng.integers(0, 3, size=n)]
    bits = rng.random((n, 16)) < dens[:, None]
    dmask = (bits * (1 << np.arange(16))[None, :]).sum(axis=1).astype(np.int64)
    zbits = (rng.random((n, 16)) < 0.04) & (rng.integers(0, 3, size=n) == 0)[:, None]
    zmask = (zbits * (1 << np.arange(16))[None, :]).sum(axis=1).astype(np.int64)
    l0 = rng.integers(1, 16, size=n)
    sc0 = (l0 * rng.uniform(3.0, 8.0, size=n)).astype(np.int64) - rng.integers(0, 8, size=n)
    thr = np.array([65, 50, 0])[rng.integers(0, 3, size=n)]
    thr = np.where(thr == 0, sc0 + rng.integers(-5, 40, size=n), thr)
    return _assemble(rng, a, wq, mm, nmm, dmask, zmask, l0, sc0, thr, m, rng.integers(0, 6, size=n) == 0)


@functools.lru_cache(maxsize=None)
def rule_cases():
    """sweep + random set as one dictionary of arrays, with the walk's answers (`reachable`, `max_len`, `open`)"""
    s, r = sweep_cases(), random_cases()
    c = {k: np.concatenate([s[k], r[k]]) for k in s}
    c["n_sweep"] = len(s["a"])
    c["reachable"], c["max_len"], c["open"] = X.walk_all(c["front"], c["nfront"], c["text"], c["l0"], c["nmm"], c["sc0"], c["thr"], c["m"],
                                                          c["mismatches"])
    return c


def rule_census(c):
    """cases per (class of a, substitutions left, the walk's answer): every cell has to hold one, or a test over the set says
    nothing about it.  Returns the table; raises with the empty cells"""
    left = c["mismatches"] - c["nmm"]
    table = np.zeros((len(CLASSES), 6, 2), dtype=np.int64)
    np.add.at(table, (c["cls"], np.minimum(left, 5), c["reachable"].astype(np.int64)), 1)
    empty = [(CLASSES[i], int(q), bool(r)) for i, q, r in zip(*np.nonzero(table == 0))]
    assert not empty, empty
    return table


def pack_cases(c, dtype):
    """the cases as records of kaiju_gpu_chain_case (dtype: api.CHAIN_CASE_DTYPE or its twin in the host test)"""
    out = np.zeros(len(c["a"]), dtype=dtype)
    out["win"], out["tx"] = c["win"], c["tx"]
    for k in ("wq", "pz", "j", "sc0", "thr", "nmm", "m", "mismatches"):
        out[k] = c[k]
    return out


def show_case(c, i):
    """one case as text (what a failing assertion prints)"""
    return {k: (c[k][i].tolist() if hasattr(c[k], "__len__") else c[k]) for k in
            ("a", "wq", "pz", "j", "l0", "mismatches", "nmm", "sc0", "thr", "m", "front", "text", "reachable", "max_len", "open")}


# ---------------------------------------------------------------------------------------------------------------------------
# Layer 2: a designed database and designed reads
# ---------------------------------------------------------------------------------------------------------------------------
"""(layer 2)  Every read is built around ONE site of the database: a stretch R of r letters that the read holds exactly (its
seed, on as many rows as the site's family has members), and in front of it the read's copy of the protein with differences
at chosen distances (distance 0 is the letter next to R: always a difference - the variant that substitutes it is the root
of the chain).  With `mismatches` = M the differences d1 = 0 < .. < dM are substituted, the (M + 1)-th at distance e (or the
fragment's start there) ends the chain at r + e letters.  NEAR side: r + e == m and the match scores exactly min_score (or
exactly the read's best so far): the read is classified by that match alone.  FAR side: one letter short (the last
difference one letter closer) or one score point short: the chain changes nothing, with or without the rule.
Reads are protein reads (input_is_protein) unless a rung says otherwise: the fragment is the read."""

import util                                                                       # noqa: E402

LETTERS = "ACDEFGHIKLMNPQRSTVW"                  # the database's letters: no Y - the one site that starts with YY is the last row
# parameter tuples: name -> (min_fragment_length, mismatches, min_score)
TUPLES = {"mm1": (11, 1, 50), "mm3": (11, 3, 42), "mm5": (15, 5, 52), "mm0": (11, 0, 42)}
SEED2 = SEED + 100
TEXT_PAD, HEAD = 64, 16 + 64                     # kTextPad; the rule looks at text positions >= 16 + kTextPad only


class Site:
    """a stretch of a protein family: members[i] = (name, taxon, protein), rend = the position behind R in every member"""
    __slots__ = ("name", "members", "rend", "r")

    def __init__(self, name, members, rend, r):
        self.name, self.members, self.rend, self.r = name, members, rend, r


class DRead:
    __slots__ = ("name", "rung", "side", "tup", "pep", "site", "pz", "r", "hopeful", "lookable", "nt", "nt2", "extra")

    def __init__(self, **kw):
        self.nt = self.nt2 = None
        self.extra = None
        self.lookable = True
        for k, v in kw.items():
            setattr(self, k, v)


def _rl(rng, n, letters=LETTERS):
    return "".join(letters[int(i)] for i in rng.integers(0, len(letters), size=n))


def _other(rng, c, letters=LETTERS, also=""):
    while True:
        x = letters[int(rng.integers(0, len(letters)))]
        if x != c and x not in also:
            return x


def _sc(a, b):
    return int(X.B62[X.ALPHABET.index(a) + 1, X.ALPHABET.index(b) + 1])


def _diag(s):
    return sum(_sc(c, c) for c in s)


class Designer:
    """draws the proteins and the reads together: a site's letters are drawn until the near-side match scores the threshold"""

    def __init__(self, seed=SEED2):
        self.rng = np.random.default_rng(seed)
        self.sites, self.reads, self.n = [], [], 0
        from kaiju_amd import synth
        self.nodes_lines, self.leaves = synth.make_taxonomy(4, 4, 4)

    def taxon(self):
        self.n += 1
        return int(self.leaves[(7 * self.n) % 64])

    def chain(self, tup, r, target, letters=LETTERS, start=False, rlet=None):
        """(protein region of 24 + r letters whose last r are R, the read's letters for it by distance, e): the read differs at
        distance 0, at M - 1 more distances below e - 1, and at e = m - r (start: the fragment starts there instead); the match of
        m letters that the substitutions open scores `target`"""
        m, M, _ = TUPLES[tup]
        e = m - r
        rng = self.rng
        for _ in range(20000):
            reg = _rl(rng, 24, letters) + (rlet if rlet else _rl(rng, r, letters))
            prot_by_d = reg[:24][::-1]                                             # distance d -> the protein's letter
            D = [0] + sorted(int(x) for x in rng.permutation(np.arange(1, e - 1))[: M - 1]) if M else []
            read_by_d = list(prot_by_d)
            for d in D:
                read_by_d[d] = _other(rng, prot_by_d[d])
            score = _diag(reg[24:]) + sum(_sc(read_by_d[d], prot_by_d[d]) for d in range(e))
            if score == target or M == 0:
                for d in range(e, 24):                                             # behind the chain: nothing matches (no other seed)
                    read_by_d[d] = _other(rng, prot_by_d[d])
                return reg, read_by_d, e, D
        raise RuntimeError(("no chain", tup, r, target))

    def family(self, name, reg, k, hopeful, e, read_by_d, trail=None):
        """k proteins that hold reg's R and the letter in front of it; member `hopeful` (None: all) holds the whole region, the
        others differ from it AND from the read at distances 1 .. 3: their chains end at once.  The letter behind R grows with
        the member's number: that is the order of their rows"""
        rng = self.rng
        left, right = _rl(rng, int(rng.integers(22, 40))), _rl(rng, int(rng.integers(8, 30)))
        members = []
        nxt = sorted(rng.permutation(len(LETTERS))[:k])
        for i in range(k):
            body = list(reg)
            if hopeful is not None and i != hopeful:
                for d in (1, 2, 3):
                    body[23 - d] = _other(rng, reg[23 - d], also=read_by_d[d])
            lf = left if i == 0 else "".join(c if rng.random() < 0.8 else _other(rng, c) for c in left)   # (diverging further left)
            members.append((f"{name}m{i}", self.taxon(), lf + "".join(body) + (trail if trail is not None else LETTERS[int(nxt[i])] + right)))
        s = Site(name, members, len(left) + len(reg), len(reg) - 24)
        self.sites.append(s)
        return s

    def add(self, rung, side, tup, site, read_by_d, nfront, r, pre=5, tail="", hopeful=0, lookable=True, extra=None, head=None):
        """the read: `pre` letters that match nothing (head: these), the letters at distances nfront - 1 .. 0, R, the tail"""
        prot = site.members[hopeful if hopeful is not None else 0][2]
        R = prot[site.rend - r: site.rend]
        head = _rl(self.rng, pre) if head is None else head
        pre = len(head)
        pep = head + "".join(read_by_d[d] for d in range(nfront - 1, -1, -1)) + R + tail
        rd = DRead(name=f"{'.'.join(str(x) for x in rung)}.{side}#{len(self.reads)}", rung=rung, side=side, tup=tup, pep=pep, site=site,
                   pz=pre + nfront - 1, r=r, hopeful=hopeful, lookable=lookable, extra=extra)
        self.reads.append(rd)
        return rd

    def pair(self, rung, tup, r, k=1, hopeful=0, pre=5, tail_n=0, reps=1, by="len", lookable=True, long_pre=0, target=None, letters=LETTERS):
        """a site and its near-side and far-side read (by: "len" - the last difference one letter closer; "score" - one point
        less; "start" - the fragment starts where the chain ends, far side one letter later)"""
        m, M, T = TUPLES[tup]
        for _ in range(reps):
            reg, rb, e, D = self.chain(tup, r, T if target is None else target, letters)
            site = self.family(f"s{len(self.sites)}", reg, k, hopeful, e, rb)
            tail = _rl(self.rng, tail_n)
            prot_by_d = reg[:24][::-1]
            far = list(rb)
            kw = dict(tup=tup, site=site, r=r, tail=tail, hopeful=hopeful)
            if by == "start":
                self.add(rung, "near", read_by_d=rb, nfront=e, pre=0, lookable=lookable, **kw)
                self.add(rung, "far", read_by_d=rb, nfront=e - 1, pre=0, lookable=False, **kw)     # (shorter than m: no variant is made)
                continue
            if by == "len":
                far[e - 1] = _other(self.rng, prot_by_d[e - 1])
            else:
                # one point less at one of the substitutions (the census drops the pair if no letter gives it)
                for d in D:
                    want = _sc(rb[d], prot_by_d[d]) - 1
                    alt = [c for c in LETTERS if c != prot_by_d[d] and _sc(c, prot_by_d[d]) == want]
                    if alt:
                        far[d] = alt[0]
                        break
            self.add(rung, "near", read_by_d=rb, nfront=e + 1, pre=pre + long_pre, lookable=lookable, **kw)
            self.add(rung, "far", read_by_d=far, nfront=e + 1, pre=pre + long_pre, lookable=lookable and by == "len", **kw)


ROW_RUNGS = [(k, w) for k in (1, 2, 3, 4) for w in ("first", "last")][1:] + [(5, "all")]
# the window the rule is asked with.  Variants are made after the whole fragment has been searched, when the window stands at
# the fragment's start: a variant position pz <= 63 is asked about with wq == 0 and a = pz (all sixteen letters, every byte
# shift of the load: a = 16 .. 20, and up to 63), a position further in refills the window with pz at its end (a = 63,
# wq = pz - 63 > 0); an item popped later carries the window of its parent.  (class, a, letters behind R)
WIN_RUNGS = [("wq0", 16, 0), ("wq0", 17, 0), ("wq0", 18, 0), ("wq0", 19, 0), ("wq0", 20, 0), ("wq0", 40, 70), ("wq0", 63, 70), ("refill", 63, 10)]
# ... and any a with wq > 0 where ONE fragment holds TWO seeds: the match further in (core B, its variant at pzB >= 64) is
# visited first and refills the window (wq = pzB - 63), the variant of the other one (core A, at pzA) is already inside it and
# is asked about with a = pzA - pzB + 63 in a window that does not start with the fragment.  (class, a); a = 0 and 2 show
# fewer letters than the near-side chain needs (four): a rule that took the window's start for the fragment's would prune it
TWO_SEED_RUNGS = [("a0_wq", 0), ("lt16_wq", 2), ("lt16_wq", 6), ("lt16_wq", 11), ("eq16_wq", 16), ("gt16_wq", 17), ("gt16_wq", 18), ("gt16_wq", 19), ("gt16_wq", 20)]
TWO_SEED_HEAD = 30                               # letters in front of core A (a run of Y: no seed, the database has no Y)


def design(seed=SEED2):
    g = Designer(seed)
    # substitutions and thresholds: length and score from both sides, chains of 1, 3 and 5 substitutions
    for tup, rs in (("mm1", (7, 8, 9)), ("mm3", (7,)), ("mm5", (7, 8, 9))):
        for r in rs:
            g.pair(("len", tup), tup, r, reps=4 if len(rs) == 1 else 2)
            g.pair(("score", tup), tup, r, reps=4 if len(rs) == 1 else 2, by="score")
            g.pair(("start", tup), tup, r, reps=2, by="start")
    # rows: families of k members, one hopeful - the first and the last row of the interval; five rows: nobody looks
    for k, w in ROW_RUNGS:
        g.pair(("rows", k, w), "mm3", 7, k=k, hopeful=None if k == 5 else 0 if w == "first" else k - 1, reps=3, lookable=k <= 4)
    # one-row parents on rows 0 .. 3 modulo 4: single sites, the census sorts them by row
    g.pair(("single",), "mm3", 7, reps=24)
    # the window
    for cls, a, tail_n in WIN_RUNGS:
        pz = 80 if cls == "refill" else a
        g.pair(("win", cls, a), "mm3", 7, tail_n=tail_n, long_pre=pz - 4 - 5, reps=2, lookable=False)
    # a parent among the last three rows: the only site that starts with Y (the alphabet's last letter)
    m, M, T = TUPLES["mm3"]
    for _ in range(1):
        while True:
            reg, rb, e, D = g.chain("mm3", 7, T)
            reg2 = reg[:24] + "YY" + reg[26:]
            if _diag(reg2[24:]) == _diag(reg[24:]):
                break
        site = g.family("last3", reg2, 1, 0, e, rb)
        far = list(rb)
        far[e - 1] = _other(g.rng, reg[:24][::-1][e - 1])
        g.add(("last3",), "near", "mm3", site, rb, e + 1, 7)
        g.add(("last3",), "far", "mm3", site, far, e + 1, 7)
    # the head of the text: the index lays the sequences out in lexicographic order behind kTextPad zero bytes, so the protein that
    # starts with AAAA comes first and its site lies within 16 + kTextPad bytes of the array's start (the census reads the array back)
    g.head_sites = []
    for _ in range(1):
        reg, rb, e, D = g.chain("mm3", 7, T)
        far = list(rb)
        far[e - 1] = _other(g.rng, reg[:24][::-1][e - 1])
        name, tax = f"head{len(g.head_sites)}", g.taxon()
        prot = "AAAA" + reg[24 - e - 1:] + "A" + _rl(g.rng, 30)                 # R starts at offset e + 5 < 16
        site = Site(name, [(name + "m0", tax, prot)], 4 + e + 1 + 7, 7)
        g.head_sites.append(site)
        g.add(("head",), "near", "mm3", site, rb, e + 1, 7, lookable=False)
        g.add(("head",), "far", "mm3", site, far, e + 1, 7, lookable=False)
    # the threshold from the read's best so far: an exact match E of 11 letters behind R sets best = 50 before the chain's second
    # variant is made; near side: the chain's match scores 50 as well (a second best match), far side 49
    E = "AILSVTKMREQ"
    assert _diag(E) == 50
    qname, qtax = "bestq", g.taxon()
    g.best_prot = (qname + "m0", qtax, _rl(g.rng, 30) + "C" + E + "C" + _rl(g.rng, 20))
    for rep in range(3):
        reg, rb, e, D = g.chain("mm3", 7, 50, letters="CDEFGHNPW")
        site = g.family(f"best{rep}", reg, 1, 0, e, rb)
        prot_by_d = reg[:24][::-1]
        far = list(rb)
        for d in D[1:]:
            want = _sc(rb[d], prot_by_d[d]) - 1
            alt = [c for c in LETTERS if c != prot_by_d[d] and _sc(c, prot_by_d[d]) == want]
            if alt:
                far[d] = alt[0]
                break
        for side, by_d in (("near", rb), ("far", far)):
            g.add(("best",), side, "mm3", site, by_d, e + 1, 7, tail=E, lookable=False, extra=(qtax, 50))
    # two seeds in one long fragment (TWO_SEED_RUNGS), ONE substitution (mm1: the variant asked about in the designed window is
    # the chain's only one - with more, a far-side variant that the conservative exit lets through is pruned one level further
    # in, in a window of its own).  Core B is the far side of a five-row family: nobody looks at it, it classifies nothing
    m1, M1, T1 = TUPLES["mm1"]
    reg_b, rb_b, e_b, _ = g.chain("mm1", 7, T1)
    site_b = g.family("twoseedB", reg_b, 5, None, e_b, rb_b)
    far_b = list(rb_b)
    far_b[e_b - 1] = _other(g.rng, reg_b[:24][::-1][e_b - 1])
    core_b = "".join(far_b[d] for d in range(e_b, -1, -1)) + reg_b[24:]
    g.two_seed_b = site_b
    for cls, a in TWO_SEED_RUNGS:
        for rep in range(2):
            reg, rb, e, D = g.chain("mm1", 7, T1)
            site = g.family(f"s{len(g.sites)}", reg, 1, 0, e, rb)
            far = list(rb)
            far[e - 1] = _other(g.rng, reg[:24][::-1][e - 1])
            gap = 63 - a - (1 + 7) - e_b                                        # letters between R of core A and core B
            tail = "Y" * gap + core_b + "Y" * 10
            for side, by_d in (("near", rb), ("far", far)):
                g.add(("win2", cls, a), side, "mm1", site, by_d, e + 1, 7, tail=tail, head="Y" * TWO_SEED_HEAD, lookable=False)
    # the fragment's start under the variant (pz == 0): the read is the substituted letter and R, m letters; near side: they score
    # exactly min_score, far side one point less.  The lane never ASKS the rule here: a variant's priority is the score of the
    # fragment up to the match's end, at pz == 0 that is the match's own score sc0, and a variant below thr is not made at all
    # (`key < thr`) while one at thr with m letters passes the gate - the rule's first line is layer 1's.  The records are checked
    for rep in range(3):
        reg, rb, e, D = g.chain("mm3", 10, T)
        site = g.family(f"s{len(g.sites)}", reg, 1, 0, e, rb)
        p0 = reg[:24][::-1][0]
        alt = [c for c in LETTERS if c != p0 and _sc(c, p0) == _sc(rb[0], p0) - 1]
        far = list(rb)
        if alt:
            far[0] = alt[0]
        g.add(("pz0",), "near", "mm3", site, rb, 1, 10, pre=0, lookable=False)
        g.add(("pz0",), "far", "mm3", site, far, 1, 10, pre=0, lookable=False)
    return g


class World2:
    pass


@functools.lru_cache(maxsize=None)
def designed():
    """the database (proteins in file order), the reads, nucleotide copies; built once per process"""
    g = design()
    W = World2()
    W.g = g
    rng = np.random.default_rng(SEED2 + 1)
    seqs = [mem for s in g.sites for mem in s.members] + [g.best_prot]
    while len(seqs) < 330 or (len(seqs) + 1) % 8 == 0:
        seqs.append((f"fill{len(seqs)}", int(g.leaves[len(seqs) % 64]), _rl(rng, int(rng.integers(50, 110)))))
    order = rng.permutation(len(seqs))
    seqs = [seqs[int(i)] for i in order]
    W.db = seqs + [g.head_sites[0].members[0]]
    W.reads = g.reads
    W.nodes_lines, W.leaves = g.nodes_lines, g.leaves
    return W


def write_db(W, workdir):
    import os
    from kaiju_amd import mkfmi, synth
    faa, fmi, nodes = (os.path.join(workdir, f) for f in ("db.faa", "db.fmi", "nodes.dmp"))
    with open(faa, "w") as f:
        for name, tax, s in W.db:
            f.write(f">{name}_{tax}\n{s}\n")
    synth.write_nodes_dmp(nodes, W.nodes_lines)
    mkfmi.build_fmi(faa, fmi, threads=2, exponent=3)
    return faa, fmi, nodes


def chain_case(rd, member):
    """what the walk gets for the read's designed chain on one member's row: the fragment's and the protein's letters in front of
    the variant (nearest first), its match of r + 1 letters and that match's score"""
    prot = rd.site.members[member][2]
    x1 = rd.site.rend - rd.r - 1                                                  # the protein's letter under the variant
    front = X.code(rd.pep[: rd.pz][::-1][:16])
    text = [X.ALPHABET.index(prot[x1 - 1 - d]) + 1 if x1 - 1 - d >= 0 else 0 for d in range(16)]
    R = prot[rd.site.rend - rd.r: rd.site.rend]
    sc0 = _diag(R) + _sc(rd.pep[rd.pz], prot[x1])
    return front, text, rd.pz, rd.r + 1, sc0


def walk_claim(rd, thr=None):
    """the designed chain by the plain walk, row by row: (rows that reach a match, longest match over the rows)"""
    m, M, T = TUPLES[rd.tup]
    reach, longest = [], 0
    for i in range(len(rd.site.members)):
        front, text, pz, l0, sc0 = chain_case(rd, i)
        ok, ln, _ = X.walk(front, text, pz, l0, 1, sc0, T if thr is None else thr, m, M)
        if ok:
            reach.append(i)
        longest = max(longest, ln)
    return reach, longest


def pack_reads(reads, nucleotide=False):
    if nucleotide:
        return util.pack([r.nt.encode() for r in reads], [r.nt2.encode() for r in reads] if any(r.nt2 for r in reads) else None)
    return util.pack([r.pep.encode() for r in reads])


def nucleotide_reads(W):
    """the same chains from nucleotide reads (six-frame translation in front of the search; tuple mm3): back-translations of the
    short reads of the len / rows rungs, ONE long read (a fragment of more than kWin residues), and pairs whose mates sit on
    different rungs - a near-side mate with a far-side one of another site, both ways round, and two near-side mates.
    Returns (singles, pairs): lists of (name, nt1, nt2, the designed reads behind the mates)"""
    back = lambda pep: "".join(util.BACK[c] for c in pep)                       # noqa: E731
    short = [r for r in W.reads if r.tup == "mm3" and r.rung[0] in ("len", "rows") and len(r.pep) <= WIN]
    long1 = [r for r in W.reads if r.rung == ("win", "refill", 63)][:2]
    singles = [(r.name + ".nt", back(r.pep), "", (r,)) for r in short + long1]
    near = [r for r in short if r.side == "near"]
    far = [r for r in short if r.side == "far"]
    pairs = []
    for q in range(8):
        a, b = near[(3 * q) % len(near)], far[(5 * q + 1) % len(far)]
        if a.site is b.site:
            b = far[(5 * q + 2) % len(far)]
        mates = (a, b) if q % 2 == 0 else (b, a)
        if q >= 6:
            mates = (a, near[(3 * q + 1) % len(near)])
        pairs.append((f"pair{q}", back(mates[0].pep), back(mates[1].pep), mates))
    return singles, pairs


def oracle_params(oracle, tup, seg=0, protein=1):
    m, M, T = TUPLES[tup]
    return oracle.params("greedy", seg=seg, use_evalue=0, protein=protein, min_fragment_length=m, mismatches=M, min_score=T)


def reads_of(reads, tup):
    """the reads of a parameter tuple; mm0 (no substitutions: the rule is never asked) runs those of mm3"""
    return [r for r in reads if r.tup == ("mm3" if tup == "mm0" else tup)]


def locate(W, text, sa):
    """where the index put every read's site: text (the index's text array, bytes) and sa (its full suffix array, uint32) -> per
    read name (row of the parent match R, text position of the variant's match).  The row cannot be chosen, only found"""
    s = "".join("$" if b == 0 or b > 20 else X.ALPHABET[b - 1] for b in bytes(text))
    row_of = {int(p): i for i, p in enumerate(np.asarray(sa).tolist())}
    out = {}
    for rd in W.reads:
        prot = rd.site.members[rd.hopeful if rd.hopeful is not None else 0][2]
        at = s.find("$" + prot + "$")
        assert at >= 0 and s.find("$" + prot + "$", at + 1) < 0, rd.name
        tp_r = at + 1 + rd.site.rend - rd.r
        out[rd.name] = (row_of[tp_r], tp_r - 1)
    return out


def census(W, records, where, nrows):
    """the designer's claims against facts that know nothing of the lanes: the plain walk puts the designed chain on the claimed
    side, and the oracle's record (records[tuple][i] for reads_of(W.reads, tuple)[i], SEG off, protein input) has the designed
    match as its best - near side - or does not contain the site - far side.  Returns (kept reads with their final rungs,
    dropped reads).  Rungs that only the built index decides - the row of a one-row parent modulo 4, the last three rows, the
    head of the text - are given here (where: locate())"""
    kept, dropped = [], []
    for tup in ("mm1", "mm3", "mm5"):
        for rd, rec in zip(reads_of(W.reads, tup), records[tup]):
            m, M, T = TUPLES[tup]
            thr = rd.extra[1] if rd.extra else T
            reach, longest = walk_claim(rd, thr)
            ids = [int(x) for x in rec["taxid"][: int(rec["n_ids"])]]
            taxa = [t for _, t, _ in rd.site.members]
            if rd.side == "near":
                want = list(range(len(taxa))) if rd.hopeful is None else [rd.hopeful]
                ok = reach == want and longest == m and int(rec["best"]) == thr and all(taxa[i] in ids for i in want)
                if rd.extra:
                    ok = ok and int(rec["n_ids"]) == 2 and rd.extra[0] in ids
            else:
                ok = not reach and not any(t in ids for t in taxa)
                if rd.extra:
                    ok = ok and ids == [rd.extra[0]] and int(rec["best"]) == rd.extra[1]
            row, tp = where[rd.name]
            rung = rd.rung
            if rung == ("head",) and tp >= HEAD:
                rung = ("head_elsewhere",)                                       # (the other end of the file: an ordinary site)
            elif rung == ("head",):
                ok = ok and tp >= TEXT_PAD
            elif rung == ("last3",):
                ok = ok and row + 4 > nrows
            elif rung == ("single",):
                rung = ("gword", row & 3)
                ok = ok and row + 4 <= nrows and tp >= HEAD
            elif tp < HEAD or row + 4 > nrows:
                ok = False
            (kept if ok else dropped).append((rd, rung))
    # a far-side read stays only with its near-side twin (they share the site): a rung is judged from both sides of one threshold
    sites = {}
    for rd, rung in kept:
        sites.setdefault(rd.site.name, set()).add(rd.side)
    both = [(rd, rung) for rd, rung in kept if sites[rd.site.name] == {"near", "far"}]
    dropped += [(rd, rung) for rd, rung in kept if sites[rd.site.name] != {"near", "far"}]
    return both, dropped


def required_rungs():
    out = [(k, t) for k in ("len", "score", "start") for t in ("mm1", "mm3", "mm5")]
    out += [("rows", k, w) for k, w in ROW_RUNGS] + [("gword", q) for q in range(4)] + [("win", c, a) for c, a, _ in WIN_RUNGS]
    out += [("win2", c, a) for c, a in TWO_SEED_RUNGS]
    return out + [("last3",), ("head",), ("best",), ("pz0",)]
