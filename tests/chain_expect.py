"""What a Greedy variant chain on ONE database row can reach, by a plain walk (the reference of test_chain_prune_emu.py and
test_gpu_chain_prune.py; the cases: chain_inputs.py).  Written from the description of the chain alone - it shares no line
with kj_chain_hopeless and knows nothing of its masks or of its score bounds:

  the item's match [pz, j] of the fragment lies on one row, so everything that happens to it and to the items that descend
  from it is an ungapped comparison, leftwards, of the fragment with the database text in front of the row's suffix:
    - the match grows by one letter while fragment and text agree;
    - where they differ a substitution takes the TEXT's letter, costs one of the `mismatches - nmm` that are left and scores
      BLOSUM62[fragment's letter][text's letter] instead of the diagonal;
    - the chain ends at the next difference once they are spent, at the fragment's start, and at a text byte that is no letter
      (a sequence's terminator, the padding in front of the first sequence).
  A match is looked at (eval_match_scores) where its growth ends: in front of every difference, and at the chain's end - the
  stopping points.  Between two of them the score only grows (every diagonal entry is positive), so they are the places where
  a match of m letters scores highest.

Letters are codes of the index alphabet, 1 .. 20 (ALPHABET[c - 1]); 0 is no letter.  A case hands the walk the SIXTEEN letters
in front of the match on both sides, nearest first (distance 0 is the letter next to the match).  A chain that is still alive
behind the sixteenth letter is open: nobody can say from the case what it reaches, so it counts as reachable."""
from __future__ import annotations

import numpy as np

ALPHABET = "ACDEFGHIKLMNPQRSTVWY"              # the index alphabet: code = position + 1
_ORDER = "ARNDCQEGHILKMFPSTWYV"                 # the order in which BLOSUM62 is usually printed (and printed below)
_B62 = """
 4 -1 -2 -2  0 -1 -1  0 -2 -1 -1 -1 -1 -2 -1  1  0 -3 -2  0
-1  5  0 -2 -3  1  0 -2  0 -3 -2  2 -1 -3 -2 -1 -1 -3 -2 -3
-2  0  6  1 -3  0  0  0  1 -3 -3  0 -2 -3 -2  1  0 -4 -2 -3
-2 -2  1  6 -3  0  2 -1 -1 -3 -4 -1 -3 -3 -1  0 -1 -4 -3 -3
 0 -3 -3 -3  9 -3 -4 -3 -3 -1 -1 -3 -1 -2 -3 -1 -1 -2 -2 -1
-1  1  0  0 -3  5  2 -2  0 -3 -2  1  0 -3 -1  0 -1 -2 -1 -2
-1  0  0  2 -4  2  5 -2  0 -3 -3  1 -2 -3 -1  0 -1 -3 -2 -2
 0 -2  0 -1 -3 -2 -2  6 -2 -4 -4 -2 -3 -3 -2  0 -2 -2 -3 -3
-2  0  1 -1 -3  0  0 -2  8 -3 -3 -1 -2 -1 -2 -1 -2 -2  2 -3
-1 -3 -3 -3 -1 -3 -3 -4 -3  4  2 -3  1  0 -3 -2 -1 -3 -1  3
-1 -2 -3 -4 -1 -2 -3 -4 -3  2  4 -2  2  0 -3 -2 -1 -2 -1  1
-1  2  0 -1 -3  1  1 -2 -1 -3 -2  5 -1 -3 -1  0 -1 -3 -2 -2
-1 -1 -2 -3 -1  0 -2 -3 -2  1  2 -1  5  0 -2 -1 -1 -1 -1  1
-2 -3 -3 -3 -2 -3 -3 -3 -1  0  0 -3  0  6 -4 -2 -2  1  3 -1
-1 -2 -2 -1 -3 -1 -1 -2 -2 -3 -3 -1 -2 -4  7 -1 -1 -4 -3 -2
 1 -1  1  0 -1  0  0  0 -1 -2 -2  0 -1 -2 -1  4  1 -3 -2 -2
 0 -1  0 -1 -1 -1 -1 -2 -2 -1 -1 -1 -1 -2 -1  1  5 -2 -2  0
-3 -3 -4 -4 -2 -2 -3 -2 -2 -3 -2 -3 -1  1 -4 -3 -2 11  2 -3
-2 -2 -2 -3 -2 -1 -2 -3  2 -1 -1 -2 -1  3 -3 -2 -2  2  7 -1
 0 -3 -3 -3 -1 -2 -2 -3 -3  3  1 -2  1 -1 -2 -2  0 -3 -1  4
"""


def blosum62():
    """B[c][d] for index codes c, d = 1 .. 20 (row and column 0: zeros, never used for a letter)"""
    rows = [[int(x) for x in line.split()] for line in _B62.strip().splitlines()]
    assert len(rows) == 20 and all(len(r) == 20 for r in rows) and all(rows[i][k] == rows[k][i] for i in range(20) for k in range(20))
    B = np.zeros((21, 21), dtype=np.int64)
    for i, a in enumerate(_ORDER):
        for k, b in enumerate(_ORDER):
            B[ALPHABET.index(a) + 1, ALPHABET.index(b) + 1] = rows[i][k]
    return B


B62 = blosum62()


def code(letters: str) -> list:
    return [ALPHABET.index(c) + 1 for c in letters]


def score(letters) -> int:
    """the diagonal sum of a string of codes (a match's own score without substitutions)"""
    return int(sum(B62[c, c] for c in letters))


def walk(front, text, pz, l0, nmm, sc0, thr, m, mismatches):
    """ONE case, letter by letter.  front / text: the fragment's and the text's codes in front of the match, nearest first
    (front may be shorter than sixteen only where the fragment starts: len(front) == min(16, pz)).
    Returns (reachable, max_len, open): some stopping point holds >= m letters with a score >= thr (or the chain is open);
    the longest match within the sixteen letters; the chain is still alive behind them"""
    assert len(front) == min(16, pz) and len(text) == 16
    length, sc, left = l0, sc0, mismatches - nmm
    reach = False
    is_open = False
    k = 0
    while True:
        if k == len(front):                       # the fragment's start - or the sixteenth letter
            is_open = k == 16 and pz > 16         # (pz == 16: the fragment starts exactly there)
            reach = reach or (length >= m and sc >= thr)
            break
        f, t = int(front[k]), int(text[k])
        if not 1 <= t <= 20:                      # no letter: the row's sequence starts here
            reach = reach or (length >= m and sc >= thr)
            break
        if f == t:
            length += 1
            sc += int(B62[f, f])
        else:
            reach = reach or (length >= m and sc >= thr)      # the match's growth ends: a stopping point
            if left == 0:
                break
            left -= 1
            length += 1
            sc += int(B62[f, t])
        k += 1
    return (reach or is_open), length, is_open


def walk_all(front, nfront, text, l0, nmm, sc0, thr, m, mismatches):
    """the same walk over arrays of cases (one step per distance; tests compare it with walk() on a sample): front, text
    (n, 16) codes nearest first, nfront (n,) = min(16, pz) with `open` possible only where the fragment goes on (pz > 16 is
    passed as nfront == 17).  Returns boolean reachable, integer max_len, boolean open"""
    front, text = np.asarray(front, dtype=np.int64), np.asarray(text, dtype=np.int64)
    n = len(front)
    length, sc = np.asarray(l0, dtype=np.int64).copy(), np.asarray(sc0, dtype=np.int64).copy()
    left = np.asarray(mismatches, dtype=np.int64) - np.asarray(nmm, dtype=np.int64)
    thr, m, nfront = (np.asarray(x, dtype=np.int64) for x in (thr, m, nfront))
    alive = np.ones(n, dtype=bool)
    reach = np.zeros(n, dtype=bool)
    for k in range(16):
        good = (length >= m) & (sc >= thr)
        f, t = front[:, k], text[:, k]
        start = alive & (nfront <= k)                                  # the fragment's start
        noletter = alive & ~start & ((t < 1) | (t > 20))
        differ = alive & ~start & ~noletter & (f != t)
        spent = differ & (left == 0)
        stop = start | noletter | differ                               # stopping points (a difference is one whether or not the chain goes on)
        reach |= stop & good
        alive &= ~(start | noletter | spent)
        same = alive & ~differ
        sub = alive & differ
        fs, ts = np.clip(f, 0, 20), np.clip(t, 0, 20)
        sc = sc + np.where(same, B62[fs, fs], 0) + np.where(sub, B62[fs, ts], 0)
        left = left - sub
        length = length + alive
    good = (length >= m) & (sc >= thr)
    is_open = alive & (nfront > 16)
    reach |= alive & good                                              # (nfront == 16: the fragment starts behind the sixteenth letter)
    return reach | is_open, length, is_open
