"""What every array of a loaded index must hold, derived from the index file and its FASTA alone (test infrastructure).

`Truth` uses numpy and the oracle's FM-index primitives - ko_fmindex_current (pinned to the reference's FMindexCurrent by
tests/golden/kat_fm.npz), ko_initial_si, ko_update_si, ko_get_suffix, ko_seq_name, ko_seq_taxid - and nothing of
kaiju_amd/csrc.  From the BWT letter of every row it builds rank and LF as prefix counts, folds UpdateSI over them for the
k-mer intervals, walks every sequence from its terminator row, and closes the loop outside any FM-index code: the residues
a walk collects must be the FASTA residues of the protein whose name the index gives that sequence number.

Orientation: the index stores every protein as the FASTA writes it.  A walk from terminator row t takes LF steps, i.e. it
reads the stored sequence from its last letter to its first; the stored sequence (offset 0 .. len-1, the order of
get_suffix's offsets and of DevIndex::text) is the FASTA record from its first residue to its last (STORED_REVERSED).
`Truth` asserts that this holds for every sequence of an index.

`compare_index` decodes the arrays of a loaded index (device: kaiju_gpu_index_read_array; host pack: the emulation's
emu_index_read_array) from the layout comments of kj_core.h - not by calling its code - and compares every element with
`Truth`.  It returns the names of the arrays it has checked."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

NONE32 = 0xffffffff
NONE64 = 0xffffffffffffffff
TEXT_PAD = 64
KLINE_MAXLEN, KLINE_SINGLE, KLINE_ESCAPE = 0xffbf, 0xffc0, 0xffff
WARN_SA_SHORT = 1
STORED_REVERSED = False       # the orientation of a stored sequence against its FASTA record (module docstring)

ARRAYS = ("rank_blocks", "count_bases", "sa_seq", "sa_taxid", "term_rows", "seq_taxid", "seq_valid", "kmer_table",
          "kmer_lines", "text", "sa_full", "row_tax", "tax_of_dense")


class Layout(C.Structure):          # kaiju_gpu_index_layout
    _fields_ = [("bytes", C.c_uint64 * len(ARRAYS)), ("C", C.c_uint64 * 22), ("bwtlen", C.c_uint64), ("n_sa", C.c_uint64),
                ("sa_skip", C.c_uint64)] + [(k, C.c_uint32) for k in
                                            ("nseq", "chpt_exp", "mb_shift", "kmer_k", "kline_k", "tv_shift", "n_dense",
                                             "beyond_lo", "beyond_n", "beyond_row", "wide", "reserved")]

    def size(self, name):
        return int(self.bytes[ARRAYS.index(name)])

    def present(self):
        return {a for a in ARRAYS if self.size(a)}


def read_fasta_records(path):
    names, seqs = [], []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                names.append(line[1:].split()[0])
                seqs.append([])
            elif line:
                seqs[-1].append(line)
    return names, ["".join(s) for s in seqs]


def fmi_sample_header(path):
    """(ncheck, chpt_exp) of the sample array as the file's header states them (suffixArray.c:282-311)"""
    with open(path, "rb") as f:
        head = f.read(4096)
    _, _, alen = struct.unpack_from("<qii", head, 0)
    _, ncheck, chpt_exp, _ = struct.unpack_from("<qqii", head, 16 + alen)
    return ncheck, chpt_exp


class Truth:
    def __init__(self, O, fmi, faa):
        self.fmi, self.faa = fmi, faa
        lib = self.lib = O.lib
        lib.ko_fmindex_current_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ko_get_suffix_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.ko_alphabet.restype = C.c_char_p
        lib.ko_alphabet.argtypes = [C.c_void_p]
        ix = self.ix = O.load_fmi(fmi)
        n = self.bwtlen = int(lib.ko_bwtlen(ix))
        nseq = self.nseq = int(lib.ko_nseq(ix))
        assert int(lib.ko_alen(ix)) == 21
        self.alphabet = lib.ko_alphabet(ix).decode()[:21]
        self.n_sa, self.chpt_exp = fmi_sample_header(fmi)
        e = self.chpt_exp
        self.sa_skip = ((nseq - 1) >> e) + 1
        # ---- L, rank, LF ----
        L = self.L = np.empty(n, dtype=np.uint8)
        lf = np.empty(n, dtype=np.int64)
        lib.ko_fmindex_current_rows(ix, 0, n, L.ctypes.data, lf.ctypes.data)
        assert L.max() <= 20
        counts = np.bincount(L, minlength=21)
        assert counts[0] == nseq
        Cc = self.C = np.zeros(22, dtype=np.int64)
        Cc[1:22] = np.cumsum(counts)
        assert Cc[21] == n
        for c in range(1, 21):
            si = (C.c_int64 * 2)()
            lib.ko_initial_si(ix, c, si)
            assert (si[0], si[1]) == (Cc[c], Cc[c + 1]), ("C[] against ko_initial_si", c)
        cum = self.cum = np.zeros((21, n + 1), dtype=np.int64)       # cum[c][k] = #{i < k : L[i] = c}
        for c in range(21):
            np.cumsum(L == c, out=cum[c, 1:])
        self.LF = Cc[L] + cum[L, np.arange(n)]                          # (terminators: C[0] = 0, the terminator's rank)
        assert (self.LF == lf).all(), "LF from the prefix counts against ko_fmindex_current"
        self.term_rows = np.nonzero(L == 0)[0].astype(np.uint64)
        # ---- sequence walks ----
        k = np.arange(nseq, dtype=np.int64)
        steps = np.zeros(nseq, dtype=np.int64)
        end_row = np.full(nseq, -1, dtype=np.int64)
        row_t = np.full(n, -1, dtype=np.int64)
        row_step = np.zeros(n, dtype=np.int64)
        active = np.arange(nseq)
        while len(active):
            kk = k[active]
            assert (row_t[kk] == -1).all(), "a row lies on two walks"
            row_t[kk] = active
            row_step[kk] = steps[active]
            done = L[kk] == 0
            end_row[active[done]] = kk[done]
            go = active[~done]
            k[go] = self.LF[kk[~done]]
            steps[go] += 1
            active = go
        assert (row_t >= 0).all(), "a row lies on no walk"
        seq_of_t = cum[0][end_row]                                      # rank of the terminator the walk ends at
        assert (np.sort(seq_of_t) == np.arange(nseq)).all()
        self.seq_len = np.zeros(nseq, dtype=np.int64)
        self.seq_len[seq_of_t] = steps
        self.row_seq = seq_of_t[row_t]
        self.row_pos = self.seq_len[self.row_seq] - row_step             # offset of the row's suffix in its sequence
        off = self.off = np.zeros(nseq + 1, dtype=np.int64)
        off[0] = TEXT_PAD
        off[1:] = TEXT_PAD + np.cumsum(self.seq_len + 1)
        assert off[nseq] - TEXT_PAD == n
        self.row_tpos = off[self.row_seq] + 1 + self.row_pos             # position in DevIndex::text of the row's suffix
        walk_text = np.zeros(TEXT_PAD + n, dtype=np.uint8)
        walk_text[self.row_tpos - 1] = L                                 # the BWT letter is the letter in front of the suffix
        # ---- the FASTA closes the loop ----
        fa_names, fa_seqs = read_fasta_records(faa)
        by_name = {}
        for nm, s in zip(fa_names, fa_seqs):
            assert nm not in by_name, ("FASTA names must be unique for the closure", nm)
            by_name[nm] = s
        code = np.zeros(256, dtype=np.uint8)
        for i, ch in enumerate(self.alphabet):
            code[ord(ch)] = i
        self.names = [lib.ko_seq_name(ix, q).decode() for q in range(nseq)]
        text = np.zeros(TEXT_PAD + n, dtype=np.uint8)
        for q, nm in enumerate(self.names):
            s = by_name[nm]
            assert len(s) == self.seq_len[q], ("length of", nm)
            res = code[np.frombuffer(s.encode(), dtype=np.uint8)]
            assert res.min() >= 1, ("a residue outside the index alphabet in", nm)
            text[off[q] + 1: off[q] + 1 + len(s)] = res[::-1] if STORED_REVERSED else res      # (see the module docstring)
        bad = np.nonzero(text != walk_text)[0]
        assert len(bad) == 0, ("the walks do not give the FASTA residues; first text position", int(bad[0]))
        self.text = text                                                 # (FASTA-derived; pads are added by the comparison)
        # ---- taxa ----
        self.seq_taxid = np.zeros(nseq, dtype=np.uint64)
        self.seq_valid = np.zeros(nseq, dtype=np.uint8)
        for q in range(nseq):
            ok = C.c_int(0)
            v = lib.ko_seq_taxid(ix, q, C.byref(ok))
            # (0: no usable id; 1: the whole name is the id; 3: the id follows the last '_', the accession in front of it
            #  is what the verbose columns print - ConsumerThread.cpp:814-832)
            self.seq_valid[q] = (3 if "_" in self.names[q] else 1) if ok.value else 0
            self.seq_taxid[q] = v if ok.value else NONE64
        # ---- rows behind the missing sample (a plain walk over LF; the reference reads out of bounds there) ----
        need = ((n - 1) >> e) - self.sa_skip + 1 if ((n - 1) >> e) >= self.sa_skip else 0
        assert self.n_sa <= need
        self.sa_short = self.n_sa < need
        beyond = np.zeros(n, dtype=bool)
        cur = np.arange(n, dtype=np.int64)
        alive = np.arange(n)
        first = True
        while len(alive):
            kk = cur[alive]
            sampled = (kk & ((1 << e) - 1)) == 0
            if first:
                sampled &= kk >= nseq                                    # (rows below nseq take their first step unconditionally)
            q = (kk >> e) - self.sa_skip
            stop = sampled & (q < self.n_sa)
            beyond[alive[sampled & (q >= self.n_sa)]] = True
            stop |= L[kk] == 0
            alive = alive[~stop]
            cur[alive] = self.LF[cur[alive]]
            first = False
        self.beyond = beyond
        assert beyond.any() == self.sa_short
        # ---- ko_get_suffix on every row a search can locate ----
        rows = np.nonzero(~beyond & (np.arange(n) >= nseq))[0].astype(np.int64)
        iseq = np.empty(len(rows), dtype=np.int32)
        pos = np.empty(len(rows), dtype=np.int64)
        lib.ko_get_suffix_rows(ix, rows.ctypes.data, len(rows), iseq.ctypes.data, pos.ctypes.data)
        bad = np.nonzero((iseq != self.row_seq[rows]) | (pos != self.row_pos[rows]))[0]
        assert len(bad) == 0, ("(sequence, offset) of the walks against ko_get_suffix; first row", int(rows[bad[0]]) if len(bad) else None)
        self._levels = {}

    # ---- rank and k-mer intervals -----------------------------------------------------------------------------------------
    def rank(self, c, k):
        return self.C[c] + self.cum[c][k]

    def kmer_level(self, k):
        """the non-empty words of k letters: (index, lo, len), index = letter matched first as the most significant digit;
        a word whose prefix is empty never appears (its interval stays {0, 0})"""
        if k in self._levels:
            return self._levels[k]
        if k == 1:
            c = np.arange(1, 21)
            ln = self.C[c + 1] - self.C[c]
            keep = ln > 0
            lv = ((c - 1)[keep].astype(np.int64), self.C[c][keep], ln[keep])
        else:
            idx, lo, ln = self.kmer_level(k - 1)
            parts = []
            for c in range(1, 21):
                a, b = self.rank(c, lo), self.rank(c, lo + ln)
                keep = a < b
                parts.append((idx[keep] * 20 + (c - 1), a[keep], (b - a)[keep]))
            idx2 = np.concatenate([p[0] for p in parts])
            o = np.argsort(idx2, kind="stable")
            lv = (idx2[o], np.concatenate([p[1] for p in parts])[o], np.concatenate([p[2] for p in parts])[o])
        self._levels[k] = lv
        return lv

    def update_si_fold(self, word):
        """the interval of a word (letters 1..20, matched in the order given) by ko_initial_si / ko_update_si themselves"""
        si = (C.c_int64 * 2)()
        self.lib.ko_initial_si(self.ix, int(word[0]), si)
        if si[1] <= si[0]:
            return (0, 0)
        for c in word[1:]:
            out = (C.c_int64 * 2)()
            if self.lib.ko_update_si(self.ix, int(c), si, out) <= 0:
                return (0, 0)
            si = out
        return (int(si[0]), int(si[1] - si[0]))

    def spot_check_kmers(self, k, n_words=2000, seed=0):
        rng = np.random.default_rng(seed + k)
        idx, lo, ln = self.kmer_level(k)
        table = dict(zip(idx.tolist(), zip(lo.tolist(), ln.tolist())))
        pick = np.concatenate([rng.choice(idx, size=min(len(idx), n_words // 2), replace=False),
                               rng.integers(0, 20 ** k, size=n_words - min(len(idx), n_words // 2))])
        for w in pick.tolist():
            word = [(w // 20 ** (k - 1 - j)) % 20 + 1 for j in range(k)]
            assert self.update_si_fold(word) == table.get(w, (0, 0)), ("k-mer interval against ko_update_si", k, word)

    def kline_stats(self, k):
        """(escape entries, single-row entries whose row holds a terminator, presence bits whose own entry is empty) of the
        lines of k-letter words - the preconditions the test indexes are built for"""
        idx, lo, ln = self.kmer_level(k)
        pw = 20 ** (k - 1)
        present = set(zip((idx // 20).tolist(), (idx % 20).tolist()))         # (line, b - 1) of the presence bits
        entry = set(zip((idx % pw).tolist(), (idx // pw).tolist()))          # (line, a - 1) of the non-empty entries
        lonely = sum(1 for m_b in present if m_b not in entry)
        return int((ln > KLINE_MAXLEN).sum()), int(((ln == 1) & (self.L[lo] == 0)).sum()), lonely


# ---- decoding and comparison ----------------------------------------------------------------------------------------------
def _same(name, got, want, what="element"):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{name}: shape {got.shape} (unit: {what}), the reference has {want.shape}"
    if got.ndim > 1:
        d = np.nonzero((got != want).any(axis=tuple(range(1, got.ndim))))[0]
    else:
        d = np.nonzero(got != want)[0]
    if len(d):
        i = int(d[0])
        raise AssertionError(f"{name}: {len(d)} differ; first {what} {i}: index holds {got[i].tolist()}, "
                             f"the reference says {want[i].tolist()}")


def expected_lines(T, k):
    """(codes of the lines that are not all zero, their 128 bytes each) for words of k letters"""
    idx, lo, ln = T.kmer_level(k)
    pw = 20 ** (k - 1)
    line_e, a = idx % pw, idx // pw                 # entry a of line M: the word a.M (a matched first)
    line_p, b = idx // 20, idx % 20                 # presence bit b of line M: the word M.b (b matched last)
    codes = np.unique(np.concatenate([line_e, line_p]))
    out = np.zeros((len(codes), 64), dtype=np.uint16)
    row = np.searchsorted(codes, line_e)
    l16 = np.where(ln == 1, KLINE_SINGLE | T.L[lo].astype(np.int64), np.where(ln <= KLINE_MAXLEN, ln, KLINE_ESCAPE))
    out[row, 3 * a] = lo & 0xffff
    out[row, 3 * a + 1] = (lo >> 16) & 0xffff
    out[row, 3 * a + 2] = l16
    pres = np.zeros(len(codes), dtype=np.uint32)
    np.bitwise_or.at(pres, np.searchsorted(codes, line_p), (1 << b).astype(np.uint32))
    out[:, 60] = pres & 0xffff
    out[:, 61] = pres >> 16
    return codes, out.view(np.uint8).reshape(len(codes), 128)


def compare_index(T: Truth, lay: Layout, read, ids_sequence=False):
    """read(name) -> the bytes of that array as a uint8 array.  Returns the set of array names compared."""
    n, nseq, e = T.bwtlen, T.nseq, T.chpt_exp
    checked = set()
    # scalars
    assert (lay.bwtlen, lay.nseq, lay.chpt_exp, lay.n_sa, lay.sa_skip) == (n, nseq, e, T.n_sa, T.sa_skip), "scalars of the layout"
    _same("C[]", np.array(lay.C[:], dtype=np.int64), np.concatenate([T.C[:21], [n]]))
    wide = bool(lay.wide)
    assert wide == (lay.size("count_bases") != 0)
    seq_taxid = np.arange(nseq, dtype=np.uint64) if ids_sequence else T.seq_taxid
    seq_valid = np.full(nseq, 3, dtype=np.uint8) if ids_sequence else T.seq_valid
    # 1. rank blocks (+ count bases)
    nb = (n >> 6) + 1
    assert lay.size("rank_blocks") == nb * 128
    blk = read("rank_blocks").view(np.dtype([("plane", "<u8", (5,)), ("cnt", "<u4", (20,)), ("pad", "<u4", (2,))]))
    bits = np.unpackbits(blk["plane"].copy().view(np.uint8).reshape(nb, 5, 8), axis=2, bitorder="little")      # [block][plane][row]
    letters = (bits.astype(np.uint8) << np.arange(5, dtype=np.uint8)[None, :, None]).sum(axis=1, dtype=np.uint8).reshape(-1)
    _same("rank_blocks (planes: BWT letter of every row)", letters[:n], T.L, "row")
    k0 = np.arange(nb, dtype=np.int64) * 64
    want = np.stack([T.rank(c, k0) for c in range(1, 21)], axis=1)                     # [block][letter]: rank(c, 64 b)
    got = blk["cnt"].astype(np.int64)
    if wide:
        assert lay.size("count_bases") == ((n >> lay.mb_shift) + 1) * 160
        base = read("count_bases").view("<u8").reshape(-1, 20).astype(np.int64)
        got = got + base[k0 >> lay.mb_shift]
        checked.add("count_bases")
    _same("rank_blocks (count base + count of every block and letter, the block behind the last row included)", got, want, "block")
    checked.add("rank_blocks")
    # 2. terminator rows, SA sample, per-sequence tables
    _same("term_rows", read("term_rows").view("<u8"), T.term_rows)
    smp_row = (np.arange(T.n_sa, dtype=np.int64) + T.sa_skip) << e
    assert (smp_row < n).all()
    _same("sa_seq", read("sa_seq").view("<u4"), T.row_seq[smp_row].astype(np.uint32), "sample")
    _same("seq_taxid", read("seq_taxid").view("<u8"), seq_taxid, "sequence")
    _same("seq_valid", read("seq_valid"), seq_valid, "sequence")
    checked |= {"term_rows", "sa_seq", "seq_taxid", "seq_valid"}
    if lay.size("sa_taxid"):
        assert not wide
        want = np.concatenate([seq_taxid[T.row_seq[smp_row]], [NONE64, NONE64]]).astype(np.uint64)      # (two entries of padding: no id)
        _same("sa_taxid", read("sa_taxid").view("<u8"), want, "sample")
        checked.add("sa_taxid")
    else:
        assert wide, "a narrow index keeps the taxon ids of its samples"
    # 3. k-mer table
    if lay.size("kmer_table"):
        k = int(lay.kmer_k)
        idx, lo, ln = T.kmer_level(k)
        assert lay.size("kmer_table") == 20 ** k * (16 if wide else 8)
        got = read("kmer_table").view("<u8" if wide else "<u4").reshape(-1, 2)
        nz = np.nonzero(got.any(axis=1))[0]                          # (every other word: empty = {0, 0})
        _same(f"kmer_table (k = {k}: the words whose entry is not {{0, 0}})", nz, idx, "word")
        _same(f"kmer_table (k = {k}: lo, len of every word that occurs; word = its place among them)", got[nz].astype(np.int64),
              np.stack([lo, ln], axis=1), "word")
        assert (got[:, 0].astype(np.uint64) + got[:, 1] <= n).all(), "kmer_table: lo + len beyond bwtlen"
        checked.add("kmer_table")
    # 4. k-mer lines
    if lay.size("kmer_lines"):
        k = int(lay.kline_k)
        assert not wide and lay.size("kmer_lines") == 20 ** (k - 1) * 128
        lines = read("kmer_lines").reshape(-1, 128)
        nz = np.nonzero(lines.view("<u8").any(axis=1))[0]
        codes, want = expected_lines(T, k)
        _same(f"kmer_lines (k = {k}: the lines that are not all zero)", nz, codes, "line")
        got = lines[nz]
        d = np.nonzero((got != want).any(axis=1))[0]
        if len(d):
            i = int(d[0])
            byte = int(np.nonzero(got[i] != want[i])[0][0])
            part = f"entry a = {byte // 6 + 1}" if byte < 120 else "presence bits" if byte < 124 else "bytes 124..127"
            raise AssertionError(f"kmer_lines (k = {k}): {len(d)} lines differ; first line {int(codes[i])}, {part} (byte {byte}): "
                                 f"index holds {got[i, byte - byte % 2: byte - byte % 2 + 6].tolist()}, the reference says "
                                 f"{want[i, byte - byte % 2: byte - byte % 2 + 6].tolist()}")
        checked.add("kmer_lines")
    # the taxon of every row
    contributes = seq_valid[T.row_seq].astype(bool) & ~T.beyond
    row_taxon = seq_taxid[T.row_seq]

    def check_row_tax():
        assert lay.size("row_tax") == n * 4 and lay.size("tax_of_dense") == lay.n_dense * 8
        rt = read("row_tax").view("<u4")
        tod = read("tax_of_dense").view("<u8")
        _same("row_tax (0xffffffff exactly on the rows that contribute no id)", rt == NONE32, ~contributes, "row")
        assert len(np.unique(tod)) == len(tod), "tax_of_dense holds a taxon twice"
        assert rt[contributes].max(initial=0) < len(tod), "row_tax: a dense index beyond tax_of_dense"
        _same("tax_of_dense[row_tax[r]] (taxon of every row)", tod[rt[contributes]], row_taxon[contributes], "contributing row")
        assert set(tod.tolist()) == set(seq_taxid[seq_valid.astype(bool)].tolist()), "tax_of_dense: not the taxa of the usable names"
        checked.update({"row_tax", "tax_of_dense"})

    def check_text():
        size = lay.size("text")
        assert size >= TEXT_PAD + n + TEXT_PAD, "text: no room for the pad behind the last sequence"
        want = np.zeros(size, dtype=np.uint8)
        want[:len(T.text)] = T.text
        _same("text (64 zero bytes, 0 + residues per sequence, zero padding)", read("text"), want, "byte")
        checked.add("text")

    if not wide:
        # 5. text and positions, narrow; 6. row_tax
        assert (lay.size("text") != 0) == (lay.size("sa_full") != 0) == (lay.size("row_tax") != 0) == (lay.size("tax_of_dense") != 0)
        if lay.size("text"):
            check_text()
            assert lay.size("sa_full") == n * 4
            sa = read("sa_full").view("<u4")
            _same("sa_full (text position of every row)", sa, T.row_tpos.astype(np.uint32), "row")
            assert (np.sort(sa) == np.arange(TEXT_PAD + 1, TEXT_PAD + 1 + n)).all(), "sa_full is no permutation of the text positions"
            checked.add("sa_full")
            check_row_tax()
            brows = np.nonzero(T.beyond)[0]
            if len(brows):
                tp = T.row_tpos[brows]
                assert tp.max() - tp.min() + 1 == len(brows)
                assert (lay.beyond_lo, lay.beyond_n) == (tp.min(), len(brows)), ("beyond_lo / beyond_n", lay.beyond_lo, lay.beyond_n, int(tp.min()), len(brows))
                assert T.beyond[lay.beyond_row], ("beyond_row is no row behind the missing sample", lay.beyond_row)
            else:
                assert (lay.beyond_lo, lay.beyond_n, lay.beyond_row) == (0, 0, 0)
        else:
            assert (lay.beyond_lo, lay.beyond_n, lay.beyond_row) == (0, 0, 0)
    else:
        # 7. text and positions, wide
        assert (lay.size("text") != 0) == (lay.size("sa_full") != 0)
        assert (lay.size("row_tax") != 0) == (lay.size("tax_of_dense") != 0)
        if lay.size("text"):
            check_text()
            s = int(lay.tv_shift)
            ne = (n >> s) + 1
            assert lay.size("sa_full") == ne * 5 + 16
            raw = read("sa_full")
            ent = raw[:ne * 5].reshape(ne, 5).astype(np.uint64)
            got = ent[:, 0] | ent[:, 1] << 8 | ent[:, 2] << 16 | ent[:, 3] << 24 | ent[:, 4] << 32
            want = np.full(ne, (1 << 40) - 1, dtype=np.uint64)                       # (all ones: no entry - the one behind the last row)
            r = np.arange(0, n, 1 << s)
            want[r >> s] = T.row_tpos[r].astype(np.uint64)
            _same(f"sa_tpos5 (tv_shift = {s}: text position of every 2^s-th row)", got, want, "entry")
            _same("sa_tpos5 (the 16 pad bytes)", raw[ne * 5:], np.zeros(16, dtype=np.uint8), "byte")
            checked.add("sa_full")
        if lay.size("row_tax"):
            assert not T.sa_short
            check_row_tax()
        assert (lay.beyond_lo, lay.beyond_n, lay.beyond_row) == (0, 0, 0)
    return checked


# ---- the test indexes ------------------------------------------------------------------------------------------------------
AA = "ACDEFGHIKLMNPQRSTVWY"


def _write_fasta(path, names, seqs):
    with open(path, "w") as f:
        for nm, s in zip(names, seqs):
            f.write(f">{nm}\n{s}\n")


def _check_size(bwtlen):
    assert bwtlen % 65536 != 0 and bwtlen % 65536 < 65408, "size at which the reference's rank has a bug: pick another seed"


def make_index_b(d, align64=False):
    """400 i.i.d. proteins of 30..400 residues, five names whose number overflows strtoul (no usable taxon id,
    ConsumerThread.cpp:809-833), 37 taxa.  nseq % 8 == 0, and two trims of the last protein:
      B (align64 False): bwtlen % 8 != 0 - the reference's sample array is one short (KAIJU_IDX_WARN_SA_SHORT);
      D (align64 True):  bwtlen % 64 == 0 - the rank block behind the last row is empty.
    One index cannot be both: the header counts (bwtlen >> e) - (nseq >> e) samples, get_suffix needs
    ((bwtlen - 1) >> e) - ((nseq - 1) >> e); with nseq % 8 == 0 these differ exactly when bwtlen % 8 != 0."""
    from kaiju_amd import mkfmi
    rng = np.random.default_rng(4001)
    nseq = 400
    lens = rng.integers(30, 401, size=nseq)
    lens[-1] = 100
    lens[-1] -= (int(lens.sum()) + nseq) % 64
    if not align64:
        lens[-1] -= 3
    assert lens[-1] >= 30
    taxa = 5000 + 7 * np.arange(37)
    names, seqs = [], []
    for i in range(nseq):
        tx = "99999999999999999999999" if i in (3, 77, 200, 201, 399) else str(int(taxa[rng.integers(0, len(taxa))]))
        names.append(f"B{i:04d}.1_{tx}")
        seqs.append("".join(AA[c] for c in rng.integers(0, 20, size=int(lens[i]))))
    _check_size(int(lens.sum()) + nseq)
    stem = "d" if align64 else "b"
    faa, fmi = str(d / f"{stem}.faa"), str(d / f"{stem}.fmi")
    _write_fasta(faa, names, seqs)
    mkfmi.build_fmi(faa, fmi, threads=4, exponent=3)
    return fmi, faa


def make_index_c(d, homopolymer=2000):
    """about 300 proteins in families of 5..40 near-identical members (synth.make_db_hard) plus 40 proteins of `homopolymer`
    times one letter: intervals of many rows, k-mer intervals above 65 471 rows (the escape entry of a k-mer line) at
    k = 2, 3 and 4; nseq % 8 != 0 and bwtlen % 64 != 0"""
    from kaiju_amd import mkfmi, synth
    _, leaves = synth.make_taxonomy(3, 3, 3)
    db = synth.make_db_hard(nseq=301, seed=4002, leaves=leaves, fam_lo=5, fam_hi=40, max_len=400)
    names = list(db.names)
    seqs = ["".join(synth.AA[c] for c in db.codes[db.offsets[i]:db.offsets[i + 1]]) for i in range(db.nseq)]
    for j in range(40):
        names.append(f"HP{j:03d}.1_{int(leaves[j % len(leaves)])}")
        seqs.append("K" * homopolymer)
    names.append("TAIL.1_1")
    seqs.append("ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWY")
    while len(names) % 8 == 0 or (sum(map(len, seqs)) + len(seqs)) % 64 == 0:
        seqs[-1] += "W"
    _check_size(sum(map(len, seqs)) + len(seqs))
    faa, fmi = str(d / "c.faa"), str(d / "c.fmi")
    _write_fasta(faa, names, seqs)
    mkfmi.build_fmi(faa, fmi, threads=4, exponent=3)
    return fmi, faa


def check_preconditions(which, T: Truth, warnings):
    """the edges an index was built for, asserted from the reference alone"""
    assert bool(warnings & WARN_SA_SHORT) == (which == "B") == T.sa_short
    if which == "B":
        assert T.nseq % 8 == 0 and T.bwtlen % 8 != 0
        assert T.beyond.any(), "no row behind the missing sample"
    if which == "D":
        assert T.nseq % 8 == 0 and T.bwtlen % 64 == 0
    if which in "BD":
        assert int((T.seq_valid == 0).sum()) == 5
        assert len(set(T.seq_taxid[T.seq_valid != 0].tolist())) < T.nseq
    if which == "C":
        assert T.nseq % 8 != 0 and T.bwtlen % 64 != 0
        stats = {k: T.kline_stats(k) for k in (2, 3, 4, 5)}
        for k in (2, 3, 4):
            assert stats[k][0] >= 1, ("no escape entry", k)
        assert sum(s[1] for s in stats.values()) >= 1, "no single-row entry whose row holds a terminator"
        assert sum(s[2] for s in stats.values()) >= 1, "no presence bit whose own entry is empty"
