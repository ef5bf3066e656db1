"""Inputs of the record-extraction tests (tests/test_ingest_emu.py on the host, tests/test_gpu_ingest.py on the device): data
only.  Every one is the smallest text that can break one pass of kaiju_amd/csrc/ingest.hip.  cases(T, S) wants the tile size
in bytes and the elements per scan block as the implementation exports them (ingest_emu_constants).

A case is (id, fastq, keep_names, text1, text2 or None)."""
import numpy as np

from test_cli_ingest import make_fasta, make_fastq


def _fq(i, seq=b"ACGT", name=None, eol=b"\n"):
    name = name if name is not None else b"r%d" % i
    return b"@" + name + eol + seq + eol + b"+" + eol + b"I" * len(seq) + eol


def _fq_short(n, blank_every=0):
    """n FASTQ records of 1 - 3 letters"""
    out = []
    for i in range(n):
        out.append(_fq(i, b"ACG"[: 1 + i % 3]))
        if blank_every and i % blank_every == 0:
            out.append(b"\n")
    return b"".join(out)


def _fq_lines(n_lines):
    """a FASTQ text of exactly n_lines lines that has lines of length 0 (the state-machine path): records with an empty
    sequence line, blank lines in front of headers"""
    out, k, i = [], 0, 0
    while k < n_lines:
        if i % 3 == 0 and k + 1 <= n_lines:
            out.append(b"\n"); k += 1
            if k >= n_lines:
                break
        rec = [b"@q%d" % i, b"" if i % 4 == 1 else b"ACGTA"[: 1 + i % 5], b"+", b"" if i % 4 == 1 else b"IIIII"[: 1 + i % 5]]
        take = min(4, n_lines - k)
        out.append(b"".join(l + b"\n" for l in rec[:take])); k += take
        i += 1
    t = b"".join(out)
    assert t.count(b"\n") == n_lines
    return t


def _fa_lines(n_lines):
    """a FASTA text of exactly n_lines lines"""
    out = []
    for k in range(n_lines):
        out.append(b">s%d x\n" % k if k % 3 == 0 else (b"ACGTTGCA"[: 1 + k % 8] + b"\n"))
    return b"".join(out)


def _nl_at(pos):
    """a FASTQ record whose header line ends with the '\\n' at byte pos"""
    return b"@" + b"n" * (pos - 1) + b"\nACGT\n+\nIIII\n"


def _exact(nbytes):
    """one FASTQ record of exactly nbytes bytes"""
    L = (nbytes - 7) // 2
    t = b"@x\n" + b"C" * L + b"\n+\n" + b"I" * (nbytes - 7 - L) + b"\n"
    assert len(t) == nbytes
    return t


def cases(T, S):
    rng = np.random.default_rng(20)
    c = []

    def add(name, fastq, text1, text2=None, keep=False):
        c.append((name, fastq, keep, text1, text2))

    # tiles
    for d in (-1, 0, 1):
        add("nl_at_T%+d" % d, True, _nl_at(T + d))
    add("line_over_three_tiles", True, _fq(0) + b"@long\n" + b"ACGT" * (T // 2 + 100) + b"\n+\n" + b"I" * 10 + b"\n" + _fq(2))
    add("exactly_T_bytes", True, _exact(T))
    add("T_plus_1_bytes", True, _exact(T + 1))
    add("exactly_T_bytes_no_final_newline", True, _exact(T + 1)[:-1])
    add("empty_text", True, b"")
    add("one_newline", True, b"\n")
    add("only_empty_lines", True, b"\n\n\n\n\n")
    add("empty_text_fasta", False, b"")
    add("only_empty_lines_fasta", False, b"\n\n\n")
    # scans: one block, two levels; lines and records
    for n in (S - 1, S, S + 1, S * S - 1, S * S, S * S + 1):
        add("fq_state_machine_%d_lines" % n, True, _fq_lines(n))
        add("fa_%d_lines" % n, False, _fa_lines(n))
    for n in (S * S - 1, S * S, S * S + 1):
        add("fq_%d_short_records" % n, True, _fq_short(n))
    add("fq_short_records_blanks", True, _fq_short(3 * S + 5, blank_every=7))
    # zero-length reads, blank lines, CRLF, no final newline
    add("fq_empty_sequence_line", True, _fq(0) + b"@e\n\n+\n\n" + _fq(2) + b"\n\n" + _fq(3, b"") + _fq(4))
    add("fq_blank_lines_at_start", True, b"\n\n\n" + _fq(0) + _fq(1))
    add("fq_crlf", True, b"".join(_fq(i, b"ACGTAC", eol=b"\r\n") for i in range(40)))
    add("fq_crlf_blank_lines", True, b"\r\n".join(_fq(i, b"ACGTAC", eol=b"\r\n") for i in range(5)))
    add("fq_no_final_newline", True, (_fq(0) + _fq(1, b"GGCC")).rstrip(b"\n"))
    # a last record that is cut
    add("fq_cut_after_header", True, _fq(0) + b"@cut")
    add("fq_cut_after_header_nl", True, _fq(0) + b"@cut\n")
    add("fq_cut_after_sequence", True, _fq(0) + b"@cut\nACGTT")
    add("fq_cut_after_sequence_nl", True, _fq(0) + b"@cut\nACGTT\n")
    add("fq_cut_after_separator", True, _fq(0) + b"@cut\nACGTT\n+\n")
    add("fq_cut_blank_path", True, b"\n" + _fq(0) + b"@cut\nACGTT\n+")
    # quality lines that look like something else, bytes that are no letters
    add("fq_quality_lookalikes", True, b"@a\nACGT\n+\n@III\n@b\nACGT\n+\n+III\n@c\nACGT\n+\n>III\n@d\n@CGT\n@\n@III\n")
    add("fq_quality_lookalikes_blank", True, b"\n@a\nACGT\n+\n@III\n\n@b\nACGT\n+\n+III\n@c\n\n+\n>III\n")
    junk = bytes(range(0, 10)) + bytes(range(11, 256))
    add("fq_no_letters", True, b"@j\n" + junk + b"AC-G*T01" + b"\n+\nI\n" + _fq(1))
    add("fa_no_letters", False, b">j\n" + junk + b"\nAC-G*T01\n" + junk[128:] + b"\n>k\nAC\n")
    # names
    add("fq_names", True, _fq(0, name=b"a/1") + _fq(1, name=b"b c") + _fq(2, name=b"d\te") + _fq(3, name=b"") + _fq(4, name=b"/x") + _fq(5, name=b"n" * 40 + b" z"))
    add("fq_keep_names_crlf", True, b"".join(_fq(i, name=b"n%d x/1" % i, eol=b"\r\n") for i in range(9)), keep=True)
    add("fa_keep_names", False, b">a b/1\tc\nACGT\n>d\nAC\n", keep=True)
    # FASTA
    add("fa_wrapped", False, make_fasta(np.random.default_rng(3), 40, width=17))
    add("fa_empty_lines_in_body", False, b">a\nACGT\n\n\nGG\n>b\n\nTT\n")
    add("fa_gt_inside_line", False, b">a\nAC>GT\nA>\n>b x>y\nTT>\n")
    add("fa_first_line_no_gt", False, b"\n\nxfirst line\nACGT\nGG\n>b\nTT\n")
    add("fa_header_only", False, b">a\n>b\nAC\n>c\n")
    add("fa_header_only_no_nl", False, b">a\nACGT\n>b")
    add("fa_cr_only_line_first", False, b"\r\n>a\r\nACGT\r\n")
    long_seq = bytes(rng.choice(list(b"ACGT"), 100000).tolist())
    add("fa_100000_letters", False, b">s\nAC\n>long\n" + b"\n".join(long_seq[k:k + 70] for k in range(0, 100000, 70)) + b"\n>t\nGG\n")
    add("fa_100000_letters_one_line", False, b">s\nAC\n>long\n" + long_seq + b"\n>t\nGG\n")
    # pairs
    n = 2 * S + 3
    p1 = b"".join(_fq(i, b"ACGTAC", name=b"p%d/1" % i) for i in range(n))
    p2 = b"".join(_fq(i, b"TTGCA", name=b"p%d/2" % i) for i in range(n))

    def renamed(which):
        return b"".join(_fq(i, b"TTGCA", name=(b"p%d/2" % i) if i not in which else b"q%d/2" % i) for i in range(n))
    add("pair_equal", True, p1, p2)
    add("pair_mismatch_0", True, p1, renamed({0, 5, n - 1}))
    add("pair_mismatch_1", True, p1, renamed({1, n - 1}))
    add("pair_mismatch_last", True, p1, renamed({n - 1}))
    add("pair_second_longer", True, p1, p2 + _fq(n, name=b"p%d/2" % n))
    add("pair_second_shorter", True, p1, b"".join(_fq(i, b"TTGCA", name=b"p%d/2" % i) for i in range(n - 1)))
    add("pair_fasta", False, b">a/1\nACGT\nAC\n>b/1\nGG\n", b">a/2\nTT\n>b/2\nCCC\nC\n")
    add("pair_blank_second", True, p1, b"\n" + p2)
    # fuzz
    add("fuzz_fastq", True, make_fastq(np.random.default_rng(41), 2000))
    add("fuzz_fastq_crlf_blanks", True, make_fastq(np.random.default_rng(42), 2000, crlf=True, blanks=True, final_newline=False))
    add("fuzz_fasta", False, make_fasta(np.random.default_rng(43), 2000))
    return c
