"""A model of util/kaiju-gbk2faa.pl in Python: what the emulation (tests/test_gbk_emu.py) and the GPU tests
(tests/test_gpu_gbk.py) compare with.  tests/test_gbk_expect_golden.py pins it on the files the unmodified script wrote
(tests/golden/make_golden_gbk.py) and, where perl and the reference are present, on the script itself.

The rules are written as the script writes them - one chain of regular expressions per line, three variables carried from
line to line - and not as kaiju_amd/csrc/kj_gbk.h writes them (bytes and scans), so that the two do not share a mistake.
Python's bytes patterns are ASCII: \\s is [ \\t\\n\\r\\f\\v] and \\d is [0-9], what perl's are for strings of bytes."""
import os
import re
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "gbk")
REFERENCE = os.environ.get("KAIJU_REFERENCE", "/root/reference")
SCRIPT = os.path.join(REFERENCE, "util", "kaiju-gbk2faa.pl")

RE_TAXON = re.compile(rb'/db_xref="taxon:(\d+)"', re.S)
RE_PID = re.compile(rb'/protein_id="([^"]+)"', re.S)
RE_WHOLE = re.compile(rb'\s+/translation="([^"]+)"', re.S)
RE_OPENS = re.compile(rb'\s+/translation="([^"]+)\Z', re.S)
KEEP = frozenset(b"ARNDCQEGHILKMFPSTWYVarndcqeghilkmfpstwyv")
INFO_FIELDS = ("text_bytes", "written_bytes", "n_lines", "n_records", "letters_kept", "letters_dropped", "no_taxon_line", "overflow")
KINDS = ("taxon", "protein_id", "whole", "opens", "other")

FIXTURES = ("rules", "record", "crlf", "nopid", "tail_open", "tail_closed", "notaxon", "notaxon_late", "empty")


def golden(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def getlines(text):
    """the lines as `while(<$in_fh>) { chomp; ...` sees them: a trailing '\\n' opens no line"""
    if not text:
        return []
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    return lines


def filtered(seq):
    seq = seq.replace(b"B", b"D").replace(b"Z", b"E")
    return bytes(b for b in seq if b in KEEP)


class State:
    """what the script carries from line to line"""

    def __init__(self, taxon=None, pid=None, in_t=False):
        self.taxon, self.pid, self.in_t = taxon, pid, in_t

    def copy(self):
        return State(self.taxon, self.pid, self.in_t)

    def __eq__(self, other):
        return (self.taxon, self.pid, self.in_t) == (other.taxon, other.pid, other.in_t)

    def __repr__(self):
        return "State(%r, %r, %r)" % (self.taxon, self.pid, self.in_t)


def kind_of(line):
    """(kind from 1, capture)"""
    for kind, pat in enumerate((RE_TAXON, RE_PID, RE_WHOLE, RE_OPENS), 1):
        m = pat.search(line)
        if m:
            return kind, m.group(1)
    return 5, None


def convert(text, state=None, out_cap=None):
    """A block of text that ends behind a line end (or is the end of the file), converted from `state` (None: the start of a
    file).  Returns {"text": the whole output, "lines": its lines, "written": the whole lines in front of out_cap, "info":
    the fields of kaiju_gpu_gbk_info, "kinds": lines per kind, "state": the state behind the block - the one in front of it when
    the block overflows or lacks a taxon}"""
    before = state.copy() if state is not None else State()
    st = before.copy()
    out, kinds = [], [0] * 5
    records = kept = dropped = 0
    no_taxon_line = 0
    lines = getlines(text)

    def emit(span):
        nonlocal kept, dropped
        f = filtered(span)
        kept += len(f)
        dropped += len(span) - len(f)
        out.append(f + b"\n")

    for n, line in enumerate(lines, 1):
        kind, cap = kind_of(line)
        kinds[kind - 1] += 1
        if kind == 1:
            st.taxon = cap
        elif kind == 2:
            st.pid = cap
        elif kind in (3, 4):
            if st.taxon is None:
                no_taxon_line = no_taxon_line or n          # (the script dies here; the model goes on to count the lines)
                if kind == 4:
                    st.in_t = True
                continue
            out.append(b">" + (st.pid or b"") + b"_" + st.taxon + b"\n")
            records += 1
            if kind == 4:
                st.in_t = True
            emit(cap)
        elif st.in_t:
            emit(line)
            if b'"' in line:
                st.in_t = False
    if no_taxon_line:
        out, records, kept, dropped = [], 0, 0, 0
    full = b"".join(out)
    cap_bytes = len(full) if out_cap is None else out_cap
    written, at = [], 0
    for o in out:
        if at + len(o) > cap_bytes:
            break
        written.append(o)
        at += len(o)
    overflow = 1 if len(full) > cap_bytes else 0
    info = {"text_bytes": len(full), "written_bytes": at, "n_lines": len(lines), "n_records": records, "letters_kept": kept, "letters_dropped": dropped,
            "no_taxon_line": no_taxon_line, "overflow": overflow}
    return {"text": full, "lines": out, "written": b"".join(written), "info": info, "kinds": kinds, "state": before if (overflow or no_taxon_line) else st}


def convert_file(text):
    """(the script's output file, its exit status)"""
    r = convert(text)
    return (b"", 255) if r["info"]["no_taxon_line"] else (r["text"], 0)


def cuts_behind_lines(text):
    """every position behind a '\\n' inside the text"""
    return [k + 1 for k in range(len(text) - 1) if text[k:k + 1] == b"\n"]


def convert_blocks(text, cuts):
    """the file through convert() block by block, cut at `cuts`: (output, state behind the last block, 1-based line of the
    file that lacks a taxon or 0)"""
    st, out, lines = State(), [], 0
    for a, e in zip([0] + list(cuts), list(cuts) + [len(text)]):
        r = convert(text[a:e], st)
        if r["info"]["no_taxon_line"]:
            return b"", st, lines + r["info"]["no_taxon_line"]
        out.append(r["text"])
        st = r["state"]
        lines += r["info"]["n_lines"]
    return b"".join(out), st, 0


# ---- the script itself ----------------------------------------------------------------------------------------------
def have_script():
    return bool(shutil.which("perl")) and os.path.exists(SCRIPT)


def run_script(text, suffix=".gbk"):
    """(the file the unmodified script writes for `text`, its exit status)"""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in" + suffix), os.path.join(d, "out.faa")
        with open(src, "wb") as f:
            f.write(text)
        r = subprocess.run(["perl", SCRIPT, src, dst], capture_output=True, timeout=120)
        with open(dst, "rb") as f:
            return f.read(), r.returncode


# ---- generated texts ------------------------------------------------------------------------------------------------
FRAGMENTS = [b'/db_xref="taxon:', b'/db_xref="taxon:4"', b'/protein_id="', b'/translation="', b' /translation="', b"\t/translation=\"", b'"', b'"', b" ", b"12", b"7", b"0", b"a",
             b"MKV", b"BZbz", b"ACDEFGHIKLMNPQRSTVWY", b"xJ*", b"P1.1", b"\r", b"\x00", b"\x0b", b"\x0c", b"\x85", b"\xa0", b"/", b"taxon:", b"=", b"  ", b"acd"]


def random_text(rng, n_lines, taxon_first=True):
    """lines assembled from the fragments the rules look at"""
    lines = [b'     /db_xref="taxon:%d"' % rng.randrange(1, 99999)] if taxon_first else []
    for _ in range(n_lines):
        lines.append(b"".join(rng.choice(FRAGMENTS) for _ in range(rng.randrange(0, 7))))
    return b"\n".join(lines) + rng.choice((b"", b"\n"))


def genbank_text(rng, n_records, cds_per_record=4, origin_lines=40, taxon_digits=None, pid_len=None):
    """text in the shape of a GenBank flat file: LOCUS, source, CDS features with multi-line translations, an ORIGIN block"""
    out = []
    for r in range(n_records):
        taxon = b"".join(b"%d" % rng.randrange(1 if k == 0 else 0, 10) for k in range(taxon_digits or rng.randrange(1, 8)))
        out.append(b"LOCUS       NC_%06d            %d bp    DNA     linear   VRL 01-JAN-2020\n" % (r, origin_lines * 60))
        out.append(b"DEFINITION  Synthetic virus %d, complete genome.\nFEATURES             Location/Qualifiers\n     source          1..%d\n" % (r, origin_lines * 60))
        out.append(b'                     /organism="Synthetic virus %d"\n                     /mol_type="genomic DNA"\n                     /db_xref="taxon:%s"\n' % (r, taxon))
        for c in range(cds_per_record):
            pid = (b"YP_%09d.1" % rng.randrange(10 ** 9)) if pid_len is None else bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789._") for _ in range(pid_len))
            seq = bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQRSTVWYXBZU") for _ in range(rng.choice((5, 30, 44, 45, 200, 431))))
            out.append(b"     CDS             %d..%d\n" % (c * 300 + 1, c * 300 + 299))
            out.append(b'                     /gene="g%d"\n                     /codon_start=1\n                     /product="hypothetical protein"\n' % c)
            out.append(b'                     /protein_id="%s"\n' % pid)
            body = b'/translation="' + seq + b'"'
            first = body[:58]
            rest = [body[k:k + 58] for k in range(58, len(body), 58)]
            out.append(b"".join(b"                     " + piece + b"\n" for piece in [first] + rest))
        out.append(b"ORIGIN\n")
        for k in range(origin_lines):
            out.append(b"%9d " % (k * 60 + 1) + b" ".join(bytes(rng.choice(b"acgt") for _ in range(10)) for _ in range(6)) + b"\n")
        out.append(b"//\n")
    return b"".join(out)
