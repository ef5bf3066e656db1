"""What kaiju-addTaxonNames makes of a file of three-column lines, restated from the rules (kaiju-addTaxonNames.cpp and
util.cpp:123-192 of the reference) on bytes: the parsers of nodes.dmp and names.dmp with their quirks, the three kinds of
annotation, the lines.  tests/test_names_expect_golden.py pins this file byte for byte to the reference tool's own outputs
under tests/golden/names/; every other test of the column compares with it.

A mode is "name", "path" or "ranks:<comma separated list>"."""
import numpy as np

DIGITS = b"0123456789"
LOWER = b"abcdefghijklmnopqrstuvwxyz"


def _run(line, start, allowed):
    end = start
    while end < len(line) and line[end] in allowed:
        end += 1
    return end


def _first(line, start, allowed):
    while start < len(line) and line[start] not in allowed:
        start += 1
    return start


def parse_nodes(text):
    """{id: (parent, rank)} - first line per id wins; a line that lacks a number, holds one beyond 64 bits, or has no lower-case
    letter behind the parent is skipped altogether"""
    nodes = {}
    for line in text.split(b"\n"):
        end = _run(line, 0, DIGITS)
        if end == 0 or end == len(line) or int(line[:end]) >= 2 ** 64:
            continue
        start = _first(line, end, DIGITS)
        if start == len(line):
            continue
        end = _run(line, start, DIGITS)
        if int(line[start:end]) >= 2 ** 64:
            continue
        parent = int(line[start:end])
        r0 = _first(line, end, LOWER)
        if r0 == len(line):
            continue
        nodes.setdefault(int(line[: _run(line, 0, DIGITS)]), (parent, line[r0:_run(line, r0, LOWER + b" ")]))
    return nodes


def parse_names(text):
    """{id: name} - only lines that contain "scientific name"; first line per id wins"""
    names = {}
    for line in text.split(b"\n"):
        if b"scientific name" not in line:
            continue
        start = _first(line, 0, DIGITS)
        end = _run(line, start, DIGITS)
        if start == len(line) or end == len(line) or int(line[start:end]) >= 2 ** 64:
            continue
        n0 = _run(line, end, b"\t|")
        if n0 == len(line):
            continue
        names.setdefault(int(line[start:end]), line[n0:_first(line, n0 + 1, b"\t|")])
    return names


class Names:
    def __init__(self, nodes_text, names_text, mode="name"):
        self.nodes, self.names = parse_nodes(nodes_text), parse_names(names_text)
        self.mode = "ranks" if mode.startswith("ranks:") else mode
        self.ranks = [r.encode() for r in mode[len("ranks:"):].split(",") if r] if self.mode == "ranks" else []
        assert self.mode in ("name", "path", "ranks")
        self._memo = {}

    def name_of(self, tid):
        return self.names.get(tid, b"taxonid:%d" % tid)

    def emitted(self, taxon):
        """the ids of the walk, leaf first"""
        out, tid = [], taxon
        while tid in self.nodes and self.nodes[tid][0] != tid:
            out.append(tid)
            tid = self.nodes[tid][0]
            assert len(out) <= len(self.nodes), "a cycle: the reference would not end"
        return out

    def annotation(self, taxon):
        """bytes, or None: the line stays as it is"""
        if taxon not in self._memo:
            self._memo[taxon] = self._annotation(taxon)
        return self._memo[taxon]

    def _annotation(self, taxon):
        if taxon not in self.nodes or taxon not in self.names:
            return None
        if self.mode == "name":
            return self.names[taxon]
        walk = self.emitted(taxon)
        if self.mode == "path":
            return b"".join(self.name_of(t) + b"; " for t in reversed(walk))
        value = {}
        for t in walk:
            rank = self.nodes[t][1]
            if rank != b"no rank" and rank in self.ranks:
                value[rank] = self.name_of(t)
        return b"".join(value.get(r, b"NA") + b"; " for r in self.ranks)

    def why_unchanged(self, taxon):
        return "unknown" if taxon not in self.nodes else "unnamed" if taxon not in self.names else None

    def line(self, line, drop_unclassified=False):
        """line: without its newline.  Returns the line(s) to write, with newline (b"": none)"""
        if not line:
            return b""
        if line[:1] != b"C":
            return b"" if drop_unclassified else line + b"\n"
        f = line.split(b"\t")
        a = self.annotation(int(f[2][:_run(f[2], 0, DIGITS)]))
        return line + b"\n" if a is None else line + b"\t" + a + b"\n"

    def text(self, text, drop_unclassified=False):
        return b"".join(self.line(l, drop_unclassified) for l in text.split(b"\n"))


NAMES_INFO_FIELDS = ("text_bytes", "n_records", "n_classified", "overflow", "n_inexact", "n_unknown_taxon", "n_unnamed_taxon", "n_dropped")


def expected(names, base, drop_unclassified=False, out_cap=None):
    """base: a dict of format_expect.expected (the three-column lines of a case, everything fitting).  The same dict for the
    lines with the column: text, written, info (kaiju_gpu_format_names_info), line_off"""
    res = base["res"]
    off3 = base["line_off"]
    lines, unknown, unnamed, dropped = [], 0, 0, 0
    for r in range(len(res)):
        three = base["text"][int(off3[r]):int(off3[r + 1]) - 1]
        # (the taxon is the record's: a read name that holds a tab does not move the third column here, as it would for the tool)
        if res[r]["classified"]:
            why = names.why_unchanged(int(res[r]["taxon"]))
            unknown += why == "unknown"
            unnamed += why == "unnamed"
            a = names.annotation(int(res[r]["taxon"]))
            out = three + b"\n" if a is None else three + b"\t" + a + b"\n"
        else:
            dropped += 1 if drop_unclassified else 0
            out = b"" if drop_unclassified else three + b"\n"
        lines.append(out)
    text = b"".join(lines)
    line_off = np.concatenate([[0], np.cumsum([len(l) for l in lines], dtype=np.int64)]).astype(np.int64)
    cap = len(text) if out_cap is None else out_cap
    fit = int(np.searchsorted(line_off, cap, side="right")) - 1
    info = dict(base["info"])
    info.update(text_bytes=len(text), overflow=1 if len(text) > cap else 0, n_unknown_taxon=unknown, n_unnamed_taxon=unnamed, n_dropped=dropped)
    return {"text": text, "written": text[: int(line_off[fit])], "info": info, "line_off": line_off}
