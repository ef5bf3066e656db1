"""What kaiju2table makes of output texts, restated from the rules (kaiju2table.cpp:192-360 and util.cpp:63-77 of the
reference) on bytes: the counts per line (kaiju_amd/csrc/kj_tally.h), the sums over the tree, and the rows of the table with
the tool's own mixed float arithmetic (kaiju_amd/csrc/host/table_rows.h).  tests/test_table_expect_golden.py pins this file
byte for byte to the reference tool's own outputs under tests/golden/table/; every other test of the tally and of the table
compares with it.

Options are a dict: rank, and optionally ranks (the text of -l), min_percent (-m), min_count (-c), expand_viruses (-e),
filter_unclassified (-u), full_path (-p)."""
import numpy as np

import names_expect as ne
from annotate_expect import read_id, split_lines

VIRUSES = 10239
INFO_FIELDS = ("used", "n_lines", "n_total", "n_unclassified", "n_bad_id", "n_unknown_taxon", "n_virus")
RANKS = ("phylum", "class", "order", "family", "genus", "species")
f32 = np.float32


class Tree:
    """nodes.dmp (and names.dmp) as the tool reads them"""

    def __init__(self, nodes_text, names_text=b""):
        self.nodes = ne.parse_nodes(nodes_text)            # {id: (parent, rank)}
        self.names = ne.parse_names(names_text)

    def is_virus(self, tid):
        """is_ancestor(nodes, 10239, tid)"""
        if VIRUSES not in self.nodes or tid not in self.nodes:
            return False
        if tid == VIRUSES:
            return True
        while tid in self.nodes and tid != self.nodes[tid][0]:
            tid = self.nodes[tid][0]
            if tid == VIRUSES:
                return True
        return False

    def walk(self, tid):
        """the ids from tid upwards: in front of a node that is its own parent, behind one whose parent is no node"""
        out = []
        while tid in self.nodes and tid != self.nodes[tid][0]:
            out.append(tid)
            tid = self.nodes[tid][0]
            assert len(out) <= len(self.nodes), "a cycle: the reference would not end"
        return out

    def name_of(self, tid):
        return self.names.get(tid, b"taxonid:%d" % tid)


def line_kind(tree, line):
    """(kind, taxon): kind one of empty, unclassified, bad_id, unknown, hit"""
    if not line:
        return "empty", None
    if line[:1] != b"C":
        return "unclassified", None
    tid = read_id(line)
    if tid is None:
        return "bad_id", None
    return ("hit", tid) if tid in tree.nodes else ("unknown", tid)


def count_text(tree, text, final=True):
    """one add call: (info of the call, {taxon: direct})"""
    used = len(text) if final else text.rfind(b"\n") + 1
    lines = split_lines(text[:used])
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["used"], info["n_lines"] = used, len(lines)
    direct = {}
    for line in lines:
        kind, tid = line_kind(tree, line)
        if kind == "empty":
            continue
        info["n_total"] += 1
        if kind == "unclassified":
            info["n_unclassified"] += 1
        elif kind == "bad_id":
            info["n_bad_id"] += 1
        elif kind == "unknown":
            info["n_unknown_taxon"] += 1
        else:
            direct[tid] = direct.get(tid, 0) + 1
            info["n_virus"] += 1 if tree.is_virus(tid) else 0
    return info, direct


def add_counts(totals, direct, info, more):
    for f in INFO_FIELDS:
        totals[f] = totals.get(f, 0) + info[f]
    for t, c in more.items():
        direct[t] = direct.get(t, 0) + c


def entries_of(tree, direct):
    """the entries of kaiju_gpu_tally_result, sorted by taxon: (taxon, direct, summed, virus) for every node with summed > 0"""
    summed = {}
    for tid, reads in direct.items():
        if tree.is_virus(tid):
            summed[tid] = summed.get(tid, 0) + reads
            continue
        for a in tree.walk(tid):
            summed[a] = summed.get(a, 0) + reads
    return [(t, direct.get(t, 0), s, 1 if tree.is_virus(t) else 0) for t, s in sorted(summed.items())]


def tally(tree, texts):
    """texts added one behind the other, the last one final: (totals, entries)"""
    totals, direct = {}, {}
    for k, text in enumerate(texts):
        info, more = count_text(tree, text, final=k + 1 == len(texts))
        add_counts(totals, direct, info, more)
    if not texts:
        totals = dict.fromkeys(INFO_FIELDS, 0)
    return totals, entries_of(tree, direct)


# ---- the rows ---------------------------------------------------------------------------------------------------------
def _fmt(x):
    """%.6f of a double as glibc prints it on x86-64 (0.0 / 0.0 there is the NaN with the sign set)"""
    x = float(x)
    return b"-nan" if x != x else b"%.6f" % x


def _ratio(a, b):
    """(float)a / (float)b"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return f32(a) / f32(b)


def rank_list(text):
    return [r for r in text.split(",") if r]


def refusal(opt):
    """why the tool refuses these options, None: it does not"""
    rank, ranks = opt.get("rank", ""), opt.get("ranks")
    if not rank:
        return "no rank"
    if ranks and opt.get("full_path"):
        return "-p with -l"
    if rank not in RANKS:
        return "bad rank"
    if opt.get("min_count", 0) < 0:
        return "-c below 0"
    if not 0.0 <= opt.get("min_percent", 0.0) <= 100.0:
        return "-m outside [0, 100]"
    if opt.get("min_percent", 0.0) > 0.0 and opt.get("min_count", 0) > 0:
        return "-m with -c"
    if ranks and rank not in rank_list(ranks):
        return "rank not in -l"
    return None


def table_rows(tree, entries, totals, opt, label):
    """the rows of one input file, without the header row"""
    assert refusal(opt) is None
    rank = opt["rank"].encode()
    min_count, min_percent = int(opt.get("min_count", 0)), f32(opt.get("min_percent", 0.0))
    expand, filt, full_path = bool(opt.get("expand_viruses")), bool(opt.get("filter_unclassified")), bool(opt.get("full_path"))
    ranks = [r.encode() for r in rank_list(opt["ranks"])] if opt.get("ranks") else None
    label = label if isinstance(label, bytes) else label.encode()
    unclassified, total, virus_reads = totals["n_unclassified"], totals["n_total"], totals["n_virus"]
    if filt:
        total -= unclassified
    at_rank = below_percent = below_count = 0
    shown = []
    for tid, _, count, _ in sorted(entries):
        if tree.is_virus(tid):
            shown.append((count, tid))
            continue
        if tree.nodes[tid][1] != rank:
            continue
        as_int = count & 0xffffffff
        as_int -= 1 << 32 if as_int >> 31 else 0               # (int)count
        if as_int >= min_count:
            if _ratio(count, total) * f32(100) >= min_percent:
                shown.append((count, tid))
            else:
                below_percent += count
        else:
            below_count += count
        at_rank += count
    above = (total - at_rank if filt else total - unclassified - at_rank) - virus_reads
    above &= 2 ** 64 - 1
    shown.sort(key=lambda p: (-p[0], p[1]))

    out = []
    for count, tid in shown:
        if not expand and tree.is_virus(tid):
            continue
        row = label + b"\t" + _fmt(_ratio(count, total) * f32(100.0)) + b"\t%d\t%d\t" % (count, tid)
        if ranks is not None:
            value = {}
            for a in tree.walk(tid):
                r = tree.nodes[a][1]
                if r != b"no rank" and r in ranks:
                    value[r] = tree.name_of(a)
            row += b"".join(value.get(r, b"NA") + b";" for r in ranks)
        elif full_path:
            row += b"".join(tree.name_of(a) + b";" for a in reversed(tree.walk(tid)))
        else:
            row += tree.name_of(tid)
        out.append(row + b"\n")
    if not expand:
        p = f32(float(_ratio(virus_reads, total)) * 100.0) if virus_reads > 0 else f32(0.0)
        out.append(label + b"\t" + _fmt(p) + b"\t%d\t%d\tViruses\n" % (virus_reads, VIRUSES))
    p = f32(float(_ratio(above, total)) * 100.0) if above > 0 else f32(0.0)
    out.append(label + b"\t" + _fmt(p) + b"\t%d\tNA\tcannot be assigned to a (non-viral) %s\n" % (above, rank))
    if min_count > 0:
        out.append(label + b"\t" + _fmt(float(_ratio(below_count, total)) * 100.0) + b"\t%d\tNA\tbelong to a (non-viral) %s having less than %d reads\n" % (below_count, rank, min_count))
    if min_percent > 0.0:
        out.append(label + b"\t" + _fmt(float(_ratio(below_percent, total)) * 100.0) +
                   b"\t%d\tNA\tbelong to a (non-viral) %s with less than %s%% of all reads\n" % (below_percent, rank, ("%g" % float(min_percent)).encode()))
    out.append(label + b"\t" + _fmt(float(_ratio(unclassified, total + unclassified if filt else total)) * 100.0) + b"\t%d\tNA\tunclassified\n" % unclassified)
    return b"".join(out)


HEADER = b"file\tpercent\treads\ttaxon_id\ttaxon_name\n"


def table_of_files(tree, files, opt):
    """the whole output file: files is a list of (label, text)"""
    out = HEADER
    for label, text in files:
        totals, entries = tally(tree, [text])
        out += table_rows(tree, entries, totals, opt, label)
    return out
