"""What kaiju2krona makes of output texts, restated from the rules (kaiju2krona.cpp:116-190 of the reference) on bytes and
with strings, as the tool has them: the counts per line are those of tests/table_expect.py (kaiju_amd/csrc/kj_tally.h), the
lineage lines those of kaiju_amd/csrc/kj_krona.h.  tests/test_krona_expect_golden.py pins this file to the reference tool's own
outputs under tests/golden/krona/ (as sorted lines: the tool's order is that of a hash map); every other test of the Krona
text compares with it byte for byte, in the order of the library: ascending slot of the table that
kaiju_amd/csrc/taxon_names.cpp builds, the Unclassified line last.

ranks: the text of -l, None: no list (an empty text is a list that holds nothing)."""
import table_expect as te

INFO_FIELDS = ("text_bytes", "written_bytes", "n_lines", "n_written", "n_unnamed_taxa", "n_unnamed_reads", "n_unclassified", "overflow")
M64 = 2 ** 64 - 1


def hash_id(v):
    """kjn::hash_id"""
    v ^= v >> 33
    v = v * 0xff51afd7ed558ccd & M64
    v ^= v >> 33
    v = v * 0xc4ceb9fe1a85ec53 & M64
    v ^= v >> 33
    return v & 0xffffffff


def slots_of(tree):
    """{id: slot} of the loader's table: the nodes in file order, linear probing"""
    cap = 16
    while cap < 2 * len(tree.nodes) + 2:
        cap <<= 1
    taken, where = set(), {}
    for tid in tree.nodes:
        s = hash_id(tid) & (cap - 1)
        while s in taken:
            s = (s + 1) & (cap - 1)
        taken.add(s)
        where[tid] = s
    return where


def split_ranks(ranks):
    return None if ranks is None else {r for r in (ranks if isinstance(ranks, bytes) else ranks.encode()).split(b",") if r}


def lineage(tree, tid, listed):
    """the names of the line of node tid, as the tool collects them"""
    nodes, names = tree.nodes, tree.names
    keep = lambda t: listed is None or (t in nodes and nodes[t][1] in listed)
    out = []
    if nodes[tid][0] in names and keep(tid):
        out.append(names[tid])
    while tid in nodes and tid != nodes[tid][0]:
        parent = nodes[tid][0]
        if parent in names and keep(parent):
            out.insert(0, names[parent])
        tid = parent
    return out


def direct_of(tree, texts):
    """texts added one behind the other, each of them final: ({taxon: reads}, unclassified lines)"""
    direct, totals = {}, {}
    for text in texts:
        info, more = te.count_text(tree, text, final=True)
        te.add_counts(totals, direct, info, more)
    return direct, totals.get("n_unclassified", 0)


def lines_of(tree, direct, n_unclassified=0, unclassified=False, ranks=None):
    """(lines in the library's order, unnamed taxa, their reads)"""
    listed = split_ranks(ranks)
    where = slots_of(tree)
    lines, taxa, reads = [], 0, 0
    for tid in sorted((t for t in direct if t in tree.nodes and direct[t] > 0), key=where.get):
        if tid not in tree.names:
            taxa, reads = taxa + 1, reads + direct[tid]
            continue
        lines.append(b"%d" % direct[tid] + b"".join(b"\t" + n for n in lineage(tree, tid, listed)) + b"\n")
    if unclassified and n_unclassified > 0:
        lines.append(b"%d\tUnclassified\n" % n_unclassified)
    return lines, taxa, reads


def expected(tree, direct, n_unclassified=0, unclassified=False, ranks=None, out_cap=None):
    """what a call gives: {"text": the whole text, "written": the lines that fit out_cap, "info": the fields of the info}"""
    lines, taxa, reads = lines_of(tree, direct, n_unclassified, unclassified, ranks)
    text = b"".join(lines)
    cap = len(text) if out_cap is None else out_cap
    fit, at = 0, 0
    for line in lines:
        if at + len(line) > cap:
            break
        at, fit = at + len(line), fit + 1
    info = dict(text_bytes=len(text), written_bytes=at, n_lines=len(lines), n_written=fit, n_unnamed_taxa=taxa, n_unnamed_reads=reads,
                n_unclassified=n_unclassified if unclassified else 0, overflow=1 if len(text) > cap else 0)
    return {"text": text, "written": text[:at], "info": info}


def text_of(tree, texts, unclassified=False, ranks=None):
    direct, n_u = direct_of(tree, texts)
    return expected(tree, direct, n_u, unclassified, ranks)["text"]


def sorted_lines(text):
    assert text == b"" or text.endswith(b"\n")
    return sorted(text.split(b"\n")[:-1])
