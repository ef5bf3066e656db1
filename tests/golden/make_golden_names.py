"""Golden files of the column of kaiju-addTaxonNames:  python tests/golden/make_golden_names.py

The unmodified reference tool is compiled by the pattern rules of oracle/Makefile (its objects and those of bwt/) and linked
into oracle/_ref/kaiju-addTaxonNames (git-ignored); oracle/_ref/kaiju is built by the same Makefile.  Only data is written,
under tests/golden/names/:

  deep/     nodes.dmp, names.dmp, in.tsv: a synthetic tree from a fixed seed with every quirk of the two parsers and of the
            walk, and the tool's outputs, gzip'ed: out_name.tsv.gz, out_path.tsv.gz (-p), out_ranks.tsv.gz (-r RANKS_DEEP),
            out_path_u.tsv.gz (-u -p)
  golden/   names.dmp for tests/golden/nodes.dmp with two gaps (a taxon reads hit, an inner node), and the reference kaiju
            without -v (MEM and Greedy, single and paired) on the committed reads, piped through the tool in the three modes:
            <mode>[_pe].<name|path|ranks>.tsv.gz (-r RANKS_GOLDEN)"""
import gzip
import os
import random
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
TOOL = os.path.join(REF, "kaiju-addTaxonNames")
OUT = os.path.join(HERE, "names")
RANKS_DEEP = "genus,species,phylum,genus"
RANKS_GOLDEN = "family,genus,species"
BWT = ["_ref/obj/bwt/%s.o" % f for f in ("bwt", "compactfmi", "sequence", "suffixArray")]


def build_tool():
    objs = ["_ref/obj/kaiju-addTaxonNames.o", "_ref/obj/util.o"] + BWT
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")] + objs + ["_ref/kaiju"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["g++", "-o", TOOL] + [os.path.join(ROOT, "oracle", o) for o in objs] + ["-lpthread", "-lz"], check=True)


def tool(nodes, names, inp, out, *args):
    subprocess.run([TOOL, "-t", nodes, "-n", names, "-i", inp, "-o", out] + list(args), check=True, stderr=subprocess.DEVNULL)
    with open(out, "rb") as f, open(out + ".gz", "wb") as g, gzip.GzipFile(fileobj=g, mode="wb", mtime=0, filename="") as z:
        z.write(f.read())                              # (the outputs are kept gzip'ed, byte for byte what the tool wrote)
    os.remove(out)
    print(out + ".gz", os.path.getsize(out + ".gz"))


def node(i, parent, rank):
    return b"%d\t|\t%d\t|\t%s\t|\n" % (i, parent, rank)


def name(i, text, kind=b"scientific name"):
    return b"%d\t|\t%s\t|\t\t|\t%s\t|\n" % (i, text, kind)


def deep():
    rng = random.Random(20240607)
    d = os.path.join(OUT, "deep")
    os.makedirs(d, exist_ok=True)
    nodes, names, taxa = [], [], []
    nodes.append(node(1, 1, b"no rank"))                               # the root: its own parent
    names.append(name(1, b"root"))
    # a lineage over the taxa the format inputs use (tests/format_inputs.py: TAXA), a node without a name in its middle
    lineage = [9, 10, 99, 100, 999, 9999, 99999, 999999, 9999999, 99999999, 999999999]
    ranks = [b"phylum", b"no rank", b"class", b"genus", b"species", b"no rank", b"strain", b"genus", b"clade", b"species", b"no rank"]
    for k, (i, r) in enumerate(zip(lineage, ranks)):
        nodes.append(node(i, lineage[k - 1] if k else 1, r))
        if i != 99999:
            names.append(name(i, b"Lineage %d" % i))
    # a chain 40 deep below it: genus twice, a 300-byte name near its top, a 1-byte name, spaces and UTF-8
    chain_ranks = [b"superkingdom", b"phylum", b"class", b"order", b"family", b"genus", b"no rank", b"species group", b"species", b"subspecies"]
    for k in range(40):
        i = 1000 + k
        nodes.append(node(i, 1000 + k - 1 if k else 999999999, chain_ranks[k % 10]))
    names.append(name(1000, b"X"))
    names.append(name(1001, "Čandidatus Ünicode bacterium 木".encode()))
    names.append(name(1002, b"L" * 300))
    names.append(name(1003, b"Outer|x"))                               # a '|' inside: the name is "Outer"
    names.append(name(1004, b"fake scientific name of 1004", b"synonym"))   # a synonym line that holds the words comes first and wins
    names.append(name(1004, b"Real 1004"))
    names.append(name(1005, b"First of two"))
    names.append(name(1005, b"Second of two"))
    names.append(name(1006, b"common 1006", b"common name"))           # no scientific name at all: a node without a name in mid-lineage
    for k in range(7, 40):
        if k != 21:
            names.append(name(1000 + k, b"Chain node %d with spaces" % k))
    # leaves and oddities
    nodes.append(node(7, 1, b"species"));            names.append(name(7, b"S"))
    nodes.append(node(12, 7, b"subspecies"))                           # a leaf without a name
    nodes.append(node(77, 76, b"genus"));            names.append(name(77, b"Orphan genus"))       # the parent is no node
    nodes.append(node(78, 77, b"species"));          names.append(name(78, b"Orphan species"))
    nodes.append(b"4000\t|\t1000\t|\tSPECIES\t|\n");  names.append(name(4000, b"Dropped by its rank"))   # no lower-case letter: no node
    nodes.append(b"4001\t|\t1000\t|\tSPECIES\t|\tembl\t|\n"); names.append(name(4001, b"Rank embl"))
    nodes.append(node(4002, 4000, b"species"));      names.append(name(4002, b"Child of the dropped"))
    nodes.append(node(1002, 1, b"species"))                            # a second line for an id: the first wins
    nodes.append(node(10 ** 19, 1, b"phylum"));      names.append(name(10 ** 19, b"Twenty digits"))
    nodes.append(node(2 ** 32, 10 ** 19, b"genus"))                    # no name, twenty-digit parent
    nodes.append(node(2 ** 63, 2 ** 32, b"species")); names.append(name(2 ** 63, b"Below a generated name"))
    # lines the parsers must skip
    nodes += [b"abc\n", b"55\n", b"56\t|\t\n", b"57\t|\t1\t|\t\n", b"99999999999999999999999\t|\t1\t|\tspecies\t|\n", b"58\t|\t99999999999999999999999\t|\tspecies\t|\n", b"\n"]
    names += [b"no digits but scientific name\n", b"scientific name 59\n", b"60\t|\t|\t|\n", name(61, b"not in the tree"), b"\n",
              b"99999999999999999999999\t|\ttoo large\t|\t\t|\tscientific name\t|\n"]
    # a bush from the seed
    bush_ranks = [b"no rank", b"phylum", b"class", b"order", b"family", b"genus", b"species", b"clade"]
    ids = [1, 9, 10, 1000, 1010, 1039, 7, 77]
    for k in range(60):
        i = 5000 + k
        nodes.append(node(i, rng.choice(ids), rng.choice(bush_ranks)))
        if rng.random() < 0.85:
            names.append(name(i, bytes(rng.choice(b"abcdefghij klmnop") for _ in range(rng.randrange(1, 40)))))
        ids.append(i)
    with open(os.path.join(d, "nodes.dmp"), "wb") as f:
        f.write(b"".join(nodes))
    with open(os.path.join(d, "names.dmp"), "wb") as f:
        f.write(b"".join(names))
    taxa = [1, 12, 77, 78, 4000, 4001, 4002, 61, 777777, 10 ** 19, 2 ** 32, 2 ** 63, 7] + lineage + [1000 + k for k in range(40)] + [5000 + k for k in range(60)]
    lines = []
    for k, t in enumerate(taxa + [rng.choice(taxa) for _ in range(60)]):
        lines.append(b"C\tread%d%s\t%d\n" % (k, b"x" * rng.randrange(0, 30), t))
        if k % 9 == 4:
            lines.append(b"U\tunclassified%d\t0\n" % k)
        if k == 50:
            lines.append(b"\n")
    with open(os.path.join(d, "in.tsv"), "wb") as f:
        f.write(b"".join(lines))
    a = [os.path.join(d, f) for f in ("nodes.dmp", "names.dmp", "in.tsv")]
    tool(*a, os.path.join(d, "out_name.tsv"))
    tool(*a, os.path.join(d, "out_path.tsv"), "-p")
    tool(*a, os.path.join(d, "out_ranks.tsv"), "-r", RANKS_DEEP)
    tool(*a, os.path.join(d, "out_path_u.tsv"), "-u", "-p")


def golden():
    d = os.path.join(OUT, "golden")
    os.makedirs(d, exist_ok=True)
    nodes = os.path.join(HERE, "nodes.dmp")
    ids = [int(l.split(b"\t")[0]) for l in open(nodes, "rb") if l.strip()]
    gaps = (100005, 1003)                                              # a species many reads hit; a genus in the middle of lineages
    with open(os.path.join(d, "names.dmp"), "wb") as f:
        for i in ids:
            if i not in gaps:
                f.write(name(i, b"Taxon %d name" % i))
    tmp = os.path.join(REF, "names_tmp.tsv")
    for mode in ("mem", "greedy"):
        for pe in (False, True):
            cmd = [os.path.join(REF, "kaiju"), "-t", nodes, "-f", os.path.join(HERE, "db.fmi"), "-a", mode, "-z", "1", "-o", tmp]
            cmd += ["-i", f"{HERE}/pairs_1.fq", "-j", f"{HERE}/pairs_2.fq"] if pe else ["-i", f"{HERE}/reads.fq"]
            subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
            for kind, args in (("name", []), ("path", ["-p"]), ("ranks", ["-r", RANKS_GOLDEN])):
                tool(nodes, os.path.join(d, "names.dmp"), tmp, os.path.join(d, "%s%s.%s.tsv" % (mode, "_pe" if pe else "", kind)), *args)
    os.remove(tmp)


if __name__ == "__main__":
    build_tool()
    deep()
    golden()
