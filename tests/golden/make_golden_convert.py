"""Golden files of kaiju-convertNR:  python tests/golden/make_golden_convert.py

The unmodified reference tool is compiled by the pattern rules of oracle/Makefile (its object, util.o, Config.o and those of
bwt/) and linked into oracle/_ref/kaiju-convertNR (git-ignored), exactly as tests/golden/make_golden_krona.py builds its tool.
Only data is written, under tests/golden/convert/:

  nodes.dmp, merged.dmp   a small tree (a second line of id 562 that loses), a merged id, one that is no node, a second line of one
  list.txt                the -l file: ids with text around them, a line without digits, an id that is no node
  map.tsv                 the -g file: merged ids, duplicates whose first line inserts nothing, overflow, signs, white space,
                          lines with zero and one tab, a key of zero bytes, a key that holds \\x01, a last line without '\\n'
  excl.txt                the -e file
  nr.txt                  the nr-style text: every rule of kaiju_amd/csrc/kj_convert.h at least once
  nr_none.txt             a text of which nothing is kept
  out_<set>.txt           the tool on nr.txt for every option set of SETS;  none_default.txt: on nr_none.txt"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
TOOL = os.path.join(REF, "kaiju-convertNR")
OUT = os.path.join(HERE, "convert")
BWT = ["_ref/obj/bwt/%s.o" % f for f in ("bwt", "compactfmi", "sequence", "suffixArray")]

SETS = {
    "default": [],
    "a": ["-a"],
    "l": ["-l", "list.txt"],
    "e": ["-e", "excl.txt"],
    "ale": ["-a", "-l", "list.txt", "-e", "excl.txt"],
}

NODES = [(1, 1), (131567, 1), (2, 131567), (2157, 131567), (10239, 1), (2759, 131567), (1224, 2), (1236, 1224), (561, 1236),
         (562, 561), (564, 561), (1239, 2), (1386, 1239), (1423, 1386), (9606, 2759), (28384, 1), (10240, 10239), (562, 1)]
MERGED = [(666, 562), (777, 4242), (666, 9606)]
LIST = b"561\n  1386 a genus\nno digits here\n\n99999\n2759x12\n"
MAP = (b"accession\taccession.version\ttaxid\tgi\n"
       b"A1\tA1.1\t562\t1\n"
       b"A2\tA2.1\t564\t2\n"
       b"A3\tA3.1\t1423\t3\n"
       b"A4\tA4.1\t9606\t4\n"
       b"A5\tA5.1\t666\t5\n"                                # merged to 562
       b"A6\tA6.1\t777\t6\n"                                # merged to 4242, no node: inserts nothing
       b"A6\tA6.1\t1236\t7\n"                               # ... so this line is the first that inserts A6.1
       b"A1\tA1.1\t9606\t8\n"                               # loses against the first line of A1.1
       b"A7\tA7.1\t55555\t9\n"                              # neither node nor merged
       b"A8\tA8.1\t99999999999999999999999\t10\n"           # overflow: ULONG_MAX, skipped
       b"A8\tA8.1\t10240\t11\n"
       b"A9\tA9.1\t-1\t12\n"                                # ULONG_MAX, skipped
       b"A9\tA9.1\t+561\t13\n"
       b"B1\tB1.1\t  2157\t14\n"
       b"B2\tB2.1\t-18446744073709551054\t15\n"             # 2^64 - that = 562
       b"561\n"                                             # no tab: the key is the line, the taxon its number
       b"1386\tK1\n"                                        # one tab: the key is what follows it, the taxon the line's number
       b"X9\tY9\n"                                          # ... 0, no node
       b"\n"
       b"B3\tB3.1\t28384\t16\n"
       b"B4\tB4.1\t10239\t\n"
       b"V1\tV\x011.1\t10240\t17\n"
       b"Q0\t\t1423\t18\n"                                  # a key of zero bytes
       b"B5\tB5.1\t2\t19\r\n"
       b"B7\tB7.1\t\n"                                      # tab 2 is the last byte: 0
       b"B8\tB8.1\t564abc\t20\n"
       b"LONGKEY\tNP_0123456789012345678901234567890.12\t562\t21\n"
       b"B6\tB6.1\t1")                                      # the last line has no '\n'
EXCL = b"E1.1\n\nA4.1\n"
NR = (b"MKVNOHEADER\n"
      b"\n"
      b">A1.1 protein one\n"
      b"MKVLA\n"
      b"\n"
      b"ARNDCQEGHILKMFPSTWYV\n"
      b">A1.1 p\x01A2.1 q\n"                                  # siblings: 561
      b"mkvACDxX*-BJOUZ\r\n"
      b">A1.1 p\x01A6.1 q r s\n"                              # a node and its ancestor: 1236
      b"ACD\n"
      b">A3.1 x\x01A1.1 y\n"                                  # 2: in the default list, outside list.txt above members inside it
      b"EFG\n"
      b">A4.1 human\n"                                        # 9606: only with list.txt (and not with excl.txt)
      b"HIK\n"
      b">A1.1 a\x01A4.1 b\n"                                  # 131567
      b"LMN\n"
      b">A1.1 a\x01B3.1 b\n"                                  # 1
      b"PQR\n"
      b">B6.1 root itself\n"
      b"STV\n"
      b">ZZ.1 unknown\x01A2.1 known\n"                        # -a: the first accession has no taxon
      b"WYA\n"
      b">V\x011.1 x01 in the accession\x01\x01A1.1 z\n"       # an accession with \x01 inside; the entry "\x01A1.1"
      b"ACDE\n"
      b">A1.1 first\x01A4.1\n"                                # the last entry has no space: no entry
      b"FGHI\n"
      b">E1.1 excluded first\x01A1.1 b\n"
      b"KLMN\n"
      b">A1.1 a\x01A2.1 b\x01E1.1 excluded last\n"
      b"PQRS\n"
      b">\n"                                                  # a bare '>'
      b"TVWY\n"
      b">A5.1 merged\n"
      b"xx**--\n"                                             # a record without letters
      b">A7.1 nothing\n"
      b"AAAA\n"
      b">A8.1 virus\n"
      b"CCCC\n"
      b">A9.1 signed\x01B1.1 archaeon\x01B2.1 negative\n"     # 561, 2157, 562: 131567
      b"DDDD\n"
      b">B1.1 archaeon\n"
      b"EEEE\n"
      b">B2.1 negative\n"
      b"FFFF\n"
      b">561 no tab\x01K1 one tab\x01Y9 one tab, zero\n"      # 561, 1386: 2
      b"GGGG\n"
      b">B4.1 viruses\x01B7.1 zero\n"
      b"HHHH\n"
      b"> the accession of zero bytes\n"                      # 1423
      b"IIII\n"
      b">B5.1 cr in the map\x01B8.1 digits then letters\n"    # 2, 564: 2
      b"KKKK\n"
      b">NP_0123456789012345678901234567890.12 a long accession\n"
      b"LLLL\n"
      b">A2.1  two spaces\x01 \x01A3.1 z\r\n"                 # the entry " ": the key of zero bytes
      b"MMMM\n"
      b">A1.1 no sequence lines\n"
      b">A2.1 the last line has no line end\n"
      b"NNNN")
NR_NONE = (b">A4.1 human\n"
           b"HIK\n"
           b">nothing\n"
           b"AAA\n"
           b">B6.1 root\n"
           b"CCC\n")


def blast_objects():
    """the objects of BLAST_C in oracle/Makefile: Config.o of the tool refers to the SEG parameters"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        text = f.read().replace("\\\n", " ")
    line = [l for l in text.split("\n") if l.startswith("BLAST_C :=")][0]
    return ["_ref/obj/blast/%s.o" % c[:-2] for c in line.split(":=")[1].split()]


def build_tool():
    objs = ["_ref/obj/kaiju-convertNR.o", "_ref/obj/util.o", "_ref/obj/Config.o"] + BWT + blast_objects()
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")] + objs, check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["g++", "-o", TOOL] + [os.path.join(ROOT, "oracle", o) for o in objs] + ["-lpthread", "-lz"], check=True)


def write(name, data):
    with open(os.path.join(OUT, name), "wb") as f:
        f.write(data)


def run(nr, out, args):
    subprocess.run([TOOL, "-t", "nodes.dmp", "-m", "merged.dmp", "-g", "map.tsv", "-i", nr, "-o", out] + args, check=True, cwd=OUT,
                   stderr=subprocess.DEVNULL, timeout=60)
    print(os.path.join(OUT, out), os.path.getsize(os.path.join(OUT, out)))


if __name__ == "__main__":
    build_tool()
    os.makedirs(OUT, exist_ok=True)
    write("nodes.dmp", b"".join(b"%d\t|\t%d\t|\tno rank\t|\n" % p for p in NODES))
    write("merged.dmp", b"".join(b"%d\t|\t%d\t|\n" % p for p in MERGED))
    write("list.txt", LIST)
    write("map.tsv", MAP)
    write("excl.txt", EXCL)
    write("nr.txt", NR)
    write("nr_none.txt", NR_NONE)
    for name, args in SETS.items():
        run("nr.txt", "out_%s.txt" % name, args)
    run("nr_none.txt", "none_default.txt", [])
