"""Golden files of kaiju-convertRefSeq:  python tests/golden/make_golden_refseq.py

The unmodified reference tool is compiled by the pattern rules of oracle/Makefile (its object, util.o, Config.o and those of
bwt/) and linked into oracle/_ref/kaiju-convertRefSeq (git-ignored), exactly as tests/golden/make_golden_convert.py builds its
tool.  Only data is written, under tests/golden/refseq/:

  nodes.dmp, merged.dmp   the small tree of tests/golden/convert: a merged id that maps to a node, one that maps to none
  list.txt                the -l file: ids with text around them, a line without digits, an id that is no node
  map.tsv                 the -g file, two columns: every map rule of kaiju_amd/csrc/kj_convert.h ("kaiju-convertRefSeq") at
                          least once - the comments beside the lines of MAP say which
  faa.txt                 the text of standard input: every header rule at least once
  faa_none.txt            a text of which nothing is kept
  out_<set>.txt           the tool on faa.txt for every option set of SETS;  none_default.txt: on faa_none.txt"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
TOOL = os.path.join(REF, "kaiju-convertRefSeq")
OUT = os.path.join(HERE, "refseq")
BWT = ["_ref/obj/bwt/%s.o" % f for f in ("bwt", "compactfmi", "sequence", "suffixArray")]

SETS = {
    "default": [],
    "a": ["-a"],
    "l": ["-l", "list.txt"],
    "al": ["-a", "-l", "list.txt"],
}

NODES = [(1, 1), (131567, 1), (2, 131567), (2157, 131567), (10239, 1), (2759, 131567), (1224, 2), (1236, 1224), (561, 1236),
         (562, 561), (564, 561), (1239, 2), (1386, 1239), (1423, 1386), (9606, 2759), (28384, 1), (10240, 10239), (562, 1)]
MERGED = [(666, 562), (777, 4242), (666, 9606)]
LIST = b"561\n  1386 a genus\nno digits here\n\n99999\n2759x12\n"
MAP = (b"accession.version\ttaxid\n"
       b"WP_1.1\t562\n"                                     # a WP_ line whose taxon is a node
       b"NP_1.1\t562\n"                                     # not WP_
       b"XP_1.1\t564\n"
       b"wp_1.1\t562\n"                                     # the three bytes are case-sensitive
       b"W\t562\n"                                          # fewer than 3 bytes in front of the tab: "W\t5" is not "WP_"
       b"WP\t562\n"
       b"WP_notab\n"                                        # no tab: nothing (kaiju-convertNR takes such a line as a key)
       b"WP_\t564\n"                                        # the key "WP_"
       b"WP_\t666\n"                                        # merged: the key "WP"
       b"WP_5.1\t666\n"                                     # merged to 562: the key is "WP_5."
       b"WP_6.1\t777\n"                                     # merged to 4242, no node: inserts nothing
       b"WP_6.1\t1236\n"                                    # ... so this line is the first that inserts WP_6.1
       b"WP_7.1\t55555\n"                                   # neither node nor merged
       b"WP_8.1\t0\n"                                       # taxon 0: nothing
       b"WP_8.1\t10240\n"
       b"WP_9.1\t99999999999999999999999\n"                 # overflow: ULONG_MAX
       b"WP_9.1\t-1\n"                                      # ULONG_MAX
       b"WP_9.1\t+561\n"
       b"WP_B1.1\t  2157\n"                                 # blanks in front of the digits
       b"WP_B8.1\t564abc\n"                                 # digits, then letters
       b"WP_B5.1\t2\r\n"                                    # '\r' behind the digits
       b"WP_4C\tWP_4C.1\t562\t9\n"                          # four columns: strtoul("WP_4C.1...") is 0
       b"WP_1.1\t9606\n"                                    # loses against the first line of WP_1.1
       b"WP_12\t562\n"                                      # a full key ...
       b"WP_123\t666\n"                                     # ... in front of the truncated key that is equal to it: loses
       b"WP_345\t666\n"                                     # a truncated key "WP_34": 562 ...
       b"WP_34\t9606\n"                                     # ... in front of the full key that is equal to it: loses
       b"WP_K 1\t1423\n"                                    # a key that holds a space: no header can name it
       b"\n"
       b"WP_H.1\t9606\n"                                    # outside the default list, inside list.txt
       b"WP_R.1\t28384\n"                                   # a child of the root: in no list
       b"WP_R1\t1\n"                                        # the root itself
       b"WP_\x011.1\t10240\n"                               # '\x01' in the accession
       b"WP_B2.1\t-18446744073709551054\n"                  # 2^64 - that = 562
       b"WP_LAST.1\t1386")                                  # the last line has no '\n'
FAA = (b"MKVNOHEADER\n"                                     # sequence lines in front of the first header
       b"\n"
       b">WP_1.1 protein one\n"
       b"MKVLA\n"
       b"\n"
       b"ARNDCQEGHILKMFPSTWYV\n"
       b">WP_1.1\n"                                         # a header without a space: dropped without a lookup
       b"AAAA\n"
       b"> x\n"                                             # an accession of zero bytes
       b"CCCC\n"
       b">WP_1.1 \n"                                        # the only space is the last byte
       b"DDDD\n"
       b">WP_\x011.1 x01 in the accession\n"
       b"EEEE\n"
       b">ZZ.1 unknown\x01WP_1.1 known\n"                   # '\x01' behind the space: the second accession does not count
       b"FFFF\n"
       b">WP_5.1 the truncated key with its last byte\n"    # not found
       b"GGGG\n"
       b">WP_5. and without it\n"                           # 562
       b"HHHH\n"
       b">WP_12 the full key won\n"                         # 562
       b"IIII\n"
       b">WP_123 x\n"
       b"KKKK\n"
       b">WP_34 the truncated key won\n"                    # 562, not 9606
       b"LLLL\n"
       b">WP_345 x\n"
       b"MMMM\n"
       b">WP two bytes\n"                                   # 562
       b"NNNN\n"
       b">WP_ three bytes\n"                                # 564
       b"PPPP\n"
       b">WP_H.1 human\n"                                   # 9606: only with list.txt
       b"HIK\n"
       b">WP_R1 the root itself\n"                          # taxon 1 never keeps a record
       b"STV\n"
       b">WP_R.1 a child of the root\n"
       b"WYA\n"
       b">WP_6.1 the second line inserted it\n"             # 1236
       b"QQQQ\n"
       b">WP_7.1 nothing\n"
       b"RRRR\n"
       b">WP_8.1 virus\n"                                   # 10240
       b"SSSS\n"
       b">WP_9.1 signed\n"                                  # 561
       b"TTTT\n"
       b">WP_B1.1 archaeon\n"                               # 2157
       b"VVVV\n"
       b">WP_B8.1 digits then letters\n"                    # 564
       b"WWWW\n"
       b">WP_B5.1 cr in the map\n"                          # 2
       b"YYYY\n"
       b">WP_4C four columns\n"
       b"AAAC\n"
       b">WP_4C.1 four columns\n"
       b"AAAD\n"
       b">WP_K 1 a key with a space\n"                      # looks up "WP_K"
       b"AAAE\n"
       b">WP_B2.1 negative\n"                               # 562
       b"AAAF\n"
       b">NP_1.1 not WP_\n"
       b"AAAG\n"
       b">wp_1.1 lower case\n"
       b"AAAH\n"
       b">WP_notab x\n"
       b"AAAI\n"
       b">WP_1.1 lower case and other bytes\r\n"
       b"mkvACDxX*-BJOUZ\r\n"
       b">WP_1.1 a record without letters\n"
       b"xx**--\n"
       b">WP_1.1 no sequence lines\n"
       b">WP_LAST.1 the last line has no line end\n"
       b"NNNN")
FAA_NONE = (b">WP_H.1 human\n"
            b"HIK\n"
            b">nothing\n"
            b"AAA\n"
            b">WP_R1 root\n"
            b"CCC\n")


def blast_objects():
    """the objects of BLAST_C in oracle/Makefile: Config.o of the tool refers to the SEG parameters"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        text = f.read().replace("\\\n", " ")
    line = [l for l in text.split("\n") if l.startswith("BLAST_C :=")][0]
    return ["_ref/obj/blast/%s.o" % c[:-2] for c in line.split(":=")[1].split()]


def build_tool():
    objs = ["_ref/obj/kaiju-convertRefSeq.o", "_ref/obj/util.o", "_ref/obj/Config.o"] + BWT + blast_objects()
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")] + objs, check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["g++", "-o", TOOL] + [os.path.join(ROOT, "oracle", o) for o in objs] + ["-lpthread", "-lz"], check=True)


def write(name, data):
    with open(os.path.join(OUT, name), "wb") as f:
        f.write(data)


def run(faa, out, args):
    with open(os.path.join(OUT, faa), "rb") as f:
        subprocess.run([TOOL, "-t", "nodes.dmp", "-m", "merged.dmp", "-g", "map.tsv", "-o", out] + args, check=True, cwd=OUT, stdin=f,
                       stderr=subprocess.DEVNULL, timeout=60)
    print(os.path.join(OUT, out), os.path.getsize(os.path.join(OUT, out)))


if __name__ == "__main__":
    build_tool()
    os.makedirs(OUT, exist_ok=True)
    write("nodes.dmp", b"".join(b"%d\t|\t%d\t|\tno rank\t|\n" % p for p in NODES))
    write("merged.dmp", b"".join(b"%d\t|\t%d\t|\n" % p for p in MERGED))
    write("list.txt", LIST)
    write("map.tsv", MAP)
    write("faa.txt", FAA)
    write("faa_none.txt", FAA_NONE)
    for name, args in SETS.items():
        run("faa.txt", "out_%s.txt" % name, args)
    run("faa_none.txt", "none_default.txt", [])
