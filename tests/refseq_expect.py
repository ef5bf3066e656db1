"""A model of kaiju-convertRefSeq in plain Python: the rules in kaiju_amd/csrc/kj_convert.h ("kaiju-convertRefSeq"), one function per
rule; what the tool shares with kaiju-convertNR (getline, strtoul, the include walk, the letters) is tests/convert_expect.py.
tests/test_refseq_expect_golden.py checks it against the files the unmodified tool wrote; the emulation and the GPU tests check
the device code against it."""
import os

import convert_expect as ce

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "refseq")
ULONG_MAX, MISS, AA, DEFAULT_INCLUDE, INFO_FIELDS = ce.ULONG_MAX, ce.MISS, ce.AA, ce.DEFAULT_INCLUDE, ce.INFO_FIELDS
SETS = {"default": (False, False), "a": (True, False), "l": (False, True), "al": (True, True)}      # -a, -l


def golden(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def map_line(line, nodes, merged):
    """(key, taxon) of a non-empty line of the map file, or None where it inserts nothing"""
    t = line.find(b"\t")
    if t < 0 or line[:3] != b"WP_":
        return None
    taxon = ce.strtoul(line[t + 1:])
    if taxon == ULONG_MAX or taxon == 0:
        return None
    if taxon in nodes:
        return line[:t], taxon
    taxon = merged.get(taxon)
    if taxon is None or taxon not in nodes:
        return None
    return line[:t - 1], taxon                               # substr(0, start - 1): the accession loses its last byte


class Model:
    def __init__(self, nodes, merged):
        self.nodes, self.merged = nodes, merged
        self.map, self.lines, self.no_insert, self.duplicates = {}, 0, 0, 0

    def add_text(self, data, first_block=True):
        for k, line in enumerate(ce.getlines(data)):
            if (first_block and k == 0) or not line:
                continue
            self.lines += 1
            got = map_line(line, self.nodes, self.merged)
            if got is None:
                self.no_insert += 1
            elif got[0] in self.map:
                self.duplicates += 1
            else:
                self.map[got[0]] = got[1]
        return self

    def lookup(self, key):
        return self.map.get(key, MISS)


def convert(nodes, include, amap, text, add_acc=False, out_cap=None):
    """what the converter gives for a block: {"text", "written", "info", "records"} - records: the bytes of every kept record"""
    info = dict.fromkeys(INFO_FIELDS, 0)
    lines = ce.getlines(text)
    info["n_lines"] = len(lines)
    records, cur = [], None
    for line in lines:
        if not line:
            continue
        if line[:1] == b">":
            info["n_records"] += 1
            cur = None
            end = line.find(b" ", 1)
            t = 0
            if end >= 0:
                info["n_entries"] += 1
                t = amap.get(line[1:end], 0)
                if t > 0 and t != MISS:
                    info["n_hits"] += 1
                else:
                    t = 0
            if not t:
                info["dropped_no_taxon"] += 1
            elif not ce.included(nodes, include, t):
                info["dropped_not_included"] += 1
            else:
                info["n_kept"] += 1
                cur = [b">" + (line[1:end] + b"_" if add_acc else b"") + b"%d\n" % t]
                records.append(cur)
        elif cur is not None:
            cur.append(bytes(b for b in line if b in AA))
    records = [b"".join(r) + b"\n" for r in records]
    full = b"".join(records)
    info["text_bytes"] = len(full)
    written = full
    if out_cap is not None and len(full) > out_cap:
        info["overflow"] = 1
        at = 0
        for r in records:
            if at + len(r) > out_cap:
                break
            at += len(r)
        written = full[:at]
    info["written_bytes"] = len(written)
    return {"text": full, "written": written, "info": info, "records": records}


file_of = ce.file_of


class Fixture:
    """the files of tests/golden/refseq"""

    def __init__(self):
        self.nodes = ce.parse_pairs(golden("nodes.dmp"))
        self.merged = ce.parse_pairs(golden("merged.dmp"))
        self.pairs = ce.merged_pairs(golden("merged.dmp"))
        self.model = Model(self.nodes, self.merged).add_text(golden("map.tsv"))
        self.listed = ce.parse_list(golden("list.txt"), self.nodes)
        self.faa, self.faa_none = golden("faa.txt"), golden("faa_none.txt")

    def expected(self, name, text=None, out_cap=None):
        a, l = SETS[name]
        return convert(self.nodes, self.listed if l else DEFAULT_INCLUDE, self.model.map, self.faa if text is None else text, add_acc=a, out_cap=out_cap)
