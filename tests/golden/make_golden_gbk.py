"""Golden files of kaiju-gbk2faa:  python tests/golden/make_golden_gbk.py

Runs the unmodified util/kaiju-gbk2faa.pl of the reference (KAIJU_REFERENCE, default /root/reference) with the system's perl;
nothing is compiled.  Only data is written, under tests/golden/gbk/: per fixture <name>.gbk (the input, written from the bytes
below) and <name>.faa (the file the script wrote), and status.txt with the script's exit status per fixture.

  rules         every rule of kaiju_amd/csrc/kj_gbk.h at least once (the comments beside the lines say which)
  record        a plain record: LOCUS, source, two CDS, an ORIGIN block
  crlf          "\\r\\n" line ends: '\\r' is a byte of the line
  nopid         a translation in front of any protein id: ">_5"
  tail_open     a last line without '\\n' inside a translation;  tail_closed: one that closes it
  notaxon       the first translation has no taxon: the script dies (status 255), the file is empty
  notaxon_late  ... the same behind lines that look like output but are outside a translation
  empty         no byte"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gbk")
SCRIPT = os.path.join(os.environ.get("KAIJU_REFERENCE", "/root/reference"), "util", "kaiju-gbk2faa.pl")

RULES = b"".join([
    b'                     /db_xref="taxon:0010239"\n',               # kind 1; the digits as written
    b'                     /protein_id="P1"\n',                       # kind 2
    b'                     /translation="MKVbzBZxJ*acd"\n',           # kind 3; the filter: MKVDEacd
    b'      /db_xref="taxon:12a" /db_xref="taxon:13"\n',              # the leftmost occurrence that matches: 13
    b'      /protein_id="" /protein_id="P2"\n',                       # ... P2
    b' /translation="Q" /translation="R"\n',                          # ... Q only
    b'/translation="X"\n',                                            # no white space in front: kind 5 (a clear event outside)
    b' x/translation="ACD\n',                                         # kind 5
    b' /translation=""\n',                                            # kind 5
    b' /translation="\n',                                             # kind 5: the last bytes of a line
    b'ACD\n',                                                         # outside: nothing
    b' /translation="" /translation="ACD\n',                          # kind 4 by its second occurrence
    b'EFG\n',                                                         # inside
    b'\n',                                                            # an empty line inside: "\n"
    b'  /db_xref="taxon:77"\n',                                       # kind 1 inside: nothing printed, still inside
    b'  /protein_id="P3"\n',                                          # kind 2 inside
    b'HIK xyz 123\n',
    b' /translation="LMN"\n',                                         # kind 3 inside: a header, and the lines go on
    b'PQR\n',
    b' /translation="STV\n',                                          # kind 4 inside: a second header
    b'WYA" trailing text acd\n',                                      # closes; what follows the `"` is printed too
    b'CCC\n',                                                         # outside again
    b'\x0b/translation="AAV"\n',                                      # which bytes are white space
    b'\x0c/translation="AAF"\n',
    b'\x85/translation="AAG"\n',
    b'\xa0/translation="AAH"\n',
    b'\t/translation="AAT"\n',
    b'\r/translation="AAR"\n',
    b' \t /translation="AAS"\n',
    b' /translation="AC\x00DE"\n',                                    # NUL is a byte of the line
    b' /protein_id="P\x004"\n',
    b' /translation="KK"\n',
    b' /db_xref="taxon:1234567890123456789012345"\n',                 # 25 digits
    b' /translation="GG"\n',
    b' /protein_id="PX" /db_xref="taxon:5"\n',                        # kind 1 in front of kind 2 whatever the order in the line
    b' /translation="HH"\n',
    b' /translation="NO" /protein_id="P5"\n',                         # kind 2 in front of kind 3
    b' /translation="II"\n',
    b' /db_xref="taxon:"\n',                                          # no digit: kind 5
    b' /db_xref="taxon:12\n',                                         # no `"`: kind 5
    b' /db_xref="taxon:9" /translation="NO"\n',                       # kind 1
    b' /protein_id="\n',                                              # kind 5
    b' /translation="LL\n',                                           # kind 4
    b' /translation="MM" x\n',                                        # kind 3 inside
    b' /db_xref="taxon:8"x" /translation="NO\n',                      # kind 1 inside: the state stays
    b'NN\n',
    b'"\n',                                                           # closes with an empty line of letters
    b'PP\n',
    b' /protein_id="P6" /translation="QQ\n',                          # kind 2
    b'RR\n',                                                          # outside
    b' /translation="SS" /translation="TT\n',                         # kind 3 wins over kind 4: the state stays outside
    b'VV\n',
])

RECORD = (b"LOCUS       NC_001422               5386 bp ss-DNA     circular PHG 06-JUL-2018\n"
          b"DEFINITION  Coliphage phi-X174, complete genome.\n"
          b"ACCESSION   NC_001422\n"
          b"FEATURES             Location/Qualifiers\n"
          b"     source          1..5386\n"
          b'                     /organism="Escherichia virus phiX174"\n'
          b'                     /mol_type="genomic DNA"\n'
          b'                     /db_xref="taxon:10847"\n'
          b"     CDS             join(3981..5386,1..136)\n"
          b'                     /gene="phiX174p01"\n'
          b"                     /codon_start=1\n"
          b'                     /product="replication-associated protein"\n'
          b'                     /protein_id="NP_040703.1"\n'
          b'                     /db_xref="GeneID:2546400"\n'
          b'                     /translation="MVRSYYPSECHADYFDFERIEALKPAIEACGISTLSQSPMLGFHKQMDNRI\n'
          b"                     KLLEEILSFRMQGVEFDNGDMYVDGHKAASDVRDEFVSVTEKLMDELAQCYNVLPQLDINN\n"
          b'                     TIDHRPEGDEKWFLENEKTVTQFCRKLAAERPLKDIRDEYNYPKKKGIKDECSRLLEASTMK"\n'
          b"     CDS             51..221\n"
          b'                     /gene="phiX174p03"\n'
          b'                     /product="hypothetical protein"\n'
          b'                     /protein_id="NP_040705.1"\n'
          b'                     /translation="MSRKIILIKQELLLLVYELNRSGLLAENEKIRPILAQLEKLLLCDLSPSTNDSVKN"\n'
          b"ORIGIN\n"
          b"        1 gagttttatc gcttccatga cgcagaagtt aacactttcg gatatttctg atgagtcgaa\n"
          b"       61 aaattatctt gataaagcag gaattactac tgcttgttta cgaattaaat cgaagtggac\n"
          b"      121 tgctggcgga aaatgagaaa attcgaccta tccttgcgca gctcgagaag ctcttacttt\n"
          b"//\n")

CRLF = (b'     /db_xref="taxon:11"\r\n     /protein_id="C1"\r\n     /translation="MKV"\r\n     /translation="ACD\r\n     EFG\r\n     HIK"\r\n     LMN\r\n')
NOPID = b'  /db_xref="taxon:5"\n  /translation="MKV"\n'
TAIL_OPEN = b'  /db_xref="taxon:5"\n  /protein_id="T1"\n  /translation="MKV\n  ACD\n  EFG'
TAIL_CLOSED = b'  /db_xref="taxon:5"\n  /protein_id="T1"\n  /translation="MKV\n  ACD\n  EFG" x'
NOTAXON = b'  /protein_id="N1"\n  /translation="MKV"\n  /db_xref="taxon:5"\n  /translation="ACD"\n'
NOTAXON_LATE = b'ACD\n"\n /translation=""\n\n  /protein_id="N1"\n x /translation="MKV\n  EFG\n  /db_xref="taxon:5"\n  /translation="ACD"\n'

FIXTURES = {"rules": RULES, "record": RECORD, "crlf": CRLF, "nopid": NOPID, "tail_open": TAIL_OPEN, "tail_closed": TAIL_CLOSED, "notaxon": NOTAXON,
            "notaxon_late": NOTAXON_LATE, "empty": b""}


def main():
    if not os.path.exists(SCRIPT):
        sys.exit("the reference's script is not at " + SCRIPT)
    os.makedirs(OUT, exist_ok=True)
    status = []
    for name, text in FIXTURES.items():
        src, dst = os.path.join(OUT, name + ".gbk"), os.path.join(OUT, name + ".faa")
        with open(src, "wb") as f:
            f.write(text)
        r = subprocess.run(["perl", SCRIPT, src, dst], capture_output=True)
        status.append("%s %d\n" % (name, r.returncode))
        print(name, r.returncode, os.path.getsize(dst), r.stderr.decode(errors="replace").strip().splitlines()[-1:] if r.returncode else "")
    with open(os.path.join(OUT, "status.txt"), "w") as f:
        f.write("".join(status))


if __name__ == "__main__":
    main()
