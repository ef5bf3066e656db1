"""The argument checks of the text entry points (kaiju_amd/csrc/capi_text.hip, and the two name tables of capi_index.hip): one
table of calls, each with the status it returns and a piece of kaiju_gpu_last_error().  Every call has at most two records and
a text of a few bytes.  Where two checks could fire the input violates both, and the row says which one answers: that is the
order in which an entry point looks at its arguments, which callers see.  The rows with n = 0 pin what each entry point does
with an empty batch (they differ: some return at once, some run their passes over nothing, one looks at the index first)."""
import ctypes as C

import numpy as np
import pytest

import names_inputs
from test_gpu_parity import Hip

pytestmark = pytest.mark.gpu

OK, ARG, UNSUPPORTED = 0, -1, -7
NULLARG = (ARG, "NULL argument")
BIG = 1 << 32                         # beyond kjf::kMaxBytes = 2^32 - 32: refused before a byte is read
FASTA = b">a\nACGTACGTACGTACGT\n>b\nTTGGCCAATTGGCCAA\n"


class Env:
    """two records of nothing in particular, and contexts on the golden index: t / tp on taxon ids without the accession table
    (nucleotide / protein input), ta with it, s / sp / sa likewise on sequence ids and the sequence-name table"""

    def __init__(self, api, golden):
        self.api, self.L, self.hip = api, api.lib(), Hip()
        self.L.kj_set_last_error.argtypes = [C.c_char_p]
        self.idx = {k: api.Index(golden.fmi, id_mode=m) for k, m in (("t", api.IDS_TAXON), ("ta", api.IDS_TAXON), ("s", api.IDS_SEQUENCE),
                                                                      ("sa", api.IDS_SEQUENCE))}
        self.ctx = {}
        for k, ix, prot in (("t", "t", 0), ("tp", "t", 1), ("ta", "ta", 0), ("s", "s", 0), ("sp", "s", 1), ("sa", "sa", 0)):
            self.ctx[k] = api.Classifier(self.idx[ix], api.default_params("mem", input_is_protein=prot))
        self.tax = api.Taxonomy(golden.nodes)
        self.dtax = api.DeviceTaxonomy(self.tax, 0)
        self.tnames = api.TaxonNames(golden.nodes, names_inputs.GOLDEN_NAMES, "name")
        self.dnames = api.DeviceTaxonNames(self.tnames, 0)
        self.hits = np.zeros(2, dtype=api.HIT_DTYPE)
        self.recs = np.zeros(2, dtype=api.COMPACT_DTYPE)
        self.vout = np.zeros(2, dtype=api.VERBOSE_DTYPE)
        self.off = np.zeros(5, dtype=np.uint64)
        self.off_down = np.array([0, 4, 2, 2, 2], dtype=np.uint64)
        self.seqs = np.frombuffer(b"ACGT", dtype=np.uint8).copy()
        self.text1 = np.frombuffer(b"@a\n@b\n", dtype=np.uint8).copy()
        self.spans = np.array([(1, 1), (4, 1)], dtype=api.NAME_SPAN_DTYPE)
        self.pep = np.frombuffer(b"MK,", dtype=np.uint8).copy()
        self.pos = np.zeros(2, dtype=np.uint64)
        self.pos_out = np.array([0, 9], dtype=np.uint64)            # record 1 starts behind the three bytes of pep
        self.fasta = np.frombuffer(FASTA, dtype=np.uint8).copy()
        self.out = np.zeros(4096, dtype=np.uint8)
        self.d = self.hip.malloc(4096)                              # device scratch: 16-byte aligned, d + 8 is not
        self.hip.memset(self.d, 4096)
        self.text, self.text_bytes = C.c_void_p(0x5a5a), C.c_uint64(77)

    def info(self, dtype):
        a = np.full(1, 0xFF, dtype=np.uint8).repeat(dtype.itemsize).view(dtype)
        self.last_info = a
        return a.ctypes.data

    def h(self, k):
        return self.ctx[k]._h


def p(a):
    return a.ctypes.data


def rows():
    """(id, call(e) -> status, (status, piece of the message), check(e) or None)"""
    R = []

    def row(name, call, want, check=None):
        R.append(pytest.param(call, want, check, id=name))

    def zero_info(e):
        i = e.last_info[0]
        assert int(i["text_bytes"]) == 0 and int(i["n_records"]) == 0 and int(i["overflow"]) == 0

    def zero_text(e):
        zero_info(e)
        assert e.text.value is None and e.text_bytes.value == 0

    # ---- the three-column lines (format.hip): kaiju_gpu_format_compact[_device], kaiju_gpu_classify_text_to_text
    def fc(e, ctx="t", recs=True, off=True, n=2, paired=0, text1=True, bytes1=6, names=True, out=True, out_cap=64, info=True):
        A = e.api
        return e.L.kaiju_gpu_format_compact(e.h(ctx) if ctx else None, p(e.recs) if recs else None, p(e.off) if off else None, n, paired,
                                            p(e.text1) if text1 else None, bytes1, p(e.spans) if names else None, p(e.out) if out else None, out_cap,
                                            e.info(A.FORMAT_INFO_DTYPE) if info else None)
    row("format: ctx NULL", lambda e: fc(e, ctx=None), NULLARG)
    row("format: info NULL", lambda e: fc(e, info=False), NULLARG)
    row("format: records NULL", lambda e: fc(e, recs=False), NULLARG)
    row("format: offsets NULL", lambda e: fc(e, off=False), NULLARG)
    row("format: name spans NULL", lambda e: fc(e, names=False), NULLARG)
    row("format: text NULL", lambda e: fc(e, text1=False), NULLARG)
    row("format: out NULL", lambda e: fc(e, out=False), NULLARG)
    row("format: NULL before the size of the text", lambda e: fc(e, text1=False, bytes1=BIG), NULLARG)
    row("format: text too large", lambda e: fc(e, ctx="s", bytes1=BIG), (ARG, "a block of text must be below 2^32 - 32 bytes, a batch below 2^31 records"))
    row("format: sequence ids", lambda e: fc(e, ctx="s"), (UNSUPPORTED, "the lines of kaijux / kaijup are not made on the device"))
    row("format: sequence ids before mates of proteins", lambda e: fc(e, ctx="sp", paired=1), (UNSUPPORTED, "the lines of kaijux / kaijup are not made on the device"))
    row("format: mates of proteins", lambda e: fc(e, ctx="tp", paired=1), (ARG, "protein reads have no mates"))
    row("format: n = 0", lambda e: fc(e, n=0, recs=False, off=False, names=False, text1=False, bytes1=0), (OK, ""), zero_info)

    def fcd(e, ctx="t", n=2, paired=0, d_out=0, out_cap=64):
        return e.L.kaiju_gpu_format_compact_device(e.h(ctx) if ctx else None, e.d, e.d + 64, n, paired, e.d + 128, 6, e.d + 192, e.d + 1024 + d_out, out_cap,
                                                   e.d + 512, None)
    row("format device: ctx NULL", lambda e: fcd(e, ctx=None), NULLARG)
    row("format device: sequence ids", lambda e: fcd(e, ctx="s"), (UNSUPPORTED, "the lines of kaijux / kaijup are not made on the device"))
    row("format device: mates of proteins", lambda e: fcd(e, ctx="tp", paired=1), (ARG, "protein reads have no mates"))
    row("format device: n = 0", lambda e: fcd(e, n=0), (OK, ""))

    def t2t(e, ctx="t", t=True, text=True, nbytes=None, rec_cap=2, out=True, out_cap=4096, ip=True, fi=True):
        A = e.api
        e.parse_info = np.zeros(1, dtype=A.PARSE_INFO_DTYPE)
        return e.L.kaiju_gpu_classify_text_to_text(e.h(ctx) if ctx else None, e.dtax._h if t else None, p(e.fasta) if text else None,
                                                   len(FASTA) if nbytes is None else nbytes, None, 0, 0, 1, rec_cap, p(e.out) if out else None, out_cap,
                                                   p(e.parse_info) if ip else None, e.info(A.FORMAT_INFO_DTYPE) if fi else None)
    row("text to text: ctx NULL", lambda e: t2t(e, ctx=None), NULLARG)
    row("text to text: taxonomy NULL", lambda e: t2t(e, t=False), NULLARG)
    row("text to text: format info NULL", lambda e: t2t(e, fi=False), NULLARG)
    row("text to text: out NULL", lambda e: t2t(e, out=False), NULLARG)
    row("text to text: parse info NULL", lambda e: t2t(e, ip=False), NULLARG)
    row("text to text: text NULL", lambda e: t2t(e, text=False), NULLARG)
    row("text to text: text too large before sequence ids", lambda e: t2t(e, ctx="s", nbytes=BIG), (ARG, "a block of text must be below 2^32 - 32 bytes"))
    row("text to text: sequence ids", lambda e: t2t(e, ctx="s"), (UNSUPPORTED, "the lines of kaijux / kaijup are not made on the device"))
    row("text to text: out_cap too small", lambda e: t2t(e, out_cap=1), (ARG, "the output text needs more than out_cap bytes"),
        lambda e: int(e.last_info[0]["overflow"]) != 0 or pytest.fail("overflow not reported"))
    row("text to text: rec_cap before out_cap", lambda e: t2t(e, rec_cap=1, out_cap=1), (ARG, "the text holds more records than rec_cap"))
    row("text to text: n = 0", lambda e: t2t(e, text=False, nbytes=0, rec_cap=0, out=False, out_cap=0), (OK, ""), zero_info)

    # ---- the lines with taxon names (format_names.hip)
    def fn(e, ctx="t", recs=True, n=2, paired=0, text1=True, bytes1=6, spans=True, names=True, out=True, out_cap=256, info=True):
        A = e.api
        return e.L.kaiju_gpu_format_names(e.h(ctx) if ctx else None, p(e.recs) if recs else None, p(e.off), n, paired, p(e.text1) if text1 else None, bytes1,
                                          p(e.spans) if spans else None, e.dnames._h if names else None, 0, p(e.out) if out else None, out_cap,
                                          e.info(A.FORMAT_NAMES_INFO_DTYPE) if info else None)
    row("names: ctx NULL", lambda e: fn(e, ctx=None), NULLARG)
    row("names: info NULL", lambda e: fn(e, info=False), NULLARG)
    row("names: names NULL before sequence ids", lambda e: fn(e, ctx="s", names=False), NULLARG)
    row("names: records NULL", lambda e: fn(e, recs=False), NULLARG)
    row("names: name spans NULL", lambda e: fn(e, spans=False), NULLARG)
    row("names: text NULL", lambda e: fn(e, text1=False), NULLARG)
    row("names: out NULL", lambda e: fn(e, out=False), NULLARG)
    row("names: text too large", lambda e: fn(e, ctx="s", bytes1=BIG), (ARG, "a block of text must be below 2^32 - 32 bytes, a batch below 2^31 records"))
    row("names: sequence ids", lambda e: fn(e, ctx="s"), (UNSUPPORTED, "the lines of kaijux / kaijup carry no taxon"))
    row("names: sequence ids before mates of proteins", lambda e: fn(e, ctx="sp", paired=1), (UNSUPPORTED, "the lines of kaijux / kaijup carry no taxon"))
    row("names: mates of proteins", lambda e: fn(e, ctx="tp", paired=1), (ARG, "protein reads have no mates"))
    row("names: n = 0", lambda e: fn(e, n=0, recs=False, spans=False, text1=False, bytes1=0), (OK, ""), zero_info)

    def fnd(e, ctx="t", names=True, n=2, paired=0):
        return e.L.kaiju_gpu_format_names_device(e.h(ctx) if ctx else None, e.d, e.d + 64, n, paired, e.d + 128, 6, e.d + 192, e.dnames._h if names else None, 0,
                                                 e.d + 1024, 256, e.d + 512, None)
    row("names device: ctx NULL", lambda e: fnd(e, ctx=None), NULLARG)
    row("names device: names NULL before sequence ids", lambda e: fnd(e, ctx="s", names=False), NULLARG)
    row("names device: sequence ids", lambda e: fnd(e, ctx="s"), (UNSUPPORTED, "the lines of kaijux / kaijup carry no taxon"))
    row("names device: n = 0", lambda e: fnd(e, n=0), (OK, ""))

    def t2tn(e, ctx="t", t=True, names=True, nbytes=None, rec_cap=2, out=True, out_cap=4096, fi=True):
        A = e.api
        e.parse_info = np.zeros(1, dtype=A.PARSE_INFO_DTYPE)
        return e.L.kaiju_gpu_classify_text_to_text_names(e.h(ctx) if ctx else None, e.dtax._h if t else None, p(e.fasta) if nbytes != 0 else None,
                                                         len(FASTA) if nbytes is None else nbytes, None, 0, 0, 1, rec_cap, e.dnames._h if names else None, 0,
                                                         p(e.out) if out else None, out_cap, p(e.parse_info), e.info(A.FORMAT_NAMES_INFO_DTYPE) if fi else None)
    row("text to text names: ctx NULL", lambda e: t2tn(e, ctx=None), NULLARG)
    row("text to text names: taxonomy NULL", lambda e: t2tn(e, t=False), NULLARG)
    row("text to text names: names NULL before the size of the text", lambda e: t2tn(e, names=False, nbytes=BIG), NULLARG)
    row("text to text names: format info NULL", lambda e: t2tn(e, fi=False), NULLARG)
    row("text to text names: out NULL", lambda e: t2tn(e, out=False), NULLARG)
    row("text to text names: text too large before sequence ids", lambda e: t2tn(e, ctx="s", nbytes=BIG), (ARG, "a block of text must be below 2^32 - 32 bytes"))
    row("text to text names: sequence ids", lambda e: t2tn(e, ctx="s"), (UNSUPPORTED, "the lines of kaijux / kaijup carry no taxon"))
    row("text to text names: out_cap too small", lambda e: t2tn(e, out_cap=1), (ARG, "the output text needs more than out_cap bytes"),
        lambda e: int(e.last_info[0]["overflow"]) != 0 or pytest.fail("overflow not reported"))
    row("text to text names: rec_cap before out_cap", lambda e: t2tn(e, rec_cap=1, out_cap=1), (ARG, "the text holds more records than rec_cap"))
    row("text to text names: n = 0", lambda e: t2tn(e, nbytes=0, rec_cap=0, out=False, out_cap=0), (OK, ""), zero_info)

    # ---- the lines of kaiju -v (format_verbose.hip) and the accession table
    row("accessions: index NULL", lambda e: e.L.kaiju_gpu_index_upload_accessions(None), NULLARG)
    row("accessions: sequence ids", lambda e: e.L.kaiju_gpu_index_upload_accessions(e.idx["s"]._h), (UNSUPPORTED, "an index of sequence ids (kaijux / kaijup) has no accession column"))
    row("accessions: not uploaded", lambda e: int(e.L.kaiju_gpu_index_accession_bytes(e.idx["t"]._h)), (OK, ""))
    row("sequence names: index NULL", lambda e: e.L.kaiju_gpu_index_upload_seq_names(None), NULLARG)
    row("sequence names: not uploaded", lambda e: int(e.L.kaiju_gpu_index_seq_name_bytes(e.idx["s"]._h)), (OK, ""))

    def fv(e, ctx="ta", hits=True, vout=True, pos="pos", text=True, text_bytes=3, recs=True, off=True, n=2, paired=0, names_text=True, names_bytes=6, names=True,
           out=True, out_cap=256, info=True):
        A = e.api
        return e.L.kaiju_gpu_format_verbose(e.h(ctx) if ctx else None, p(e.hits) if hits else None, p(e.vout) if vout else None, p(getattr(e, pos)) if pos else None,
                                            p(e.pep) if text else None, text_bytes, 16, p(e.recs) if recs else None, p(e.off) if off else None, n, paired,
                                            p(e.text1) if names_text else None, names_bytes, p(e.spans) if names else None, p(e.out) if out else None, out_cap,
                                            e.info(A.FORMAT_VERBOSE_INFO_DTYPE) if info else None)
    row("verbose: ctx NULL", lambda e: fv(e, ctx=None), NULLARG)
    row("verbose: info NULL", lambda e: fv(e, info=False), NULLARG)
    row("verbose: hits NULL", lambda e: fv(e, hits=False), NULLARG)
    row("verbose: verbose records NULL", lambda e: fv(e, vout=False), NULLARG)
    row("verbose: positions NULL", lambda e: fv(e, pos=None), NULLARG)
    row("verbose: records NULL", lambda e: fv(e, recs=False), NULLARG)
    row("verbose: offsets NULL", lambda e: fv(e, off=False), NULLARG)
    row("verbose: name spans NULL", lambda e: fv(e, names=False), NULLARG)
    row("verbose: peptides NULL", lambda e: fv(e, text=False), NULLARG)
    row("verbose: names NULL before their size", lambda e: fv(e, names_text=False, names_bytes=BIG), NULLARG)
    row("verbose: out NULL", lambda e: fv(e, out=False), NULLARG)
    row("verbose: names too large before sequence ids", lambda e: fv(e, ctx="s", names_bytes=BIG), (ARG, "the names must be below 2^32 - 32 bytes, a batch below 2^31 records"))
    row("verbose: sequence ids before mates of proteins", lambda e: fv(e, ctx="sp", paired=1), (UNSUPPORTED, "the lines of kaijux / kaijup are not made on the device"))
    row("verbose: mates of proteins before the missing table", lambda e: fv(e, ctx="tp", paired=1), (ARG, "protein reads have no mates"))
    row("verbose: no accession table before the positions", lambda e: fv(e, ctx="t", pos="pos_out"), (ARG, "the index has no accession table on the device: call kaiju_gpu_index_upload_accessions() first"))
    row("verbose: text_pos outside the text", lambda e: fv(e, pos="pos_out"), (ARG, "the peptides of a record lie outside the text"))
    row("verbose: n = 0", lambda e: fv(e, n=0, hits=False, vout=False, pos=None, recs=False, off=False, names=False, text=False, text_bytes=0, names_text=False,
                                       names_bytes=0), (OK, ""), zero_info)

    def fvd(e, ctx="ta", d_out=0, out_cap=256, info=True, n=2):
        return e.L.kaiju_gpu_format_verbose_device(e.h(ctx) if ctx else None, e.d + 2048, e.d, e.d + 64, n, 0, e.d + 128, e.d + 256, e.d + 448, e.d + 480, e.d + 496, 16,
                                                   e.d + 512, 6, e.d + 192, (e.d + 1024 + d_out) if d_out is not None else None, out_cap, (e.d + 576) if info else None, None)
    row("verbose device: ctx NULL", lambda e: fvd(e, ctx=None), NULLARG)
    row("verbose device: info NULL", lambda e: fvd(e, info=False), NULLARG)
    row("verbose device: out NULL", lambda e: fvd(e, d_out=None), NULLARG)
    row("verbose device: unaligned out before sequence ids", lambda e: fvd(e, ctx="s", d_out=8), (ARG, "the output pointer must be 16-byte aligned"))
    row("verbose device: sequence ids", lambda e: fvd(e, ctx="s"), (UNSUPPORTED, "the lines of kaijux / kaijup are not made on the device"))
    row("verbose device: no accession table", lambda e: fvd(e, ctx="t"), (ARG, "the index has no accession table on the device"))
    row("verbose device: n = 0", lambda e: fvd(e, n=0), (OK, ""))

    def cvt(e, ctx="ta", t=True, off=True, n=1, paired=0, names_text=True, names_bytes=6, names=True, text=True, tb=True, info=True):
        A = e.api
        e.text, e.text_bytes = C.c_void_p(0x5a5a), C.c_uint64(77)
        return e.L.kaiju_gpu_classify_batch_verbose_text(e.h(ctx) if ctx else None, e.dtax._h if t else None, p(e.seqs), p(e.off) if off else None, n, paired,
                                                         p(e.text1) if names_text else None, names_bytes, p(e.spans) if names else None,
                                                         C.byref(e.text) if text else None, C.byref(e.text_bytes) if tb else None,
                                                         e.info(A.FORMAT_VERBOSE_INFO_DTYPE) if info else None)
    row("verbose text: ctx NULL", lambda e: cvt(e, ctx=None), NULLARG)
    row("verbose text: taxonomy NULL", lambda e: cvt(e, t=False), NULLARG)
    row("verbose text: offsets NULL", lambda e: cvt(e, off=False), NULLARG)
    row("verbose text: text NULL", lambda e: cvt(e, text=False), NULLARG)
    row("verbose text: text_bytes NULL", lambda e: cvt(e, tb=False), NULLARG)
    row("verbose text: info NULL", lambda e: cvt(e, info=False), NULLARG)
    row("verbose text: name spans NULL", lambda e: cvt(e, names=False), NULLARG)
    row("verbose text: names NULL before their size", lambda e: cvt(e, names_text=False, names_bytes=BIG), NULLARG)
    row("verbose text: names too large before sequence ids", lambda e: cvt(e, ctx="s", names_bytes=BIG), (ARG, "the names must be below 2^32 - 32 bytes, a batch below 2^31 records"))
    row("verbose text: sequence ids before mates of proteins", lambda e: cvt(e, ctx="sp", paired=1), (UNSUPPORTED, "the lines of kaijux / kaijup are not made on the device"))
    row("verbose text: mates of proteins before the missing table", lambda e: cvt(e, ctx="tp", paired=1), (ARG, "protein reads have no mates"))
    row("verbose text: no accession table", lambda e: cvt(e, ctx="t"), (ARG, "the index has no accession table on the device"))
    row("verbose text: n = 0 returns before the index is looked at", lambda e: cvt(e, ctx="sp", n=0, paired=1, names=False), (OK, ""), zero_text)

    # ---- the lines of kaijux / kaijup (format_seq.hip) and the sequence-name table
    def fs(e, ctx="sa", hits=True, off="off", n=2, paired=0, u_rule=0, seqs=True, vout=True, pos="pos", text=True, text_bytes=3, names_text=True, names_bytes=6,
           names=True, out=True, out_cap=256, info=True):
        A = e.api
        return e.L.kaiju_gpu_format_seq(e.h(ctx) if ctx else None, p(e.hits) if hits else None, p(getattr(e, off)) if off else None, n, paired, u_rule,
                                        p(e.seqs) if seqs else None, p(e.vout) if vout else None, p(getattr(e, pos)) if pos else None, p(e.pep) if text else None,
                                        text_bytes, 16, p(e.text1) if names_text else None, names_bytes, p(e.spans) if names else None, p(e.out) if out else None,
                                        out_cap, e.info(A.FORMAT_VERBOSE_INFO_DTYPE) if info else None)
    row("seq: ctx NULL", lambda e: fs(e, ctx=None), NULLARG)
    row("seq: info NULL", lambda e: fs(e, info=False), NULLARG)
    row("seq: hits NULL", lambda e: fs(e, hits=False), NULLARG)
    row("seq: offsets NULL", lambda e: fs(e, off=None), NULLARG)
    row("seq: name spans NULL", lambda e: fs(e, names=False), NULLARG)
    row("seq: verbose records NULL with peptides", lambda e: fs(e, vout=False), NULLARG)
    row("seq: positions NULL with peptides", lambda e: fs(e, pos=None), NULLARG)
    row("seq: names NULL before their size", lambda e: fs(e, names_text=False, names_bytes=BIG), NULLARG)
    row("seq: out NULL", lambda e: fs(e, out=False), NULLARG)
    row("seq: names too large before taxon ids", lambda e: fs(e, ctx="t", names_bytes=BIG), (ARG, "the names must be below 2^32 - 32 bytes, a batch below 2^31 records"))
    row("seq: taxon ids before u_rule", lambda e: fs(e, ctx="t", u_rule=7), (ARG, "the lines of kaijux / kaijup need an index loaded with KAIJU_GPU_IDS_SEQUENCE"))
    row("seq: u_rule before mates of proteins", lambda e: fs(e, ctx="sp", u_rule=7, paired=1), (ARG, "u_rule must be KAIJU_GPU_U_RULE_NUCLEOTIDE or KAIJU_GPU_U_RULE_PROTEIN"))
    row("seq: mates of proteins before the missing table", lambda e: fs(e, ctx="sp", paired=1), (ARG, "protein reads have no mates"))
    row("seq: no name table before the offsets", lambda e: fs(e, ctx="s", off="off_down"), (ARG, "the index has no sequence-name table on the device: call kaiju_gpu_index_upload_seq_names() first"))
    row("seq: decreasing offsets before the positions", lambda e: fs(e, off="off_down", pos="pos_out"), (ARG, "offsets must be non-decreasing"))
    row("seq: seqs NULL before the positions", lambda e: fs(e, off="off_seqs", u_rule=1, seqs=False, pos="pos_out"), (ARG, "seqs is NULL"))
    row("seq: text_pos outside the text", lambda e: fs(e, pos="pos_out"), (ARG, "the peptides of a record lie outside the text"))
    row("seq: n = 0", lambda e: fs(e, n=0, hits=False, off=None, names=False, vout=False, pos=None, text=False, text_bytes=0, names_text=False, names_bytes=0,
                                   seqs=False), (OK, ""), zero_info)

    def fsd(e, ctx="sa", d_out=0, info=True, n=2, u_rule=0):
        return e.L.kaiju_gpu_format_seq_device(e.h(ctx) if ctx else None, e.d + 2048, e.d + 64, n, 0, u_rule, e.d + 128, e.d + 448, e.d + 480, e.d + 496, 16, e.d + 512, 6,
                                               e.d + 192, (e.d + 1024 + d_out) if d_out is not None else None, 256, (e.d + 576) if info else None, None)
    row("seq device: ctx NULL", lambda e: fsd(e, ctx=None), NULLARG)
    row("seq device: info NULL", lambda e: fsd(e, info=False), NULLARG)
    row("seq device: out NULL", lambda e: fsd(e, d_out=None), NULLARG)
    row("seq device: unaligned out before taxon ids", lambda e: fsd(e, ctx="t", d_out=8), (ARG, "the output pointer must be 16-byte aligned"))
    row("seq device: taxon ids", lambda e: fsd(e, ctx="t"), (ARG, "the lines of kaijux / kaijup need an index loaded with KAIJU_GPU_IDS_SEQUENCE"))
    row("seq device: u_rule", lambda e: fsd(e, u_rule=-1), (ARG, "u_rule must be"))
    row("seq device: no name table", lambda e: fsd(e, ctx="s"), (ARG, "the index has no sequence-name table on the device"))
    row("seq device: n = 0", lambda e: fsd(e, n=0), (OK, ""))

    def cst(e, ctx="sa", off=True, n=1, paired=0, verbose=0, u_rule=0, names_text=True, names_bytes=6, names=True, text=True, tb=True, info=True):
        A = e.api
        e.text, e.text_bytes = C.c_void_p(0x5a5a), C.c_uint64(77)
        return e.L.kaiju_gpu_classify_batch_seq_text(e.h(ctx) if ctx else None, p(e.seqs), p(e.off) if off else None, n, paired, verbose, u_rule,
                                                     p(e.text1) if names_text else None, names_bytes, p(e.spans) if names else None,
                                                     C.byref(e.text) if text else None, C.byref(e.text_bytes) if tb else None,
                                                     e.info(A.FORMAT_VERBOSE_INFO_DTYPE) if info else None)
    row("seq text: ctx NULL", lambda e: cst(e, ctx=None), NULLARG)
    row("seq text: offsets NULL", lambda e: cst(e, off=False), NULLARG)
    row("seq text: text NULL", lambda e: cst(e, text=False), NULLARG)
    row("seq text: text_bytes NULL", lambda e: cst(e, tb=False), NULLARG)
    row("seq text: info NULL", lambda e: cst(e, info=False), NULLARG)
    row("seq text: name spans NULL", lambda e: cst(e, names=False), NULLARG)
    row("seq text: names NULL before their size", lambda e: cst(e, names_text=False, names_bytes=BIG), NULLARG)
    row("seq text: names too large before taxon ids", lambda e: cst(e, ctx="t", names_bytes=BIG), (ARG, "the names must be below 2^32 - 32 bytes, a batch below 2^31 records"))
    row("seq text: taxon ids before u_rule", lambda e: cst(e, ctx="t", u_rule=7), (ARG, "the lines of kaijux / kaijup need an index loaded with KAIJU_GPU_IDS_SEQUENCE"))
    row("seq text: n = 0 still looks at the index", lambda e: cst(e, ctx="t", n=0, names=False), (ARG, "the lines of kaijux / kaijup need an index loaded with KAIJU_GPU_IDS_SEQUENCE"), zero_text)
    row("seq text: n = 0 still looks at u_rule", lambda e: cst(e, n=0, u_rule=7, names=False), (ARG, "u_rule must be"), zero_text)
    row("seq text: n = 0 still looks for the name table", lambda e: cst(e, ctx="s", n=0, names=False), (ARG, "the index has no sequence-name table on the device"), zero_text)
    row("seq text: mates of proteins before the missing table", lambda e: cst(e, ctx="sp", paired=1), (ARG, "protein reads have no mates"))
    row("seq text: n = 0", lambda e: cst(e, n=0, names=False), (OK, ""), zero_text)
    return R


@pytest.fixture(scope="module")
def env(gpu_lib, golden):
    e = Env(gpu_lib, golden)
    e.off_seqs = np.array([0, 2, 2, 4, 4], dtype=np.uint64)
    assert e.idx["ta"].upload_accessions() > 0 and e.idx["sa"].upload_seq_names() > 0
    yield e
    e.hip.free(e.d)
    for c in e.ctx.values():
        c.close()


@pytest.mark.parametrize("call,want,check", rows())
def test_text_entry_point_refusals(env, call, want, check):
    status, piece = want
    env.L.kj_set_last_error(b"(no call has failed)")
    rc = call(env)
    message = env.L.kaiju_gpu_last_error().decode()
    print(rc, message)
    assert rc == status, (rc, message)
    if status != OK:
        assert piece in message, message
    else:
        assert message == "(no call has failed)"
    if check:
        check(env)
