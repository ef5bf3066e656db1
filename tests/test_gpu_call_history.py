"""Records do not depend on what a context, its buffers or the caller's buffers held before a call - the device's half (the
host's: test_call_history_emu.py; the cases: history_cases.py).

Caller buffers: kaiju_gpu_classify_batch_device_compact does not clear d_hits on the fused MEM path (kj_flow.h: clear_out;
include/kaiju_gpu.h: "the lanes write the header of every record and the entries they announce in it"), so d_hits and d_out
start as records of OTHER calls - only ever records the library wrote itself: a stale read of one is a wrong result here, never
a wild address.  Context history: one context runs A, then B; B's records must be those of a fresh context and the oracle's.
Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import history_cases as H
import postsearch_inputs as P
import util

pytestmark = pytest.mark.gpu

INTERNAL = 0xE0000000            # KAIJU_HIT_INEXACT, kHitRetry, kHitLocPending: none of them leaves the library
ERR_READ_TOO_LONG = 16           # kj_core.h: kErrReadTooLong


class Hip:
    """the few HIP runtime calls the device-buffer tests need, through ctypes on the runtime libkaiju_gpu.so is linked against"""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so.7")
        self.owned = []

    def ck(self, rc):
        assert rc == 0, f"HIP error {rc}"

    def malloc(self, n):
        p = C.c_void_p()
        self.ck(self.L.hipMalloc(C.byref(p), C.c_size_t(max(int(n), 16))))
        self.owned.append(p.value)
        return p.value

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes:
            self.ck(self.L.hipMemcpy(C.c_void_p(dptr), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), 1))

    def d2h(self, dptr, nbytes, dtype):
        out = np.zeros(nbytes, dtype=np.uint8)
        if nbytes:
            self.ck(self.L.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(dptr), C.c_size_t(nbytes), 2))
        return np.frombuffer(out.tobytes(), dtype=dtype)

    def memset(self, dptr, nbytes):
        if nbytes:
            self.ck(self.L.hipMemset(C.c_void_p(dptr), 0, C.c_size_t(nbytes)))

    def stream(self):
        s = C.c_void_p()
        self.ck(self.L.hipStreamCreateWithFlags(C.byref(s), 1))       # hipStreamNonBlocking
        return s.value

    def free_all(self):
        for p in self.owned:
            self.L.hipFree(C.c_void_p(p))
        self.owned = []


@pytest.fixture(scope="module")
def hip(gpu_lib):
    h = Hip()
    yield h
    h.free_all()


class World:
    """a database: the oracle's handles, the device taxonomy, the indexes (each layout loaded once), the oracle's records"""

    def __init__(self, api, oracle, fmi, nodes):
        self.api, self.oracle, self.fmi = api, oracle, fmi
        self.ix, self.otax = oracle.load_fmi(fmi), oracle.load_nodes(nodes)
        self.tax = api.Taxonomy(nodes)
        self.dtax = api.DeviceTaxonomy(self.tax, 0)
        self._idx, self._want = {}, {}

    def index(self, wide=""):
        if wide not in self._idx:
            with H.Env({"KAIJU_GPU_FORCE_WIDE": wide} if wide else {}):
                self._idx[wide] = self.api.Index(self.fmi)
            assert bool(self._idx[wide].layout().wide) == bool(wide)
        return self._idx[wide]

    def classifier(self, mode, seg, m=11, protein=False, wide="", env=None):
        with H.Env(env or {}):
            return self.api.Classifier(self.index(wide), self.api.default_params(mode, seg=seg, min_fragment_length=m, input_is_protein=int(protein)))

    def want(self, call, mode, seg, m=11, protein=False):
        key = (id(call), mode, seg, m, protein)
        if key not in self._want:
            s, o = call.oracle_batch()
            p = self.oracle.params(mode, seg=seg, use_evalue=0, min_fragment_length=m, protein=int(protein))
            self._want[key] = self.oracle.classify(self.ix, self.otax, p, s, o, paired=call.paired)
        return self._want[key]

    def compact(self, want):
        """the 16-byte records the oracle's records give: the LCA of the ids, best, flags << 8 | n_ids"""
        out = np.zeros(len(want), dtype=self.api.COMPACT_DTYPE)
        for i, w in enumerate(want):
            n = int(w["n_ids"])
            out[i] = (self.tax.lca([int(x) for x in w["taxid"][:n]]) if n else 0, int(w["best"]), (int(w["flags"]) & 3) << 8 | n)
        return out

    def close(self):
        for ix in self._idx.values():
            ix.close()


@pytest.fixture(scope="module")
def worlds(gpu_lib, oracle, golden, tmp_path_factory):
    _, fmi, nodes = P.write_db(P.inputs(), str(tmp_path_factory.mktemp("history")))
    w = {"golden": World(gpu_lib, oracle, golden.fmi, golden.nodes), "motif": World(gpu_lib, oracle, fmi, nodes)}
    yield w
    for x in w.values():
        x.close()


class DevCall:
    """a call's batch in device memory and output buffers of its own"""

    def __init__(self, hip, api, call):
        self.hip, self.api, self.call, self.n = hip, api, call, call.n
        seqs = np.ascontiguousarray(call.seqs, dtype=np.uint8)
        off = np.ascontiguousarray(call.off, dtype=np.uint64)
        self.seq_bytes = seqs.nbytes
        self.d_seqs, self.d_off = hip.malloc(seqs.nbytes + 64), hip.malloc(off.nbytes)
        self.d_hits, self.d_rec = hip.malloc(self.n * 184), hip.malloc(self.n * 16)
        hip.h2d(self.d_seqs, seqs)
        hip.h2d(self.d_off, off)

    def prefill(self, hits=None, recs=None):
        """the output buffers as an earlier call left them: records repeated or cut to this call's n; None: zeros"""
        for d, res, size, dt in ((self.d_hits, hits, 184, self.api.HIT_DTYPE), (self.d_rec, recs, 16, self.api.COMPACT_DTYPE)):
            if res is None or not len(res) or not self.n:
                self.hip.memset(d, self.n * size)
            else:
                self.hip.h2d(d, np.resize(np.ascontiguousarray(res, dtype=dt), self.n))

    def enqueue(self, clf, dtax=None, stream=0):
        if dtax is None:
            clf.classify_device(self.d_seqs, self.seq_bytes, self.d_off, self.n, self.d_hits, paired=self.call.paired, stream=stream)
        else:
            clf.classify_device_compact(dtax, self.d_seqs, self.seq_bytes, self.d_off, self.n, self.d_hits, self.d_rec, paired=self.call.paired, stream=stream)

    def results(self):
        return self.hip.d2h(self.d_hits, self.n * 184, self.api.HIT_DTYPE), self.hip.d2h(self.d_rec, self.n * 16, self.api.COMPACT_DTYPE)


def vs_oracle(want, hits):
    return [i for i in range(len(want)) if not util.same_hit(want[i], hits[i])]


# ---- caller buffers ----------------------------------------------------------------------------------------------------------
# (world, case, m): the victim runs over the records of the case's first call - and, for the routes, the other way round
CALLER_CASES = [("golden", "records_rotated", 11, False), ("golden", "records_rotated_pairs", 11, False), ("golden", "records_on_nothing", 11, False),
                ("golden", "routes_exact", 11, True), ("motif", "routes_pairs", 8, True), ("motif", "routes_single", 8, True),
                ("motif", "routes_rows", 11, True)]


@pytest.mark.parametrize("wide", ["", "16"])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_caller_buffers_hold_other_records(gpu_lib, hip, worlds, fused, wide):
    """kaiju_gpu_classify_batch_device_compact with d_hits and d_out full of the records of other calls: the same call's rotated
    by one read, a batch whose every read has a record under reads that can have none, and the routes in both directions -
    the records of plain reads under reads that take the lazy-SEG listing, the second search, the retry pass, the many-rows
    locate (the motif world, m = 8 and 11) or the exact pass, and those reads' records under plain reads.  MEM with the fused
    post-search pass and without, narrow and forced wide, single and paired, the NULL stream and an explicit one, SEG on and off.
    Where the plan does not clear d_hits (fused, narrow, the row -> taxon table; SEG lazily or off) that is asserted: id slots
    behind n_ids still hold the residue"""
    api = gpu_lib
    stream = hip.stream()
    uncleared = {}
    try:
        for seg in (1, 0):
            clfs = {}
            for world, name, m, both in CALLER_CASES:
                w = worlds[world]
                if not wide:          # the narrow index has what the fused pass needs: k-mer lines and the row -> taxon table
                    lay = w.index(wide).layout()
                    assert lay.bytes[api.INDEX_ARRAYS.index("row_tax")] > 0 and lay.bytes[api.INDEX_ARRAYS.index("kmer_lines")] > 0
                if (world, m) not in clfs:
                    clfs[(world, m)] = w.classifier("mem", seg, m, wide=wide, env={"KAIJU_GPU_FUSED_POST": fused})
                clf = clfs[(world, m)]
                case = H.by_name(H.golden_cases() if world == "golden" else H.motif_cases())[name]
                for A, B in [(case.calls[0], case.victim)] + ([(case.victim, case.calls[0])] if both else []):
                    dev = DevCall(hip, api, B)
                    bound = max(A.max_len, B.max_len)
                    clf.set_max_read_length(bound)
                    res_hits = clf.classify(A.seqs, A.off, paired=A.paired).copy()        # what another call left: written by the library
                    res_recs = clf.lca(w.dtax, res_hits).copy()
                    dev.prefill()
                    dev.enqueue(clf, w.dtax)
                    clf.synchronize()
                    hits0, recs0 = dev.results()
                    want = w.want(B, "mem", seg, m)
                    assert not vs_oracle(want, hits0), (name, B.name, seg, "zeroed buffers")
                    if world == "golden":      # (the motif world has ids that nodes.dmp lacks: its 16-byte records are test_gpu_postsearch.py's)
                        assert (recs0 == w.compact(want)).all(), (name, B.name, seg, "zeroed buffers", np.nonzero(recs0 != w.compact(want))[0][:5])
                    for s in (0, stream):
                        dev.prefill(res_hits, res_recs)
                        dev.enqueue(clf, w.dtax, stream=s)
                        clf.synchronize()
                        hits, recs = dev.results()
                        assert (recs == recs0).all(), (name, B.name, seg, s != 0, np.nonzero(recs != recs0)[0][:5])
                        assert H.specified_equal(hits, hits0) and not (hits["flags"] & INTERNAL).any(), (name, B.name, seg, s != 0)
                        assert clf.stats().error_flags == 0
                        behind = np.arange(21)[None, :] >= hits["n_ids"][:, None]
                        key = (seg == 0 or bound <= 287)                                # the fast stage 1 (lazy SEG) or no SEG at all
                        uncleared[key] = uncleared.get(key, False) or bool((hits["taxid"][behind] != 0).any())
            for c in clfs.values():
                c.close()
        # d_hits was the caller's memory as it stood exactly where kj_flow.h says so - and cleared everywhere else
        assert uncleared[True] == (fused == "1" and not wide) and not uncleared[False], (fused, wide, uncleared)
    finally:
        hip.free_all()


# ---- context history ---------------------------------------------------------------------------------------------------------
def run_call(clf, hip, api, call):
    """host buffers (the entry point measures the read lengths itself) unless the case is about the bound the caller gives -
    or about an empty batch, which only the device-resident entry point hands on to the launch"""
    if call.n and call.max_len == max([1] + [len(x) for x in call.reads1] + [len(x) for x in (call.reads2 or [])]) and not call.too_long:
        return clf.classify(call.seqs, call.off, paired=call.paired).copy()
    dev = DevCall(hip, api, call)
    clf.set_max_read_length(call.max_len)
    dev.prefill()
    dev.enqueue(clf)
    clf.synchronize()
    return dev.results()[0]


ALL_CASES = [(w, c.name, mode) for w, cases in (("golden", H.golden_cases()), ("motif", H.motif_cases())) for c in cases if c.device for mode in c.modes]


@pytest.mark.parametrize("world,name,mode", ALL_CASES, ids=[f"{n}-{m}" for _, n, m in ALL_CASES])
def test_context_history(gpu_lib, hip, worlds, world, name, mode):
    """one context runs the calls of a case in order; the last call's records == a fresh context's == the oracle's.  Chain cases:
    the calls back and forth on ONE context, the first again at the end - every result equals that call's first"""
    api, w = gpu_lib, worlds[world]
    case = H.by_name(H.golden_cases() if world == "golden" else H.motif_cases())[name]
    env = {"KAIJU_GPU_STAGE1": "old"} if name == "continuation_old_short" else {}
    try:
        for seg in case.segs:
            B = case.victim
            fresh = w.classifier(mode, seg, case.m, case.protein, env=env)
            solo = run_call(fresh, hip, api, B)
            assert fresh.stats().error_flags == (ERR_READ_TOO_LONG if B.too_long else 0), (name, mode, seg)
            fresh.close()
            assert not vs_oracle(w.want(B, mode, seg, case.m, case.protein), solo), (name, mode, seg, "fresh context vs the oracle")
            clf = w.classifier(mode, seg, case.m, case.protein, env=env)
            first = {}
            order = case.calls + (case.calls[-2::-1] + case.calls[1:] + case.calls[:1] if case.chain else [])
            for call in order:
                got = run_call(clf, hip, api, call)
                assert not (got["flags"] & INTERNAL).any(), (name, mode, seg, call.name)
                if call.name not in first:
                    first[call.name] = got
                    assert not vs_oracle(w.want(call, mode, seg, case.m, case.protein), got), (name, mode, seg, call.name, "vs the oracle")
                assert (got == first[call.name]).all(), (name, mode, seg, call.name, np.nonzero(got != first[call.name])[0][:5])
            assert (first[B.name] == solo).all(), (name, mode, seg, np.nonzero(first[B.name] != solo)[0][:5])
            clf.close()
    finally:
        hip.free_all()


# ---- no synchronisation between the calls --------------------------------------------------------------------------------------
BACK_TO_BACK = [("golden", "layout_paired_single", "mem"), ("golden", "shrink", "mem"), ("golden", "routes_exact", "greedy"),
                ("motif", "routes_pairs", "mem"), ("motif", "routes_rows", "greedy")]


@pytest.mark.parametrize("world,name,mode", BACK_TO_BACK, ids=[f"{n}-{m}" for _, n, m in BACK_TO_BACK])
def test_calls_enqueued_back_to_back(gpu_lib, hip, worlds, world, name, mode):
    """A and B on the context's stream into different caller buffers, one synchronize() at the end: both == their solo results
    (the 16-byte records too)"""
    api, w = gpu_lib, worlds[world]
    case = H.by_name(H.golden_cases() if world == "golden" else H.motif_cases())[name]
    A, B = case.calls[0], case.victim
    bound = max(A.max_len, B.max_len)
    try:
        solo = {}
        for call in (A, B):
            c = w.classifier(mode, 1, case.m)
            c.set_max_read_length(bound)
            d = DevCall(hip, api, call)
            d.prefill()
            d.enqueue(c, w.dtax)
            c.synchronize()
            solo[call.name] = d.results()
            assert not vs_oracle(w.want(call, mode, 1, case.m), solo[call.name][0]), (name, call.name)
            c.close()
        clf = w.classifier(mode, 1, case.m)
        clf.set_max_read_length(bound)
        devs = [DevCall(hip, api, call) for call in (A, B, A)]
        for d in devs:
            d.prefill()
        for d in devs:
            d.enqueue(clf, w.dtax)
        clf.synchronize()
        assert clf.stats().error_flags == 0
        for d in devs:
            hits, recs = d.results()
            assert H.specified_equal(hits, solo[d.call.name][0]) and (recs == solo[d.call.name][1]).all(), (name, d.call.name)
        clf.close()
    finally:
        hip.free_all()


@pytest.mark.parametrize("mode", ["mem", "greedy"])
def test_two_contexts_on_one_index(gpu_lib, hip, worlds, mode):
    """the shape of a benchmark step: context 0 runs A, B, A while context 1 runs B, A, B, enqueued alternately on their own
    streams without synchronising in between; every result == its solo result"""
    api, w = gpu_lib, worlds["golden"]
    case = H.by_name(H.golden_cases())["layout_paired_single"]
    A, B = case.calls
    bound = max(A.max_len, B.max_len)
    try:
        solo = {}
        for call in (A, B):
            c = w.classifier(mode, 1)
            c.set_max_read_length(bound)
            d = DevCall(hip, api, call)
            d.prefill()
            d.enqueue(c, w.dtax)
            c.synchronize()
            solo[call.name] = d.results()
            assert not vs_oracle(w.want(call, mode, 1), solo[call.name][0]), call.name
            c.close()
        ctx = [w.classifier(mode, 1), w.classifier(mode, 1)]
        for c in ctx:
            c.set_max_read_length(bound)
        devs = [[DevCall(hip, api, call) for call in calls] for calls in ((A, B, A), (B, A, B))]
        for row in devs:
            for d in row:
                d.prefill(solo[B.name if d.call is A else A.name][0], solo[B.name if d.call is A else A.name][1])   # the other call's records
        for step in range(3):
            for k in (0, 1):
                devs[k][step].enqueue(ctx[k], w.dtax)
        for c in ctx:
            c.synchronize()
            assert c.stats().error_flags == 0
        for k in (0, 1):
            for step, d in enumerate(devs[k]):
                hits, recs = d.results()
                assert H.specified_equal(hits, solo[d.call.name][0]) and (recs == solo[d.call.name][1]).all(), (mode, k, step)
        for c in ctx:
            c.close()
    finally:
        hip.free_all()


# ---- kaiju -v -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mem", "greedy"])
def test_verbose_buffers_after_many_accessions(gpu_lib, golden, oracle, mode):
    """a -v context: A's reads have 20 accessions and a matched peptide each (tests/golden/idcap: a family of 30 identical
    proteins), B's reads at the same indices have few or none; columns 4 - 7 of B through classify_verbose_packed == a fresh
    context's, the hit records == the oracle's"""
    api = gpu_lib
    d = os.path.join(golden.dir, "idcap")
    _, reads = util.read_fastq(os.path.join(d, "reads.fq"))
    idx = api.Index(os.path.join(d, "db.fmi"))
    oix, otax = oracle.load_fmi(os.path.join(d, "db.fmi")), oracle.load_nodes(golden.nodes)      # (the ids are compared, no LCA)
    nothing = H.nothing_reads(len(reads))
    few = [golden.reads[i] if i % 3 == 0 else nothing[i] if i % 3 == 1 else reads[i][: len(reads[i]) // 2] for i in range(len(reads))]
    A, B = util.pack(reads), util.pack(few)
    try:
        for seg in (1, 0):
            fresh = api.Classifier(idx, api.default_params(mode, seg=seg))
            h0, v0, p0, t0 = fresh.classify_verbose_packed(*B)
            fresh.close()
            want = oracle.classify(oix, otax, oracle.params(mode, seg=seg, use_evalue=0), *B)
            assert not vs_oracle(want, h0), (mode, seg)
            clf = api.Classifier(idx, api.default_params(mode, seg=seg))
            ha, va, _, ta = clf.classify_verbose_packed(*A)
            assert int(va["n_acc"].max()) == 20 and (va["text_len"] >= 11).all()        # (the residue is there)
            h1, v1, p1, t1 = clf.classify_verbose_packed(*B)
            assert (h1 == h0).all() and (v1["n_acc"] == v0["n_acc"]).all() and (v1["text_len"] == v0["text_len"]).all() and (v1["truncated"] == v0["truncated"]).all()
            k = np.arange(20)[None, :] < v0["n_acc"][:, None]
            assert (np.where(k, v1["acc_iseq"], 0) == np.where(k, v0["acc_iseq"], 0)).all()
            assert (p1 == p0).all() and t1 == t0, (mode, seg)
            # ... and an empty batch, then A again
            clf.classify_verbose_packed(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
            ha2, va2, _, ta2 = clf.classify_verbose_packed(*A)
            assert (ha2 == ha).all() and (va2["n_acc"] == va["n_acc"]).all() and ta2 == ta
            clf.close()
    finally:
        idx.close()


# ---- the text entry points ------------------------------------------------------------------------------------------------------
def fastq(names, reads):
    return b"".join(b"@" + n + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for n, r in zip(names, reads))


@pytest.mark.parametrize("mode", ["mem", "greedy"])
def test_text_entry_points_after_a_larger_block(gpu_lib, golden, worlds, mode):
    """classify_text_to_text, parse_block and format_compact on one context: a large block with long names, then a small block
    with short names, then a block of reads that are all unclassified; text, records and info structs == a fresh context's"""
    api, w = gpu_lib, worlds["golden"]
    short = [r for r in golden.reads if len(r) <= 150]
    big = fastq([b"a_long_read_name_with_a_lot_of_text_in_it_number_%06d/1 and a comment" % i for i in range(len(short))], short)
    small = fastq([b"r%d" % i for i in range(37)], short[5:42])
    none = fastq([b"u%d" % i for i in range(29)], [x for x in H.nothing_reads(60) if x][:29])
    blocks = (big, small, none, small)

    def run(clf, t):
        a = clf.classify_text_to_text(w.dtax, t)
        e = api.parse_block(clf, t)
        recs = clf.classify_compact(w.dtax, np.ascontiguousarray(e["seqs"], dtype=np.uint8), np.ascontiguousarray(e["off"], dtype=np.uint64))
        names = np.zeros(len(recs), dtype=api.NAME_SPAN_DTYPE)
        names["pos"], names["len"] = e["names"][:, 0], e["names"][:, 1]
        out, finfo = clf.format_compact(recs, e["off"], t, names)
        return (a["text"], a["info"].tobytes(), a["format_info"].tobytes(), e["seqs"].tobytes(), e["off"].tobytes(), e["names"].tobytes(),
                e["info"].tobytes(), recs.tobytes(), bytes(out[: int(finfo["text_bytes"])]), finfo.tobytes())

    solo = []
    for t in blocks:
        c = w.classifier(mode, 1)
        solo.append(run(c, t))
        c.close()
    assert solo[0][0].count(b"\n") == len(short) and b"C\t" in solo[0][0] and solo[2][0].count(b"U\t") == 29 and b"C\t" not in solo[2][0]
    assert solo[1][0] == solo[1][8]                                  # (both routes to the text agree)
    clf = w.classifier(mode, 1)
    for k, t in enumerate(blocks):
        got = run(clf, t)
        assert got == solo[k], (mode, k, [i for i in range(len(got)) if got[i] != solo[k][i]])
    clf.close()
