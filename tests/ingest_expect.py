"""What record extraction must produce for one text: the reading loop of BlockCursor::next (csrc/host/kaiju_main.cpp; the
reference's kaiju.cpp:288-386) with positions, format and keep_names as arguments; and the buffers parse_blocks makes of
one or two such texts.  Shared by tests/test_ingest_emu.py and tests/test_gpu_ingest.py."""
import numpy as np

NO_MISMATCH = 0xffffffff


def ref_spans(text: bytes, fastq: bool, keep_names: bool = False):
    """list of (name position, name length, stripped sequence)"""
    starts, p = [], 0
    while p < len(text):
        e = text.find(b"\n", p)
        e = len(text) if e < 0 else e
        starts.append((p, e))
        p = e + 1
    strip = lambda s: bytes(c for c in s if (65 <= c <= 90) or (97 <= c <= 122))
    i, out = 0, []
    while True:
        while i < len(starts) and starts[i][0] == starts[i][1]:
            i += 1
        if i >= len(starts):
            break
        a, e = starts[i]
        i += 1
        name = text[a + 1:e]
        if not keep_names:
            for k, ch in enumerate(name):
                if ch in b" /\t\r":
                    name = name[:k]
                    break
        if fastq:
            seq = strip(text[starts[i][0]:starts[i][1]]) if i < len(starts) else b""
            i += 3
        else:
            j = i
            while j < len(starts) and text[starts[j][0]:starts[j][0] + 1] != b">":
                j += 1
            seq = strip(text[starts[i][0]:starts[j - 1][1]]) if j > i else b""
            i = j
        out.append((a + 1, len(name), seq))
    return out


def expected(text1: bytes, text2, fastq: bool, keep_names: bool = False, rec_cap=None):
    r1 = ref_spans(text1, fastq, keep_names)
    r2 = ref_spans(text2, fastq, keep_names) if text2 is not None else None
    n = len(r1) if r2 is None else min(len(r1), len(r2))
    total = n
    if rec_cap is not None:
        n = min(n, rec_cap)
    seqs, off, mismatch, max_mate = bytearray(), [0], NO_MISMATCH, 0
    for r in range(n):
        seqs += r1[r][2]
        off.append(len(seqs))
        if r2 is not None:
            seqs += r2[r][2]
            a, b = r1[r], r2[r]
            if mismatch == NO_MISMATCH and text1[a[0]:a[0] + a[1]] != text2[b[0]:b[0] + b[1]]:
                mismatch = r
            max_mate = max(max_mate, len(b[2]))
        off.append(len(seqs))
        max_mate = max(max_mate, len(r1[r][2]))
    return {"seqs": np.frombuffer(bytes(seqs), dtype=np.uint8), "off": np.array(off, dtype=np.uint64),
            "names": np.array([(a, l) for a, l, _ in r1[:n]], dtype=np.uint32).reshape(n, 2),
            "n_records": len(r1), "n_records2": len(r2) if r2 is not None else 0, "max_mate_len": max_mate,
            "name_mismatch": mismatch, "seq_bytes": len(seqs), "overflow": 1 if (rec_cap is not None and total > rec_cap) else 0}
