"""Inputs and the reference loop shared by tests/test_revision_edits_host.py and tests/test_gpu_device_edits.py (no test here).

`loop_edits` is the per-read, per-window restatement of the rule text of include/nanorev.h (nrv_edit) in plain Python: it
shares no code with hoststage (no revision_edits, no emit_calls, no merge_calls).  `density_case` builds calls whose every
window is a deletion, an insertion or no edit at all; `carry_case` is one call of 257 * 256 + 3 events in four reads, one of which
spans more than 256 tiles of 256 events: the smallest shape at which the device's tile scan carries across its 256-wide passes."""
import struct

import numpy as np

from report_cases import LAB, T

EDIT_DTYPE = np.dtype([("pos_in", "<u4"), ("pos_out", "<u4"), ("kind", "u1"), ("ref", "u1"), ("alt", "u1"), ("qual", "u1"), ("conf", "<f4")])


def loop_edits(bases, ev_len, a1, a2, p1, p2, qc, T=T):
    """(records as 16-byte strings joined, edit_off list) by the rule text, one read and one window at a time."""
    o = (T - 1) // 2
    clip = lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)
    blob, edit_off, ev_off = [], [0], 0
    for L in (int(x) for x in ev_len):
        n_r = max(L - T, 0)
        out = 0                                                   # characters of the revised read emitted so far
        for j in range(L):
            if not (o <= j < o + n_r):
                out += 1
                continue
            w = ev_off + (j - o)
            orig = chr(bases[ev_off + j])
            x, y = int(a1[w]), int(a2[w]) + 1
            kind = alt = k = None
            if x == y and x >= 2:
                k = 1
                if LAB[clip(x, 0, 5)] != orig:
                    kind, alt = 1, LAB[clip(x, 0, 5)]
            elif x == 0 and y >= 2:
                k, kind, alt = 2, 2, LAB[clip(y, 0, 5)]
            elif x == 1 and y == 1:
                k, kind, alt = 0, 3, "-"
            else:
                k = 1
            if kind is not None:
                conf = np.float32(0)
                if p1 is not None and p2 is not None:
                    u, v = np.float32(p1[w][clip(int(a1[w]), 0, 5)]), np.float32(p2[w][clip(int(a2[w]), 0, 4)])
                    conf = v if v < u else u
                blob.append(struct.pack("<IIBBBB", j, out, kind, ord(orig), ord(alt), int(qc[w]) if qc is not None else 0)
                            + np.float32(conf).tobytes())
            out += k
        edit_off.append(len(blob))
        ev_off += L
    return b"".join(blob), edit_off


def replay(orig, records):
    """A read's records applied to its original bases (bytes): substitute at pos_in, insert alt behind it, delete it."""
    by_pos = {int(e["pos_in"]): e for e in records}
    out = bytearray()
    for j, b in enumerate(orig):
        e = by_pos.get(j)
        if e is None:
            out.append(b)
        elif e["kind"] == 1:
            out.append(int(e["alt"]))
        elif e["kind"] == 2:
            out += bytes([b, int(e["alt"])])
    return bytes(out)


def _rows(rng, n):
    p1 = rng.random((n, 6)).astype(np.float32)
    p2 = rng.random((n, 5)).astype(np.float32)
    return p1, p2


def density_case(what, ev_len=(0, 300, 0, 13, 256, 700, 0), seed=7, T=T):
    """`what`: "deletion" (a1 = 1, a2 = 0 everywhere), "insertion" (a1 = 0, a2 a base) or "none" (both models repeat the basecaller)."""
    rng = np.random.default_rng(seed)
    el = np.array(ev_len, np.int64)
    N = int(el.sum())
    n = max(N - T, 0)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, N)].copy()
    if what == "deletion":
        a1, a2 = np.full(n, 1, np.int8), np.zeros(n, np.int8)
    elif what == "insertion":
        a1, a2 = np.zeros(n, np.int8), rng.integers(1, 5, n).astype(np.int8)
    else:
        lab_of = {ord("C"): 2, ord("T"): 3, ord("G"): 4, ord("A"): 5}
        a1 = np.array([lab_of[b] for b in bases[(T - 1) // 2:(T - 1) // 2 + n]], np.int8)
        a2 = (a1 - 1).astype(np.int8)
    p1, p2 = _rows(rng, n)
    return {"bases": bases, "ev_len": el, "a1": a1, "a2": a2, "p1": p1, "p2": p2, "qc": rng.integers(34, 74, n).astype(np.uint8),
            "N": N, "n": n}


def carry_case(deletions, seed=9, T=T):
    """257 * 256 + 3 events in four reads; the second spans 256 * 256 + 100 events (more than 256 tiles)."""
    rng = np.random.default_rng(seed)
    el = np.array([90, 256 * 256 + 100, 0, 69], np.int64)
    N = int(el.sum())
    assert N == 257 * 256 + 3 and el[1] > 256 * 256 and (el >= 0).all()
    n = N - T
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, N)].copy()
    if deletions:
        a1, a2 = np.full(n, 1, np.int8), np.zeros(n, np.int8)
    else:
        a1, a2 = rng.integers(0, 6, n).astype(np.int8), rng.integers(0, 5, n).astype(np.int8)
    p1, p2 = _rows(rng, n)
    return {"bases": bases, "ev_len": el, "a1": a1, "a2": a2, "p1": p1, "p2": p2, "qc": rng.integers(34, 74, n).astype(np.uint8),
            "N": N, "n": n}
