"""Inputs and the reference loop shared by tests/test_revision_report_host.py and tests/test_gpu_device_report.py (no test here).

`report_case(T=11)` is ONE call of ~2.8 k events.  The order of the read lengths (`ev_len_for(T)`) is chosen for the device
kernel's tiles of 256 events: the first non-empty read ends on a tile edge (256), tile 1 holds the reads of T - 1, T, T + 1, 1 and
T + 2 events and the head of the next, every later boundary falls mid-tile, the read of 3 * 256 + 5 events covers whole tiles,
and reads without events stand first, in the middle and last.  At the shipped T = 11 the lengths are the mix {0, 1, 10, 11, 12,
13, 255, 256, 257, 600} plus that read (`EV_LEN`); tests/test_window_lengths_host.py pins those arrays by their sha256.
`loop_report` is the per-read, per-window restatement of the rule text of include/nanorev.h in plain Python: it shares no code
with hoststage (no emit_calls, no merge_calls)."""
import numpy as np

T = 11
TIE_EPS = 4e-4
LAB = "D-CTGA"


def ev_len_for(T):
    """The read lengths of `report_case(T)`: reads of T - 1, T (no window), T + 1 (one) and T + 2 events share tile 1."""
    return [max(x, 0) for x in (0, 256, 0, T - 1, T, T + 1, 1, T + 2, 255, 257, 600, 3 * 256 + 5, 0, 600, 0)]


EV_LEN = ev_len_for(T)
assert EV_LEN == [0, 256, 0, 10, 11, 12, 1, 13, 255, 257, 600, 3 * 256 + 5, 0, 600, 0]


def report_case(seed=2604, T=T):
    rng = np.random.default_rng(seed)
    el = np.array(ev_len_for(T), np.int64)
    N = int(el.sum())
    n = N - T
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, N)].copy()
    # calls: half of the windows say what the basecaller said (so that every class of the merge is well populated)
    lab_of = {ord("C"): 2, ord("T"): 3, ord("G"): 4, ord("A"): 5}
    a1 = rng.integers(0, 6, n).astype(np.int8)
    a2 = rng.integers(0, 5, n).astype(np.int8)
    centre = np.array([lab_of[b] for b in bases[(T - 1) // 2:(T - 1) // 2 + n]], np.int8)
    same = rng.random(n) < 0.5
    a1[same] = centre[same]
    agree = same & (rng.random(n) < 0.7)
    a2[agree] = centre[agree] - 1
    odd = rng.choice(n, 40, replace=False)                       # out-of-range labels, clipped as the merge clips them
    a1[odd[:10]], a1[odd[10:20]], a2[odd[20:30]], a2[odd[30:]] = -3, 9, -3, 9
    a1[odd[5]], a2[odd[5]] = 9, 8                                # x == y == 9: an agreement on the clipped label
    # rows with well separated values (top1 - top2 ~ 0.3), so that the near-ties are the planted ones and no others
    p1 = (rng.permuted(np.tile([0.5, 0.2, 0.12, 0.08, 0.06, 0.04], (n, 1)), axis=1) + 0.004 * rng.random((n, 6))).astype(np.float32)
    p2 = (rng.permuted(np.tile([0.5, 0.2, 0.14, 0.1, 0.06], (n, 1)), axis=1) + 0.004 * rng.random((n, 5))).astype(np.float32)
    e = np.float32(TIE_EPS)
    lo, hi = np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(1))
    w0 = int(el[:10].sum()) + 20                                 # windows in the middle of the first read of 600 events
    p1[w0:w0 + 8], p2[w0:w0 + 8] = 0, 0
    p1[w0:w0 + 8, 0], p2[w0:w0 + 8, 0] = 1, 1                    # margin 1 in both models unless overwritten below
    p1[w0 + 0, 3] = 1                                            # an exact tie (model 1)
    p2[w0 + 1, 4] = 1                                            # an exact tie (model 2)
    p1[w0 + 2] = [0, 0, lo, 0, 0, 0]                             # one ulp below tie_eps: a near-tie
    p1[w0 + 3] = [0, 0, 0, e, 0, 0]                              # exactly tie_eps: not one
    p1[w0 + 4] = [0, hi, 0, 0, 0, 0]                             # one ulp above: not one
    p2[w0 + 5] = [0, lo, 0, 0, 0]
    p2[w0 + 6] = [0, 0, 0, hi, 0]
    p1[w0 + 7, 2] = np.nan                                       # a NaN row
    p2[w0 + 30, 0] = np.nan
    p1[w0 + 31] = np.nan
    # ... but never at the class the quality is read from: min(p1[a1], p2[a2]) stays a number
    a1[w0 + 7], a2[w0 + 30] = 0, 1
    p1[w0 + 31, min(max(int(a1[w0 + 31]), 0), 5)] = 0.5
    qc = rng.integers(34, 74, n).astype(np.uint8)
    return {"bases": bases, "ev_len": el, "a1": a1, "a2": a2, "p1": p1, "p2": p2, "qc": qc, "N": N, "n": n, "w0": w0}


def _near_tie_row(row, eps):
    vals = [np.float32(v) for v in row]
    if any(v != v for v in vals):
        return True
    vals.sort()
    with np.errstate(invalid="ignore"):
        return not (np.float32(vals[-1] - vals[-2]) >= np.float32(eps))


def loop_report(bases, ev_len, a1, a2, p1, p2, qc, T=T, tie_eps=TIE_EPS):
    """uint64[n_reads][24] by the rule text, one read and one window at a time."""
    o = (T - 1) // 2
    clip = lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)
    rep = np.zeros((len(ev_len), 24), np.uint64)
    ev_off = 0
    for r, L in enumerate(int(x) for x in ev_len):
        row = [0] * 24
        n_r = max(L - T, 0)
        row[0], row[1], row[3] = L, n_r, L - n_r
        out = q_sum = 0
        for j in range(L):
            if not (o <= j < o + n_r):
                out += 1
                q_sum += ord("#") - 33
                continue
            w = ev_off + (j - o)
            orig = chr(bases[ev_off + j])
            x, y = int(a1[w]), int(a2[w]) + 1
            if x == y and x >= 2:
                k = 1
                row[4 if LAB[clip(x, 0, 5)] == orig else 5] += 1
            elif x == 0 and y >= 2:
                k = 2
                row[6] += 1
            elif x == 1 and y == 1:
                k = 0
                row[7] += 1
            else:
                k = 1
                row[8] += 1
            out += k
            row[9 + clip(int(a1[w]), 0, 5)] += 1
            row[15 + clip(int(a2[w]), 0, 4)] += 1
            row[20] += LAB[clip(y, 0, 5)] == orig
            if p1 is not None and p2 is not None:
                row[21] += _near_tie_row(p1[w], tie_eps) or _near_tie_row(p2[w], tie_eps)
            if qc is not None:
                q_sum += k * (int(qc[w]) - 33)
        row[2] = out
        row[22] = q_sum if qc is not None else 0
        rep[r] = row
        ev_off += L
    return rep
