"""Inputs and the reference loop shared by tests/test_score_host.py and tests/test_gpu_device_score.py (no test here).

`score_case(seed, T)` is `report_cases.report_case(seed, T)` - a read boundary on a tile edge, five reads in one tile of 256
events, a read over whole tiles, reads without events first, in the middle and last, out-of-range a1 / a2 and NaN rows - with
label bytes planted on top (read indices are those of `report_cases.ev_len_for`):
  * seeded random VALID bytes everywhere: codes 1 .. 5 x bit 3 x bit 4; all twenty values once more in a row in read 10;
  * 0xFF runs at both ends of reads 8, 10, 11 and 13, reaching past the edge events into the windows (a clip), and one in the
    middle of read 11; read 9 is unlabelled altogether;
  * bytes with the codes 0, 6 and 7 (never labelled, whatever their other bits) and bytes with bits 5 .. 7 set whose code is
    valid (labelled: only 0xFF itself means "no label");
  * in read 13, windows whose p[w][y] - and, a1 / a2 set to the true class, whose p[w][c] - is 0, 1.0, a denormal, NaN, +Inf,
    a negative, a value above 1, and `nextafter` either side of three `score_thr` entries (and the entries themselves).
`loop_score` is the per-read, per-window restatement of the rule text of include/nanorev.h
(nrv_revise_reads_raw_score_begin) in plain Python: it shares no code with hoststage."""
import struct

import numpy as np

import report_cases

VALID = [c | b3 | b4 for c in range(1, 6) for b3 in (0, 8) for b4 in (0, 16)]
NEVER = [0x00, 0x08, 0x10, 0x18, 0x06, 0x07, 0x0E, 0x1F, 0x26, 0xF8, 0xFE]      # codes 0, 6 and 7
HIGH_BITS = [0x20 | 3, 0x40 | 5 | 8, 0x80 | 1, 0xE0 | 2 | 16, 0xE0 | 4 | 8 | 16]  # codes 3, 5, 1, 2, 4: labelled
LAB = "D-CTGA"


def score_thr():
    from nanoreviser_amd.cli import phred_thresholds
    return np.array(phred_thresholds(), np.float32)


def score_case(seed=2604, T=report_cases.T):
    c = dict(report_cases.report_case(seed, T))
    for k in ("a1", "a2", "p1", "p2"):
        c[k] = c[k].copy()
    rng = np.random.default_rng(seed + 77)
    el, N, n = c["ev_len"], c["N"], c["n"]
    o = (T - 1) // 2
    ev_off = np.cumsum(el) - el
    thr = score_thr()
    lab = np.array(VALID, np.uint8)[rng.integers(0, len(VALID), N)]
    for r in (8, 10, 11, 13):                                   # clips: past the edge events at either end
        lab[ev_off[r]:ev_off[r] + o + 3] = 0xFF
        lab[ev_off[r] + el[r] - (T - o) - 4:ev_off[r] + el[r]] = 0xFF
    lab[ev_off[11] + 300:ev_off[11] + 310] = 0xFF               # ... and a run in the middle
    lab[ev_off[9]:ev_off[9] + el[9]] = 0xFF                     # a fully unlabelled read
    e0 = int(ev_off[10]) + o + 40                               # events that are window centres of read 10
    lab[e0:e0 + len(VALID)] = VALID
    lab[e0 + 30:e0 + 30 + len(NEVER)] = NEVER
    lab[e0 + 50:e0 + 50 + len(HIGH_BITS)] = HIGH_BITS
    # planted probabilities, read 13: window w has its centre at event w + o
    near = []
    for k in (0, 17, 38):
        near += [np.nextafter(thr[k], np.float32(0)), thr[k], np.nextafter(thr[k], np.float32(2))]
    vals = [np.float32(0), np.float32(1), np.float32(1e-40), np.float32(np.nan), np.float32(np.inf), np.float32(-0.25),
            np.float32(1.5), np.float32(0.5), np.float32(2.0 ** -126), np.float32(-0.0)] + near
    w = int(ev_off[13]) + 60
    for i, v in enumerate(vals):
        for own in (False, True):                               # own: the models answer the true class, so p[w][c] is v too
            code = 1 + (i + own) % 5
            byte = code | (16 if (i % 3 == 0) else 0)
            lab[w + o] = byte
            y1, y2 = (0 if byte & 16 else code), code - 1
            c["p1"][w, y1], c["p2"][w, y2] = v, v
            if own:
                c["a1"][w], c["a2"][w] = y1, y2
            w += 1
    assert w < ev_off[13] + el[13] - T - 20
    c["labels"], c["score_thr"] = lab, thr
    return c


def loop_nll16(p):
    u = struct.unpack("<I", struct.pack("<f", float(np.float32(p))))[0] if not isinstance(p, int) else p
    e, m = (u >> 23) & 255, u & 0x7FFFFF
    if (u >> 31) or e == 0 or e == 255:
        return 127 << 16
    if e >= 127:
        return 0
    y, f = (1 << 23) | m, 0
    for _ in range(16):
        y = (y * y) >> 23
        f <<= 1
        if y >= 1 << 24:
            f |= 1
            y >>= 1
    return ((127 - e) << 16) - f


def _bits(p):
    return int(np.array(p, np.float32).view(np.uint32))


def _bin(thr, p):
    p = np.float32(p)
    return sum(1 for t in thr if np.float32(t) <= p)            # a NaN compares false: bin 0


def loop_score(bases, ev_len, a1, a2, p1, p2, labels, thr, T):
    """uint64[n_reads][248] by the rule text, one read and one window at a time."""
    o = (T - 1) // 2
    clip = lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)
    out = np.zeros((len(ev_len), 248), np.uint64)
    ev_off = 0
    for r, L in enumerate(int(x) for x in ev_len):
        row = [0] * 248
        n_r = max(L - T, 0)
        row[0] = n_r
        for i in range(n_r):
            w, j = ev_off + i, o + i
            lb = int(labels[ev_off + j])
            code = lb & 7
            if lb == 0xFF or not 1 <= code <= 5:
                continue
            row[1] += 1
            y1 = 0 if lb & 16 else code
            y2 = code - 1
            x, y = int(a1[w]), int(a2[w]) + 1
            c1, c2 = clip(int(a1[w]), 0, 5), clip(int(a2[w]), 0, 4)
            row[2 + 6 * y1 + c1] += 1
            row[38 + 5 * y2 + c2] += 1
            if p1 is not None and p2 is not None:
                b1, b2 = _bin(thr, p1[w][c1]), _bin(thr, p2[w][c2])
                row[63 + b1] += 1
                row[103 + b1] += c1 == y1
                row[143 + b2] += 1
                row[183 + b2] += c2 == y2
                row[223] += loop_nll16(_bits(p1[w][y1]))
                row[224] += loop_nll16(_bits(p2[w][y2]))
            orig = chr(bases[ev_off + j])
            if x == y and x >= 2:
                d = 0 if LAB[clip(x, 0, 5)] == orig else 1
            elif x == 0 and y >= 2:
                d = 2
            elif x == 1 and y == 1:
                d = 3
            else:
                d = 4
            k = 3 if lb & 16 else (2 if code == 1 else (1 if lb & 8 else 0))
            row[225 + 4 * d + k] += 1
            row[245] += d == 1 and clip(x, 0, 5) == code
        out[r] = row
        ev_off += L
    return out


_CASES = {}


def cached_case(seed=2604, T=report_cases.T):
    """(case, loop_score with rows, loop_score without), computed once per process and left unchanged."""
    if (seed, T) not in _CASES:
        c = score_case(seed, T)
        args = (c["bases"], c["ev_len"], c["a1"], c["a2"])
        _CASES[seed, T] = (c, loop_score(*args, c["p1"], c["p2"], c["labels"], c["score_thr"], T),
                           loop_score(*args, None, None, c["labels"], c["score_thr"], T))
    return _CASES[seed, T]
