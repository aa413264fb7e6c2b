"""Inputs and the reference loop shared by tests/test_read_profile_host.py and tests/test_gpu_device_profile.py (no test here).

`profile_case()` is `report_cases.report_case()` - imported, unchanged, so the tile layout is inherited: a read boundary on a tile
edge, five reads in one tile, a read over whole tiles, empty reads first, in the middle and last, ~2.8 k events - with, on top,
  * ~240 planted confidences in windows outside w0 .. w0 + 32: every step thr[k] of cli.phred_thresholds(), one ulp below and one
    ulp above it, written at the class the quality reads (clip(a1, 0, 5) / clip(a2, 0, 4)) in model 1 with model 2 at 1.0 and the
    other way round, so that either model decides min(p1, p2) on every one of them; and values of Phred 1 and Phred 40 in model 1;
  * ~30 original bases 'N' and 10 'a', which count as "other".
NaN stays away from the gathered class as in `report_case`.  The helper asserts what the case claims: all 40 Phred bins 1 .. 40
are populated, `phred_chars` and `phred_lookup` agree on every planted value, and "other" is non-zero.
`loop_profile` is the per-read, per-event restatement of the rule text of include/nanorev.h in plain Python: it shares no code with
hoststage (no emit_calls, no merge_calls, no read_profile)."""
import numpy as np

from nanoreviser_amd import cli
from report_cases import LAB, T, report_case


def window_qc(c):
    """The Phred character of every window of a case, as the device computes it: the thresholds on min(p1[clip a1], p2[clip a2])."""
    i = np.arange(c["n"])
    return cli.phred_lookup(np.minimum(c["p1"][i, np.clip(c["a1"], 0, 5)], c["p2"][i, np.clip(c["a2"], 0, 4)]))


def profile_case(seed=2604):
    c = report_case(seed)
    rng = np.random.default_rng(seed + 1)
    thr = cli.phred_thresholds()
    n, w0 = c["n"], c["w0"]
    one, zero = np.float32(1), np.float32(0)
    both_ways = np.concatenate([thr, np.nextafter(thr, zero), np.nextafter(thr, one)]).astype(np.float32)
    m1_only = np.array([0.0, 0.1, 0.2056, 0.9999, 0.99995, 1.0], np.float32)
    vals = np.concatenate([both_ways, m1_only, both_ways])
    in_m1 = np.concatenate([np.ones(both_ways.size + m1_only.size, bool), np.zeros(both_ways.size, bool)])
    free = np.setdiff1d(np.arange(n), np.arange(w0, w0 + 32))
    # a planted window must emit something: not the pair (1, 0), which deletes the base
    free = free[~((c["a1"][free] == 1) & (c["a2"][free] == 0))]
    ws = rng.choice(free, vals.size, replace=False)
    g1, g2 = np.clip(c["a1"][ws], 0, 5), np.clip(c["a2"][ws], 0, 4)
    c["p1"][ws, g1] = np.where(in_m1, vals, one)
    c["p2"][ws, g2] = np.where(in_m1, one, vals)
    ev = rng.choice(c["N"], 40, replace=False)
    c["bases"][ev[:30]], c["bases"][ev[30:]] = ord("N"), ord("a")
    c["planted"], c["planted_conf"] = ws, vals
    c["qc"] = window_qc(c)
    # what the case claims
    conf = vals.reshape(-1, 1)
    assert np.array_equal(cli.phred_chars(conf, conf), cli.phred_lookup(vals))
    assert np.array_equal(c["qc"][ws], cli.phred_lookup(vals))
    prof = loop_profile(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"])
    assert (prof[:, 1:41].sum(0) > 0).all() and not prof[:, 0].any() and not prof[:, 41].any()
    assert prof[:, 46].sum() > 0
    return c


def loop_profile(bases, ev_len, a1, a2, qc, T=T):
    """uint64[n_reads][48] by the rule text, one read and one event at a time.  qc: the Phred character of every window."""
    o = (T - 1) // 2
    clip = lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)
    prof = np.zeros((len(ev_len), 48), np.uint64)
    ev_off = 0
    for r, L in enumerate(int(x) for x in ev_len):
        row = [0] * 48
        n_r = max(L - T, 0)
        for j in range(L):
            orig = chr(bases[ev_off + j])
            if not (o <= j < o + n_r):
                chars, q = [orig], ord("#") - 33
            else:
                w = ev_off + (j - o)
                x, y = int(a1[w]), int(a2[w]) + 1
                if x == y and x >= 2:
                    chars = [LAB[clip(x, 0, 5)]]
                elif x == 0 and y >= 2:
                    chars = [orig, LAB[clip(y, 0, 5)]]
                elif x == 1 and y == 1:
                    chars = []
                else:
                    chars = [orig]
                q = clip(int(qc[w]) - 33, 0, 41)
            for ch in chars:
                row[q] += 1
                row[42 + ("ACGT".index(ch) if ch in "ACGT" else 4)] += 1
        prof[r] = row
        ev_off += L
    return prof
