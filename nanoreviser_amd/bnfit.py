"""Re-estimating the BatchNorm statistics inside the fitted section from rows of the set: the DEFINITION of what the engine's
nrv_fit_bn_reestimate computes (include/nanorev.h, csrc/nrv_bnfit.h).  NumPy only.

The BatchNorms INSIDE the fitted section, in tensor order (gamma, beta, moving_mean, moving_variance each):
  lstm3 depth   bn_l3 (tensors 40 .. 43, 256 channels)
  signal depth  bn_c1 (2 .. 5, 8), bn_c2 (8 .. 11, 8), bn_l3
  full depth    bn_c1, bn_c2, bn_l1 (18 .. 21, 32), bn_l2 (28 .. 31, 128), bn_l3
Per channel, over the given rows (an index may repeat): the mean and the BIASED variance of the activation the BatchNorm
normalises - bn_c1: a1 = relu(conv1(sig) + b1) over (row, t, the 50 samples); bn_c2: a2 = relu(conv2(c1) + b2) likewise;
bn_l1 / bn_l2 / bn_l3: the RAW Bi-LSTM output H1 / H2 / H3 over (row, t) - at the model's CURRENT parameter vector.

THE SUMS.  With the pivot p = the LOADED moving mean (f32 widened to f64) and x the activation in the evaluation's format widened
to f64:  S1 = sum (x - p), S2 = sum (x - p)^2 in f64, m = S1 / N, mean = p + m, var = max(S2 / N - m m, 0), no contraction; mean
and var are rounded once to f32, because they become f32 tensors.

THE STAGES run in dependency order - {bn_c1, bn_l1}, {bn_c2, bn_l2}, {bn_l3} - and a BatchNorm is re-estimated with every
BatchNorm in front of it already replaced: behind a stage its (mean, var) are folded with the loaded gamma and beta to the
(s, h) pair of the inference form exactly as signalfit.conv_bn / fullfit.read_bn / the engine's bn_fold fold a loaded model, and
the next stage's activations are formed with those.  gamma and beta are never touched.  A second call on its own result returns
the same bytes: nothing a stage reads has changed.

The forward pieces are fullfit.read_branch, signalfit.branch / xin and lstm3fit.lstm; they are used, not restated.
"""
from __future__ import annotations

import numpy as np

from . import fullfit, lstm3fit, signalfit
from .lstm4fit import BN_EPS

BATCHNORMS = {"bn_c1": (2, 8), "bn_c2": (8, 8), "bn_l1": (18, 32), "bn_l2": (28, 128), "bn_l3": (40, 256)}   # first tensor, channels
_STAGES = (("bn_c1", "bn_l1"), ("bn_c2", "bn_l2"), ("bn_l3",))
_INSIDE = {"lstm3": ("bn_l3",), "signal": ("bn_c1", "bn_c2", "bn_l3"), "full": ("bn_c1", "bn_c2", "bn_l1", "bn_l2", "bn_l3")}


def inside(depth: str):
    """The BatchNorms inside the fitted section in tensor order: the `which` of nrv_fit_bn_get."""
    if depth not in _INSIDE:
        raise ValueError(f"no BatchNorm lies inside the fitted section at depth {depth!r}")
    return _INSIDE[depth]


def stages(depth: str):
    """The stages in dependency order, each a tuple of names; one pass over the rows each."""
    names = inside(depth)
    return tuple(s for s in (tuple(n for n in st if n in names) for st in _STAGES) if s)


def bn_of(m):
    """name -> (gamma, beta, moving_mean, moving_variance) f32 of a model's five BatchNorms."""
    return {k: tuple(np.asarray(m.tensors[base + i], np.float32).reshape(-1) for i in range(4)) for k, (base, _) in BATCHNORMS.items()}


def fold(gamma, beta, mean, var):
    """(s, h) f32 as the engine's bn_fold forms them: s = gamma / sqrt(var + eps), h = beta - mean s, every step in f32."""
    g, be, mu, v = [np.asarray(a, np.float32) for a in (gamma, beta, mean, var)]
    s = (g / np.sqrt(v + np.float32(BN_EPS))).astype(np.float32)
    return s, (be - mu * s).astype(np.float32)


def moments(x, pivot):
    """x [N][channels] in any format, pivot f32 [channels] -> dict(n, s1, s2 f64, mean, var f32) by THE SUMS above."""
    x = np.asarray(x)
    x = x.reshape(-1, x.shape[-1]).astype(np.float64)
    p = np.asarray(pivot, np.float32).astype(np.float64)
    n = x.shape[0]
    d = x - p
    s1, s2 = d.sum(axis=0), (d * d).sum(axis=0)
    m = s1 / np.float64(n)
    mean = p + m
    var = np.maximum(s2 / np.float64(n) - m * m, 0.0)
    return {"n": int(n), "s1": s1, "s2": s2, "mean": mean.astype(np.float32), "var": var.astype(np.float32)}


def activations(depth: str, names, x, sig, theta, pairs, T: int, C: int, act: int = 0, dtype=np.float64):
    """The activations the BatchNorms `names` of one stage normalise -> {name: [N][channels]}.  x: feat [n][T][6] (full), x2
    [n][T][128] (signal) or Xin [n][T][192] (lstm3); pairs: name -> the CURRENT (s, h) of every BatchNorm inside the section."""
    theta = np.asarray(theta)
    out = {}
    if depth == "lstm3":
        return {"bn_l3": lstm3fit.lstm(x, theta, T, C, act, dtype)[1].reshape(-1, 256)}
    th_sig = theta[fullfit.N_READ:] if depth == "full" else theta
    k = None
    if depth == "full":
        k = fullfit.read_branch(x, theta, pairs["bn_l1"] + pairs["bn_l2"], T, C, act, dtype)
        out["bn_l1"], out["bn_l2"] = k["H1"].reshape(-1, 32), k["H2"].reshape(-1, 128)
    br = signalfit.branch(sig, th_sig, pairs["bn_c1"] + pairs["bn_c2"], T, C, dtype)
    out["bn_c1"], out["bn_c2"] = br["a1"].reshape(-1, 8), br["a2"].reshape(-1, 8)
    if "bn_l3" in names:
        xin = signalfit.xin(k["X2b"] if depth == "full" else x, br["S"], T, dtype)
        out["bn_l3"] = lstm3fit.lstm(xin, th_sig[signalfit.N_SIGNAL:], T, C, act, dtype)[1].reshape(-1, 256)
    return {n: out[n] for n in names}


def reestimate(depth: str, x, sig, theta, bn, rows, T: int, C: int, act: int = 0, dtype=np.float64, acts=activations):
    """-> {name: dict(n, s1, s2, mean, var)} for every BatchNorm inside the section, in tensor order.  bn: bn_of(model), the LOADED tensors;
    rows: indices into x / sig; acts: another evaluation of `activations` (the tests' restatements)."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    if rows.size < 1:
        raise ValueError("no rows")
    x = np.asarray(x)[rows]
    sig = None if sig is None else np.asarray(sig)[rows]
    pairs = {n: fold(*bn[n]) for n in inside(depth)}
    out = {}
    for names in stages(depth):
        a = acts(depth, names, x, sig, theta, pairs, T, C, act, dtype)
        for n in names:
            out[n] = moments(a[n], bn[n][2])
            pairs[n] = fold(bn[n][0], bn[n][1], out[n]["mean"], out[n]["var"])
    return {n: out[n] for n in inside(depth)}


def folded(bn, stats):
    """name -> (s, h) f32 of every re-estimated BatchNorm: the pairs the fit runs on behind nrv_fit_bn_reestimate."""
    return {n: fold(bn[n][0], bn[n][1], st["mean"], st["var"]) for n, st in stats.items()}


def with_stats(m, stats):
    """The model with the moving_mean / moving_variance tensors of every BatchNorm in `stats` replaced; every other tensor keeps
    its bytes."""
    from .weights import ModelWeights
    ts = list(m.tensors)
    for n, st in stats.items():
        base = BATCHNORMS[n][0]
        for i, key in ((2, "mean"), (3, "var")):
            ts[base + i] = np.asarray(st[key], np.float32).reshape(np.asarray(m.tensors[base + i]).shape).copy()
    return ModelWeights(ts, m.T, m.n_class, m.source + "+bnfit")


def drift(bn, stats):
    """Per BatchNorm how far the statistics moved -> {name: dict(n, max_dmean_sigma: the largest |new mean - old mean| /
    sqrt(old var + eps), var_ratio_min / var_ratio_max: the range of new var / old var over its channels)}."""
    out = {}
    for n, st in stats.items():
        mu, var = bn[n][2].astype(np.float64), bn[n][3].astype(np.float64)
        ratio = st["var"].astype(np.float64)[var > 0] / var[var > 0]          # (a channel loaded with variance 0 has no ratio)
        ratio = ratio if ratio.size else np.ones(1)
        out[n] = {"n": int(st["n"]), "max_dmean_sigma": float(np.max(np.abs(st["mean"].astype(np.float64) - mu) / np.sqrt(var + BN_EPS))),
                  "var_ratio_min": float(np.min(ratio)), "var_ratio_max": float(np.max(ratio))}
    return out
