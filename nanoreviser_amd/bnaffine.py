"""Fitting gamma and beta of the BatchNorms inside the fitted section: the DEFINITION of what the engine's nrv_fit_* entry points
compute while nrv_fit_set_bn_affine is on (include/nanorev.h, csrc/nrv_bnaffine.h).  NumPy only.

A BatchNorm inside the section (bnfit.inside(depth), in tensor order) is applied in its inference form on the CURRENT moving
statistics, y = x s + h with r = 1 / sqrt(var + eps), s = gamma r, h = beta - mean s; the fold is bnfit.fold - every step in f32,
no contraction.  gamma and beta are parameters.  THE STATED DEVIATION of the three depths remains: the statistics stay frozen
during a step, where Keras in training phase would normalise with the batch's; they move only by bnfit.reestimate.

THE VECTOR.  The block goes in FRONT of the depth's own vector: for every BatchNorm inside, in tensor order, gamma [C] then
beta [C] - 512 floats at lstm3 depth, 544 at signal depth, 864 at full depth (fitdepth.BN_BLOCK).

THE GRADIENT.  With dy the derivative of the batch's SUM of row losses by the BatchNorm's output, x the activation it normalises
and n the batch's rows, per channel
    g_gamma = r sum dy (x - mean) / n          g_beta = sum dy / n
over (row, t) for bn_l1 / bn_l2 / bn_l3 and over (row, t, the 50 samples) for bn_c1 / bn_c2.  The pivoted form IS the definition:
sum dy x - mean sum dy cancels, because x is about mean.  The five (dy, x) pairs are the `taps` of lstm3fit / signalfit /
fullfit; they are used, not restated.  Every other gradient is the depth's own on the folded pairs.

`x` is the depth's first row array - Xin [n][T][192] (lstm3), x2 [n][T][128] (signal), feat [n][T][6] (full) -, `sig` the
samples [n][T][50] (None at lstm3 depth), `stats` name -> (mean, var) f32: the current moving statistics."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import bnfit, fitdepth
from .bnfit import BATCHNORMS
from .lstm4fit import BN_EPS
from .tailfit import FitOpts, FitState, FitStats, adam_step

_CB, _RB, _L3 = ("bn_c1", "bn_c2"), ("bn_l1", "bn_l2"), ("bn_l3",)


def n_block(depth: str) -> int:
    """NRV_FIT_PARAMS_BN(depth): the block's floats."""
    return 2 * sum(BATCHNORMS[k][1] for k in bnfit.inside(depth))


def n_params(depth: str, T: int, C: int) -> int:
    return n_block(depth) + fitdepth.BY_NAME[depth].fit.n_params(T, C)


def spans(depth: str):
    """name -> (slice of gamma, slice of beta) in the vector."""
    out, at = {}, 0
    for k in bnfit.inside(depth):
        c = BATCHNORMS[k][1]
        out[k] = (slice(at, at + c), slice(at + c, at + 2 * c))
        at += 2 * c
    return out


def pack(depth: str, gb, theta, dtype=np.float32) -> np.ndarray:
    """gb: name -> (gamma, beta); theta: the depth's own vector."""
    front = [np.asarray(a, dtype).ravel() for k in bnfit.inside(depth) for a in gb[k]]
    return np.concatenate(front + [np.asarray(theta, dtype).ravel()])


def unpack(depth: str, vec, T: int, C: int):
    """-> ({name: (gamma, beta)}, the depth's own vector) (views)."""
    vec = np.asarray(vec)
    if vec.size != n_params(depth, T, C):
        raise ValueError(f"parameter vector of {vec.size} floats, expected {n_params(depth, T, C)} for T={T}, C={C} at {depth} depth "
                         "with the BatchNorm block in front")
    return {k: (vec[g], vec[b]) for k, (g, b) in spans(depth).items()}, vec[n_block(depth):]


def params_from_model(depth: str, m, dtype=np.float32) -> np.ndarray:
    """The model's own tensors base, base + 1 of every BatchNorm inside, then the depth's params_from_model: what
    nrv_fit_begin(params = NULL) starts from."""
    bn = bnfit.bn_of(m)
    return pack(depth, {k: bn[k][:2] for k in bnfit.inside(depth)}, fitdepth.BY_NAME[depth].fit.params_from_model(m, dtype), dtype)


def stats_of(m):
    """name -> (moving_mean, moving_variance) f32 of a model's five BatchNorms."""
    return {k: v[2:] for k, v in bnfit.bn_of(m).items()}


def pairs_of(depth: str, vec, stats, dtype=np.float32):
    """name -> (s, h) of every BatchNorm inside from the vector's gamma / beta and `stats`.  At float32 this IS bnfit.fold; any
    other dtype forms the same expression in that format (the tests differentiate a float64 loss)."""
    dt = np.dtype(dtype)
    vec = np.asarray(vec)
    out = {}
    for k, (g, b) in spans(depth).items():
        mean, var = stats[k]
        if dt == np.float32:
            out[k] = bnfit.fold(vec[g], vec[b], mean, var)
        else:
            s = vec[g].astype(dt) / np.sqrt(np.asarray(var).astype(dt) + dt.type(BN_EPS))
            out[k] = (s, vec[b].astype(dt) - np.asarray(mean).astype(dt) * s)
    return out


def _data(depth, x, sig):
    return (x,) if depth == "lstm3" else (x, sig)


def _bn_args(depth, pairs):
    """The BatchNorm arguments of the depth's functions, in their order: [rb,] [cb,] sc, sh."""
    out = ()
    if depth == "full":
        out += (pairs["bn_l1"] + pairs["bn_l2"],)
    if depth != "lstm3":
        out += (pairs["bn_c1"] + pairs["bn_c2"],)
    return out + pairs["bn_l3"]


def batch_terms(depth: str, x, sig, y, vec, stats, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64,
                fold_dtype=np.float32, drop=None):
    """One batch -> (g [block + P]: the gradient of L, FitStats of the batch with steps = nonfinite = 0).  drop: dropout.terms of
    the batch's set rows (signal and full depth): bn_c2's dy is then the masked dF."""
    dt = np.dtype(dtype)
    fit = fitdepth.BY_NAME[depth].fit
    theta = np.asarray(vec)[n_block(depth):]
    pairs = pairs_of(depth, vec, stats, fold_dtype)
    taps = {}
    fn = fit.batch_terms if depth == "full" else fit.batch_terms_dx
    out = fn(*_data(depth, x, sig), y, theta, *_bn_args(depth, pairs), T, C, opts, act, dt, taps=taps,
             **({} if drop is None else {"drop": drop}))
    g, st = out[0], out[1]
    n = dt.type(np.asarray(y).shape[0])
    front = []
    for k in bnfit.inside(depth):
        c = BATCHNORMS[k][1]
        dy, xa = taps[k]
        mean, var = [np.asarray(a).astype(dt) for a in stats[k]]
        r = dt.type(1) / np.sqrt(var + dt.type(BN_EPS))
        dy, xa = dy.reshape(-1, c), xa.reshape(-1, c)
        front += [r * (dy * (xa - mean)).sum(axis=0) / n, dy.sum(axis=0) / n]
    return np.concatenate([a.astype(dt) for a in front] + [g]), st


def epoch(depth: str, x, sig, y, state: FitState, order, stats, T: int, C: int, opts: FitOpts, act: int = 0,
          dtype=np.float64) -> FitStats:
    """tailfit.epoch's rule: consecutive batches of opts.B in the order of `order`, a batch with a non-finite gradient skipped
    and counted - it changes nothing -, statistics before each update.  The pairs are refolded from the new gamma, beta and the
    current statistics behind every update: batch_terms folds them from the vector it is given."""
    dt = np.dtype(dtype)
    order = np.asarray(order, np.int64).reshape(-1)
    x, y = np.asarray(x), np.asarray(y)
    sig = None if sig is None else np.asarray(sig)
    tot = FitStats()
    for s in range(0, order.size, opts.B):
        idx = order[s:s + opts.B]
        with np.errstate(all="ignore"):
            g, st = batch_terms(depth, x[idx], None if sig is None else sig[idx], y[idx], state.theta, stats, T, C, opts, act, dt)
        if not np.isfinite(g).all():
            tot.nonfinite += 1
            continue
        state.t += 1
        state.theta, state.m, state.v = adam_step(state.theta, state.m, state.v, g, opts, state.t, dt)
        st.steps = 1
        tot.add(st)
    return tot


def evaluate(depth: str, x, sig, y, vec, order, stats, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64,
             fold_dtype=np.float32):
    """-> (p [n][C], FitStats): forward only, on the pairs folded from the vector."""
    fit = fitdepth.BY_NAME[depth].fit
    pairs = pairs_of(depth, vec, stats, fold_dtype)
    return fit.evaluate(*_data(depth, x, sig), y, np.asarray(vec)[n_block(depth):], order, *_bn_args(depth, pairs), T, C, opts, act,
                        dtype)


def fitted_model(depth: str, m, vec, T: Optional[int] = None):
    """The depth's own fitted_model with gamma, beta of every BatchNorm inside written into tensors base, base + 1.  Moving mean
    and variance keep their bytes (bnfit.with_stats replaces those)."""
    from .weights import ModelWeights
    T = m.T if T is None else T
    vec = np.asarray(vec, np.float32)
    gb, theta = unpack(depth, vec, T, m.n_class)
    base_m = fitdepth.BY_NAME[depth].fit.fitted_model(m, theta, T)
    ts = list(base_m.tensors)
    for k, pair in gb.items():
        base = BATCHNORMS[k][0]
        for i, a in enumerate(pair):
            ts[base + i] = a.astype(np.float32).reshape(np.asarray(m.tensors[base + i]).shape).copy()
    return ModelWeights(ts, T, m.n_class, base_m.source + "+bnaffine")
