"""Fitting the signal branch with lstm3 and everything behind it: the DEFINITION of what the engine's nrv_fit_* entry points
compute at depth NRV_FIT_SIGNAL (include/nanorev.h, csrc/nrv_signalfit.h).  NumPy only.

Fitted are the signal branch's own tensors - conv1.kernel [3][1][8] (tensor 0), conv1.bias [8] (1), conv2.kernel [3][8][8] (6),
conv2.bias [8] (7), sig_dense.kernel [400][64] (32), sig_dense.bias [64] (33) - and everything lstm3fit.py fits (tensors
34 .. 39, 44 .. 59 and the centres).  lstm1, lstm2 and their BatchNorms (12 .. 31) are frozen, so a window IS the pair
(x2 [T][128], sig [T][50]): the BatchNorm'd f32 lstm2 output and the normalised samples of the window's T events.  One vector
per model,
  [w1 24 | b1 8 | w2 192 | b2 8 | Ws 25600 | bs 64 | lstm3fit's vector]       n_params(T, C) = 25896 + lstm3fit.n_params(T, C).

TWO STATED DEVIATIONS from Keras in training phase.
 1. The three BatchNorms inside the fitted section (tensors 2 .. 5, 8 .. 11 and 40 .. 43) are FROZEN and applied in their
    inference form from the moving statistics, exactly as lstm3fit.py treats 40 .. 43: behind a convolution that is
    relu(conv) * s + h, one multiply and one add.  The written model's BatchNorm tensors are the loaded ones, byte for byte.
    (s1, h1, s2, h2) - `cb` - and (sc, sh) are arguments of every numeric function here.
 2. The reference's Dropout(0.2) behind the identity block is not applied.  This deviation holds only while the switch is off:
    with `drop = (mask, keepf)` (dropout.py; nrv_fit_set_dropout on the device) batch_terms* and epoch drop F as the reference
    does - Fd = F / keepf where kept, else 0, and dF likewise on the way back.  drop = None changes nothing by a bit; evaluate
    never drops.

Forward, for each (row, t), p = 0 .. 49 a sample, o a channel; padding is `same`, out-of-range taps are zero:
  a1[p][o] = relu(b1[o] + sum_k sig[p + k - 1] w1[k][o])                 c1 = a1 * s1 + h1
  a2[p][o] = relu(b2[o] + sum_{k, ci} c1[p + k - 1][ci] w2[k][ci][o])    F[p * 8 + o] = a2 * s2 + h2 + sig[p]
  S = F Ws + bs                                                          Xin = [x2 | S], then lstm3fit.forward.
Everything behind Xin IS lstm3fit's: loss, options, Adam step, epoch order and files are used, not restated.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import dropout, headfit, lstm3fit, lstm4fit, tailfit  # noqa: F401
from .lstm4fit import BN_EPS
from .tailfit import (FitOpts, FitState, FitStats, adam_step, default_opts, epoch_order, lr_t, val_split,  # noqa: F401
                      write_f32)

N_SIG_IN, N_CH, N_FLAT, N_S = 50, 8, 400, 64
_SHAPES = ((3, N_CH), (N_CH,), (3, N_CH, N_CH), (N_CH,), (N_FLAT, N_S), (N_S,))
N_SIGNAL = sum(int(np.prod(s)) for s in _SHAPES)               # 25896
_TENSOR_IDS = (0, 1, 6, 7, 32, 33)


def n_params(T: int, C: int) -> int:
    """NRV_FIT_PARAMS_SIGNAL(T, C)."""
    return N_SIGNAL + lstm3fit.n_params(T, C)


def pack(w1, b1, w2, b2, Ws, bs, *rest, dtype=np.float32) -> np.ndarray:
    """The six signal-branch tensors, then lstm3fit.pack's twenty-three."""
    return np.concatenate([np.asarray(a, dtype).ravel() for a in (w1, b1, w2, b2, Ws, bs)] + [lstm3fit.pack(*rest, dtype=dtype)])


def unpack(theta, T: int, C: int):
    """-> [w1 [3][8], b1, w2 [3][8][8], b2, Ws [400][64], bs] + lstm3fit.unpack's list (views)."""
    theta = np.asarray(theta)
    if theta.size != n_params(T, C):
        raise ValueError(f"parameter vector of {theta.size} floats, expected {n_params(T, C)} for T={T}, C={C} at signal depth")
    out, at = [], 0
    for s in _SHAPES:
        n = int(np.prod(s))
        out.append(theta[at:at + n].reshape(s))
        at += n
    return out + lstm3fit.unpack(theta[at:], T, C)


def params_from_model(m, dtype=np.float32) -> np.ndarray:
    """A model's own tensors 0, 1, 6, 7, 32 .. 39 and 44 .. 59 with zero centres: what nrv_fit_begin(params = NULL) starts from
    at signal depth."""
    t = m.tensors
    return np.concatenate([np.asarray(t[i], dtype).ravel() for i in _TENSOR_IDS] + [lstm3fit.params_from_model(m, dtype)])


def with_lstm3(theta, theta_lstm3) -> np.ndarray:
    """theta with everything behind the signal branch replaced by a vector of lstm3fit's layout."""
    out = np.array(theta, np.float32)
    out[N_SIGNAL:] = np.asarray(theta_lstm3, np.float32)
    return out


def conv_bn(m):
    """(s1, h1, s2, h2) f32 [8] each: the two frozen BatchNorms of the conv block (tensors 2 .. 5 and 8 .. 11) as the engine's
    bn_fold forms them."""
    out = []
    for base in (2, 8):
        g, be, mu, var = [np.asarray(m.tensors[base + i], np.float32) for i in range(4)]
        s = (g / np.sqrt(var + np.float32(BN_EPS))).astype(np.float32)
        out += [s, (be - mu * s).astype(np.float32)]
    return tuple(out)


# ---- forward, loss, gradient ---------------------------------------------------------------------------------------------
def branch(sig, theta, cb, T: int, C: int, dtype=np.float64, drop=None):
    """-> dict(sig [n][T][50], z1 / a1 / c1 [n][T][50][8], z2 / a2, F [n][T][400], S [n][T][64]); z are the conv
    pre-activations.  drop = (mask uint8 [n][T][400], keepf): F is the DROPPED F, what S and gWs are formed from."""
    dt = np.dtype(dtype)
    w1, b1, w2, b2, Ws, bs = [a.astype(dt) for a in unpack(theta, T, C)[:6]]
    s1, h1, s2, h2 = [np.asarray(a).astype(dt) for a in cb]
    sig = np.asarray(sig).astype(dt).reshape(-1, T, N_SIG_IN)
    sp = np.pad(sig, ((0, 0), (0, 0), (1, 1)))
    z1 = b1 + sum(sp[..., k:k + N_SIG_IN, None] * w1[k] for k in range(3))
    a1 = np.maximum(z1, 0)
    c1 = a1 * s1 + h1
    cp = np.pad(c1, ((0, 0), (0, 0), (1, 1), (0, 0)))
    z2 = b2 + sum(cp[..., k:k + N_SIG_IN, :] @ w2[k] for k in range(3))
    a2 = np.maximum(z2, 0)
    F = dropout.apply((a2 * s2 + h2 + sig[..., None]).reshape(-1, T, N_FLAT), drop, dt)
    return {"sig": sig, "z1": z1, "a1": a1, "c1": c1, "z2": z2, "a2": a2, "F": F, "S": F @ Ws + bs}


def xin(x2, S, T: int, dtype=np.float64):
    """[x2 | S] [n][T][192], the model's concatenate."""
    dt = np.dtype(dtype)
    return np.concatenate([np.asarray(x2).astype(dt).reshape(-1, T, 128), np.asarray(S).astype(dt)], axis=2)


def forward(x2, sig, theta, cb, sc, sh, T: int, C: int, act: int = 0, dtype=np.float64):
    """-> (S [n][T][64],) + lstm3fit.forward's (H3, Xb4, X4, mo, f, p)."""
    S = branch(sig, theta, cb, T, C, dtype)["S"]
    return (S,) + lstm3fit.forward(xin(x2, S, T, dtype), np.asarray(theta)[N_SIGNAL:], sc, sh, T, C, act, dtype)


def batch_terms(x2, sig, y, theta, cb, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64, drop=None):
    """One batch -> (g [P]: the gradient of L, FitStats of the batch with steps = nonfinite = 0).  ReLU sides are decided on the
    forward value; every gradient is divided by n as the LSTM blocks' are.  drop: dropout.terms of the batch's set rows."""
    return batch_terms_dx(x2, sig, y, theta, cb, sc, sh, T, C, opts, act, dtype, drop=drop)[:2]


def batch_terms_dx(x2, sig, y, theta, cb, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64, taps=None,
                   drop=None):
    """batch_terms and the data gradient behind it -> (g, FitStats, dx2 [n][T][128]: columns 0 .. 127 of lstm3fit's dXin - the
    derivative of the batch's SUM of row losses by x2, not divided by n).  fullfit.py goes on from it.  taps: a dict that
    receives lstm3fit's "bn_l3" and "bn_c2": (dF [n][T][50][8], a2), "bn_c1": (dc1, a1) - what bnaffine.py sums; nothing returned
    depends on it.  drop = (mask, keepf): F and dF go through the dropout (the statistics are the dropped forward's)."""
    dt = np.dtype(dtype)
    theta = np.asarray(theta)
    k = branch(sig, theta, cb, T, C, dt, drop)
    n = k["sig"].shape[0]
    g3, st, dXin = lstm3fit.batch_terms_dx(xin(x2, k["S"], T, dt), y, theta[N_SIGNAL:], sc, sh, T, C, opts, act, dt, taps)
    w1, b1, w2, b2, Ws, bs = [a.astype(dt) for a in unpack(theta, T, C)[:6]]
    s1, s2 = np.asarray(cb[0]).astype(dt), np.asarray(cb[2]).astype(dt)
    dS = dXin[..., 128:]
    gWs = k["F"].reshape(-1, N_FLAT).T @ dS.reshape(-1, N_S)
    gbs = dS.reshape(-1, N_S).sum(axis=0)
    dF = dropout.apply(dS @ Ws.T, drop, dt).reshape(n, T, N_SIG_IN, N_CH)
    da2 = np.where(k["a2"] > 0, dF * s2, dt.type(0))
    cp = np.pad(k["c1"], ((0, 0), (0, 0), (1, 1), (0, 0)))
    dp = np.pad(da2, ((0, 0), (0, 0), (1, 1), (0, 0)))     # dp[q] = da2[q - 1]
    gw2 = np.stack([np.einsum("ntpc,ntpo->co", cp[..., kk:kk + N_SIG_IN, :], da2) for kk in range(3)])
    gb2 = da2.sum(axis=(0, 1, 2))
    dc1 = sum(dp[..., 2 - kk:2 - kk + N_SIG_IN, :] @ w2[kk].T for kk in range(3))      # da2[p - kk + 1]
    if taps is not None:
        taps["bn_c2"], taps["bn_c1"] = (dF, k["a2"]), (dc1, k["a1"])
    da1 = np.where(k["a1"] > 0, dc1 * s1, dt.type(0))
    sp = np.pad(k["sig"], ((0, 0), (0, 0), (1, 1)))
    gw1 = np.stack([np.einsum("ntp,ntpo->o", sp[..., kk:kk + N_SIG_IN], da1) for kk in range(3)])
    gb1 = da1.sum(axis=(0, 1, 2))
    g = np.concatenate([a.ravel() for a in (gw1, gb1, gw2, gb2, gWs, gbs)]) / dt.type(n)
    return np.concatenate([g.astype(dt), g3]), st, dXin[..., :128]


def epoch(x2, sig, y, state: FitState, order, cb, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0,
          dtype=np.float64, drop=None) -> FitStats:
    """tailfit.epoch's rule on signal rows: consecutive batches of opts.B in the order of `order`, a batch with a non-finite
    gradient skipped and counted, statistics before each update.  drop: a dropout.Stream - batch k of the call drops at draw + k
    on its set rows, and the stream advances by the number of batches, skipped ones included."""
    dt = np.dtype(dtype)
    order = np.asarray(order, np.int64).reshape(-1)
    x2, sig, y = np.asarray(x2).reshape(-1, T, 128), np.asarray(sig).reshape(-1, T, N_SIG_IN), np.asarray(y)
    tot = FitStats()
    for s in range(0, order.size, opts.B):
        idx = order[s:s + opts.B]
        with np.errstate(all="ignore"):
            g, st = batch_terms(x2[idx], sig[idx], y[idx], state.theta, cb, sc, sh, T, C, opts, act, dt,
                                None if drop is None else drop.batch(s // opts.B, idx, T))
        if not np.isfinite(g).all():
            tot.nonfinite += 1
            continue
        state.t += 1
        state.theta, state.m, state.v = adam_step(state.theta, state.m, state.v, g, opts, state.t, dt)
        st.steps = 1
        tot.add(st)
    if drop is not None:
        drop.advance(-(-order.size // opts.B))
    return tot


def evaluate(x2, sig, y, theta, order, cb, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64):
    """-> (p [n][C], FitStats): forward only."""
    order = np.asarray(order, np.int64).reshape(-1)
    x2, sig = np.asarray(x2).reshape(-1, T, 128)[order], np.asarray(sig).reshape(-1, T, N_SIG_IN)[order]
    y = np.asarray(y)[order]
    with np.errstate(all="ignore"):
        out = forward(x2, sig, theta, cb, sc, sh, T, C, act, dtype)
        X4, p = out[3], out[6]
        st = FitStats()
        if order.size:
            st = headfit.batch_terms(X4, y, np.asarray(theta)[N_SIGNAL + lstm3fit.N_LSTM3 + lstm4fit.N_LSTM4:], T, C, opts,
                                     dtype)[1]
        return p, st


def fitted_model(m, theta, T: Optional[int] = None):
    """The model with tensors 0, 1, 6, 7, 32 .. 39 and 44 .. 59 replaced by theta's; every other tensor (the BatchNorms 2 .. 5,
    8 .. 11 and 40 .. 43, lstm1 and lstm2 with theirs) keeps its bytes."""
    from .weights import ModelWeights
    T = m.T if T is None else T
    theta = np.asarray(theta, np.float32)
    m3 = lstm3fit.fitted_model(m, theta[N_SIGNAL:], T)
    ts = list(m3.tensors)
    for i, a in zip(_TENSOR_IDS, unpack(theta, T, m.n_class)[:6]):
        ts[i] = a.astype(np.float32).reshape(np.asarray(m.tensors[i]).shape).copy()
    return ModelWeights(ts, T, m.n_class, m.source + "+signalfit")
