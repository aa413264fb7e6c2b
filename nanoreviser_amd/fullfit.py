"""Fitting the read branch too - the whole model: the DEFINITION of what the engine's nrv_fit_* entry points compute at depth
NRV_FIT_FULL (include/nanorev.h, csrc/nrv_fullfit.h).  NumPy only.

Fitted are lstm1 - the 6 -> 16 Bi-LSTM on the read features, tensors 12 .. 17: W [6][64], U [16][64], b [64] per direction - and
lstm2 - the 32 -> 64 Bi-LSTM behind it, tensors 22 .. 27: W [32][256], U [64][256], b [256] - forward direction first, gate
columns in Keras order i, f, c, o, and everything signalfit.py fits (tensors 0, 1, 6, 7, 32 .. 39, 44 .. 59 and the centres):
every tensor of the 60 that is no BatchNorm's.  A window IS its raw inputs, the pair (feat [T][6], sig [T][50]) nrv_predict*
takes.  One vector per model,
  [W1f | U1f | b1f | W1b | U1b | b1b | W2f | U2f | b2f | W2b | U2b | b2b | signalfit's vector]
                                                                              n_params(T, C) = 52608 + signalfit.n_params(T, C).

THE STATED DEVIATIONS are signalfit's, with two more BatchNorms under the first: bn_l1 (tensors 18 .. 21) and bn_l2 (28 .. 31)
are FROZEN and applied in their inference form from the moving statistics, X1b = h1 * s_l1 + h_l1 and X2b = h2 * s_l2 + h_l2 - one
multiply and one add, (s_l1, h_l1, s_l2, h_l2) - `rb` - as read_bn forms them.  The written model's BatchNorm tensors are the
loaded ones, byte for byte.  Dropout is not applied - a deviation that holds only while the switch is off: with
`drop = (mask, keepf)` (dropout.py; nrv_fit_set_dropout on the device) batch_terms and epoch drop F as signalfit does.

Forward: lstm1 and lstm2 by lstm3fit's step rule with H = 16 and H = 64 (the backward direction walks t = T - 1 .. 0), then
Xin = [X2b | S] and signalfit's forward.  Backward: signalfit's, whose batch_terms_dx also returns dXin[..., :128];
dH2 = dXin[..., :128] * s_l2 and back through time in lstm2; dX1b = sum over the directions (forward first) of dz2 W2^T,
dH1 = dX1b * s_l1 and back through time in lstm1.  gW = sum x_t^T dz, gU = sum h_{s-1}^T dz (raw h; zero at T = 1), gb = sum dz,
everything divided by n.  Everything behind Xin IS signalfit's: loss, options, Adam step, epoch order and files are used, not
restated.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import headfit, lstm3fit, lstm4fit, signalfit, tailfit  # noqa: F401
from .lstm4fit import BN_EPS, _act, _act_d
from .tailfit import (FitOpts, FitState, FitStats, adam_step, default_opts, epoch_order, lr_t, val_split,  # noqa: F401
                      write_f32)

N_FEAT, N_SIG_IN = 6, 50
_LAYERS = ((6, 16), (32, 64))                                  # (inputs, units) of lstm1, lstm2
_SHAPES = tuple(s for d, h in _LAYERS for _ in range(2) for s in ((d, 4 * h), (h, 4 * h), (4 * h,)))
N_LSTM1 = 2 * (6 * 64 + 16 * 64 + 64)                          # 2944
N_LSTM2 = 2 * (32 * 256 + 64 * 256 + 256)                      # 49664
N_READ = N_LSTM1 + N_LSTM2                                     # 52608
_TENSOR_IDS = tuple(range(12, 18)) + tuple(range(22, 28))


def n_params(T: int, C: int) -> int:
    """NRV_FIT_PARAMS_FULL(T, C)."""
    return N_READ + signalfit.n_params(T, C)


def pack(*parts, dtype=np.float32) -> np.ndarray:
    """The twelve read-branch tensors, then signalfit.pack's twenty-nine."""
    return np.concatenate([np.asarray(a, dtype).ravel() for a in parts[:12]] + [signalfit.pack(*parts[12:], dtype=dtype)])


def unpack(theta, T: int, C: int):
    """-> [W1f, U1f, b1f, W1b, U1b, b1b, W2f, U2f, b2f, W2b, U2b, b2b] + signalfit.unpack's list (views)."""
    theta = np.asarray(theta)
    if theta.size != n_params(T, C):
        raise ValueError(f"parameter vector of {theta.size} floats, expected {n_params(T, C)} for T={T}, C={C} at full depth")
    out, at = [], 0
    for s in _SHAPES:
        n = int(np.prod(s))
        out.append(theta[at:at + n].reshape(s))
        at += n
    return out + signalfit.unpack(theta[at:], T, C)


def params_from_model(m, dtype=np.float32) -> np.ndarray:
    """A model's own non-BatchNorm tensors with zero centres: what nrv_fit_begin(params = NULL) starts from at full depth."""
    t = m.tensors
    return np.concatenate([np.asarray(t[i], dtype).ravel() for i in _TENSOR_IDS] + [signalfit.params_from_model(m, dtype)])


def with_signal(theta, theta_signal) -> np.ndarray:
    """theta with everything behind the read branch replaced by a vector of signalfit's layout."""
    out = np.array(theta, np.float32)
    out[N_READ:] = np.asarray(theta_signal, np.float32)
    return out


def read_bn(m):
    """(s_l1, h_l1 f32 [32], s_l2, h_l2 f32 [128]): the two frozen BatchNorms of the read branch (tensors 18 .. 21 and 28 .. 31)
    as the engine's bn_fold forms them."""
    out = []
    for base in (18, 28):
        g, be, mu, var = [np.asarray(m.tensors[base + i], np.float32) for i in range(4)]
        s = (g / np.sqrt(var + np.float32(BN_EPS))).astype(np.float32)
        out += [s, (be - mu * s).astype(np.float32)]
    return tuple(out)


# ---- forward, loss, gradient ---------------------------------------------------------------------------------------------
def _bilstm(X, parts, H: int, T: int, act: int, dt):
    """lstm3fit.lstm's step rule for any width -> (Hr [n][T][2H]: the RAW output [h_fw | h_bw] in input time order, per
    direction a dict of i f g o c [n][T][H] in STEP order and z [n][T][4H])."""
    n = X.shape[0]
    Hr = np.zeros((n, T, 2 * H), dt)
    keep = []
    for d in range(2):
        W, U, b = parts[3 * d:3 * d + 3]
        h, c = np.zeros((n, H), dt), np.zeros((n, H), dt)
        k = {q: np.zeros((n, T, H), dt) for q in "ifgoc"}
        k["z"] = np.zeros((n, T, 4 * H), dt)
        for s in range(T):
            t = T - 1 - s if d else s
            z = X[:, t] @ W + h @ U + b
            i, f, o = _act(z[:, :H], act), _act(z[:, H:2 * H], act), _act(z[:, 3 * H:], act)
            g = np.tanh(z[:, 2 * H:3 * H])
            c = f * c + i * g
            h = o * np.tanh(c)
            Hr[:, t, d * H:(d + 1) * H] = h
            for q, v in zip("ifgocz", (i, f, g, o, c, z)):
                k[q][:, s] = v
        keep.append(k)
    return Hr, keep


def _bilstm_back(X, Hr, keep, dH, parts, H: int, T: int, act: int, dt, want_dx: bool):
    """Back through time, lstm3fit.batch_terms_dx's rule for any width: dH [n][T][2H] is the derivative of the batch's SUM of row
    losses by the raw output -> ([gW, gU, gb] x 2 as sums, dX [n][T][D] or None)."""
    n, D = X.shape[0], X.shape[2]
    one = dt.type(1)
    grads = []
    dX = np.zeros((n, T, D), dt) if want_dx else None
    for d in range(2):
        W, U = parts[3 * d], parts[3 * d + 1]
        k = keep[d]
        gW, gU, gb = np.zeros((D, 4 * H), dt), np.zeros((H, 4 * H), dt), np.zeros(4 * H, dt)
        dz_next = np.zeros((n, 4 * H), dt)
        dcf = np.zeros((n, H), dt)
        for s in range(T - 1, -1, -1):
            t = T - 1 - s if d else s
            i, f, g, o, c = (k[q][:, s] for q in "ifgoc")
            c_prev = k["c"][:, s - 1] if s > 0 else np.zeros((n, H), dt)
            h_prev = Hr[:, (t + 1 if d else t - 1), d * H:(d + 1) * H] if s > 0 else np.zeros((n, H), dt)
            dh = dH[:, t, d * H:(d + 1) * H] + dz_next @ U.T
            tc = np.tanh(c)
            do = dh * tc
            dc = dh * o * (one - tc * tc) + dcf
            dz = np.concatenate([dc * g * _act_d(i, act), dc * c_prev * _act_d(f, act), dc * i * (one - g * g),
                                 do * _act_d(o, act)], axis=1)
            gW += X[:, t].T @ dz
            gU += h_prev.T @ dz
            gb += dz.sum(axis=0)
            if want_dx:
                dX[:, t] += dz @ W.T
            dcf = dc * f
            dz_next = dz
        grads += [gW, gU, gb]
    return grads, dX


def read_branch(feat, theta, rb, T: int, C: int, act: int = 0, dtype=np.float64):
    """-> dict(feat [n][T][6], H1 [n][T][32] and H2 [n][T][128] raw, X1b, X2b behind their BatchNorms, k1 / k2: the kept gates of
    _bilstm)."""
    dt = np.dtype(dtype)
    parts = [a.astype(dt) for a in unpack(theta, T, C)[:12]]
    s1, h1, s2, h2 = [np.asarray(a).astype(dt) for a in rb]
    feat = np.asarray(feat).astype(dt).reshape(-1, T, N_FEAT)
    H1, k1 = _bilstm(feat, parts[:6], 16, T, act, dt)
    X1b = (H1 * s1).astype(dt) + h1
    H2, k2 = _bilstm(X1b, parts[6:], 64, T, act, dt)
    X2b = (H2 * s2).astype(dt) + h2
    return {"feat": feat, "H1": H1, "X1b": X1b, "H2": H2, "X2b": X2b, "k1": k1, "k2": k2}


def forward(feat, sig, theta, rb, cb, sc, sh, T: int, C: int, act: int = 0, dtype=np.float64):
    """-> (X2b [n][T][128],) + signalfit.forward's (S, H3, Xb4, X4, mo, f, p)."""
    X2b = read_branch(feat, theta, rb, T, C, act, dtype)["X2b"]
    return (X2b,) + signalfit.forward(X2b, sig, np.asarray(theta)[N_READ:], cb, sc, sh, T, C, act, dtype)


def batch_terms(feat, sig, y, theta, rb, cb, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64, taps=None,
                drop=None):
    """One batch -> (g [P]: the gradient of L, FitStats of the batch with steps = nonfinite = 0).  Gate derivatives are decided
    on the forward value; every gradient is divided by n.  taps: a dict that receives signalfit's three pairs and "bn_l2":
    (dx2, the raw H2), "bn_l1": (dX1b, the raw H1) - what bnaffine.py sums; nothing returned depends on it.  drop: dropout.terms of
    the batch's set rows, handed to signalfit."""
    dt = np.dtype(dtype)
    theta = np.asarray(theta)
    k = read_branch(feat, theta, rb, T, C, act, dt)
    n = k["feat"].shape[0]
    gs, st, dx2 = signalfit.batch_terms_dx(k["X2b"], sig, y, theta[N_READ:], cb, sc, sh, T, C, opts, act, dt, taps, drop)
    parts = [a.astype(dt) for a in unpack(theta, T, C)[:12]]
    s1, s2 = np.asarray(rb[0]).astype(dt), np.asarray(rb[2]).astype(dt)
    g2, dX1b = _bilstm_back(k["X1b"], k["H2"], k["k2"], dx2 * s2, parts[6:], 64, T, act, dt, True)
    if taps is not None:
        taps["bn_l2"], taps["bn_l1"] = (dx2, k["H2"]), (dX1b, k["H1"])
    g1, _ = _bilstm_back(k["feat"], k["H1"], k["k1"], dX1b * s1, parts[:6], 16, T, act, dt, False)
    g = np.concatenate([a.ravel() for a in g1 + g2]) / dt.type(n)
    return np.concatenate([g.astype(dt), gs]), st


def epoch(feat, sig, y, state: FitState, order, rb, cb, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0,
          dtype=np.float64, drop=None) -> FitStats:
    """tailfit.epoch's rule on raw windows: consecutive batches of opts.B in the order of `order`, a batch with a non-finite
    gradient skipped and counted, statistics before each update.  drop: a dropout.Stream, as signalfit.epoch takes it."""
    dt = np.dtype(dtype)
    order = np.asarray(order, np.int64).reshape(-1)
    feat, sig, y = np.asarray(feat).reshape(-1, T, N_FEAT), np.asarray(sig).reshape(-1, T, N_SIG_IN), np.asarray(y)
    tot = FitStats()
    for s in range(0, order.size, opts.B):
        idx = order[s:s + opts.B]
        with np.errstate(all="ignore"):
            g, st = batch_terms(feat[idx], sig[idx], y[idx], state.theta, rb, cb, sc, sh, T, C, opts, act, dt,
                                drop=None if drop is None else drop.batch(s // opts.B, idx, T))
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


def evaluate(feat, sig, y, theta, order, rb, cb, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64):
    """-> (p [n][C], FitStats): forward only."""
    order = np.asarray(order, np.int64).reshape(-1)
    feat, sig = np.asarray(feat).reshape(-1, T, N_FEAT)[order], np.asarray(sig).reshape(-1, T, N_SIG_IN)[order]
    y = np.asarray(y)[order]
    with np.errstate(all="ignore"):
        out = forward(feat, sig, theta, rb, cb, sc, sh, T, C, act, dtype)
        X4, p = out[4], out[7]
        st = FitStats()
        if order.size:
            at = N_READ + signalfit.N_SIGNAL + lstm3fit.N_LSTM3 + lstm4fit.N_LSTM4
            st = headfit.batch_terms(X4, y, np.asarray(theta)[at:], T, C, opts, dtype)[1]
        return p, st


def fitted_model(m, theta, T: Optional[int] = None):
    """The model with its forty non-BatchNorm tensors replaced by theta's; the twenty BatchNorm tensors (2 .. 5, 8 .. 11,
    18 .. 21, 28 .. 31 and 40 .. 43) keep their bytes."""
    from .weights import ModelWeights
    T = m.T if T is None else T
    theta = np.asarray(theta, np.float32)
    ms = signalfit.fitted_model(m, theta[N_READ:], T)
    ts = list(ms.tensors)
    for i, a in zip(_TENSOR_IDS, unpack(theta, T, m.n_class)[:12]):
        ts[i] = a.astype(np.float32).reshape(np.asarray(m.tensors[i]).shape).copy()
    return ModelWeights(ts, T, m.n_class, m.source + "+fullfit")
