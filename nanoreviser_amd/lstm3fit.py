"""Fitting the 192 -> 128 Bi-LSTM with everything behind it: the DEFINITION of what the engine's nrv_fit_* entry points compute
at depth NRV_FIT_LSTM3 (include/nanorev.h, csrc/nrv_lstm3fit.h).  NumPy only.

Fitted are lstm3 - the 192 -> 128 Bi-LSTM where the read branch and the signal branch meet, tensors 34 .. 39: W [192][512],
U [128][512], b [512] per direction, forward first, gate columns in Keras order i, f, c, o - and everything lstm4fit.py fits
(tensors 44 .. 59 and the centres).  Tensors 0 .. 33 are frozen, so a window IS Xin [T][192]: the BatchNorm'd f32 lstm2 output
(128 values), then signal_x_out (64 values), in the order of the model's concatenate.  One parameter vector per model,
  [W3f | U3f | b3f | W3b | U3b | b3b | lstm4fit's vector]         n_params(T, C) = 328704 + lstm4fit.n_params(T, C) floats.

A STATED DEVIATION.  The BatchNorm between lstm3 and lstm4 (tensors 40 .. 43) lies inside the fitted section.  It is FROZEN and
applied in its inference form, Xb4 = h3 * sc + sh - one multiply and one add, sc and sh as lstm4fit.bn_scale_shift forms them
from the moving statistics.  Keras in training phase would normalise with the batch's statistics and would fit gamma and beta;
this depth fine-tunes with the moving statistics fixed.  sc and sh are arguments of every numeric function here.

Everything behind Xb4 IS lstm4fit's (then headfit's and tailfit's): forward, loss, options, Adam step, epoch order and files
are used, not restated.  `act` and `dtype` are as in lstm4fit.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import headfit, lstm4fit, tailfit  # noqa: F401
from .lstm4fit import _act, _act_d, bn_scale_shift  # noqa: F401
from .tailfit import (FitOpts, FitState, FitStats, adam_step, default_opts, epoch_order, lr_t, val_split,  # noqa: F401
                      write_f32)

D_X, H = 192, 128
N_DIR = D_X * 4 * H + H * 4 * H + 4 * H                        # 164352
N_LSTM3 = 2 * N_DIR                                            # 328704
_DIR_SHAPES = ((D_X, 4 * H), (H, 4 * H), (4 * H,))


def n_params(T: int, C: int) -> int:
    """NRV_FIT_PARAMS_LSTM3(T, C)."""
    return N_LSTM3 + lstm4fit.n_params(T, C)


def pack(Wf, Uf, bf, Wb, Ub, bb, *rest, dtype=np.float32) -> np.ndarray:
    """The six lstm3 tensors, then lstm4fit.pack's seventeen."""
    return np.concatenate([np.asarray(a, dtype).ravel() for a in (Wf, Uf, bf, Wb, Ub, bb)] + [lstm4fit.pack(*rest, dtype=dtype)])


def unpack(theta, T: int, C: int):
    """-> [W3f, U3f, b3f, W3b, U3b, b3b, W4f, U4f, b4f, W4b, U4b, b4b, W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce] (views)."""
    theta = np.asarray(theta)
    if theta.size != n_params(T, C):
        raise ValueError(f"parameter vector of {theta.size} floats, expected {n_params(T, C)} for T={T}, C={C} at lstm3 depth")
    out, at = [], 0
    for _ in range(2):
        for s in _DIR_SHAPES:
            n = int(np.prod(s))
            out.append(theta[at:at + n].reshape(s))
            at += n
    return out + lstm4fit.unpack(theta[at:], T, C)


def params_from_model(m, dtype=np.float32) -> np.ndarray:
    """A model's own tensors 34 .. 39 and 44 .. 59 with zero centres: what nrv_fit_begin(params = NULL) starts from at lstm3
    depth."""
    t = m.tensors
    return np.concatenate([np.asarray(t[i], dtype).ravel() for i in range(34, 40)] + [lstm4fit.params_from_model(m, dtype)])


def with_lstm4(theta, theta_lstm4) -> np.ndarray:
    """theta with everything behind lstm3 replaced by a vector of lstm4fit's layout."""
    out = np.array(theta, np.float32)
    out[N_LSTM3:] = np.asarray(theta_lstm4, np.float32)
    return out


# ---- forward, loss, gradient ---------------------------------------------------------------------------------------------
def lstm(Xin, theta, T: int, C: int, act: int = 0, dtype=np.float64):
    """-> (Xin [n][T][192], H3 [n][T][256]: the RAW lstm3 output [h_fw | h_bw] in input time order, per direction a dict of
    i f g o c [n][T][128] in STEP order and z [n][T][512])."""
    dt = np.dtype(dtype)
    parts = [a.astype(dt) for a in unpack(theta, T, C)[:6]]
    Xin = np.asarray(Xin).astype(dt).reshape(-1, T, D_X)
    n = Xin.shape[0]
    H3 = np.zeros((n, T, 2 * H), dt)
    keep = []
    for d in range(2):
        W, U, b = parts[3 * d:3 * d + 3]
        h, c = np.zeros((n, H), dt), np.zeros((n, H), dt)
        k = {q: np.zeros((n, T, H), dt) for q in "ifgoc"}
        k["z"] = np.zeros((n, T, 4 * H), dt)
        for s in range(T):
            t = T - 1 - s if d else s
            z = Xin[:, t] @ W + h @ U + b
            i, f, o = _act(z[:, :H], act), _act(z[:, H:2 * H], act), _act(z[:, 3 * H:], act)
            g = np.tanh(z[:, 2 * H:3 * H])
            c = f * c + i * g
            h = o * np.tanh(c)
            H3[:, t, d * H:(d + 1) * H] = h
            for q, v in zip("ifgocz", (i, f, g, o, c, z)):
                k[q][:, s] = v
        keep.append(k)
    return Xin, H3, keep


def bn(H3, sc, sh, dtype=np.float64):
    """Xb4 = h3 * sc + sh in `dtype`: one multiply and one add (the frozen BatchNorm in its inference form)."""
    dt = np.dtype(dtype)
    return (np.asarray(H3).astype(dt) * np.asarray(sc).astype(dt)).astype(dt) + np.asarray(sh).astype(dt)


def forward(Xin, theta, sc, sh, T: int, C: int, act: int = 0, dtype=np.float64):
    """-> (H3 [n][T][256], Xb4 [n][T][256], X4 [n][T][128], mo [n][T][6], f [n][16], p [n][C])."""
    H3 = lstm(Xin, theta, T, C, act, dtype)[1]
    Xb4 = bn(H3, sc, sh, dtype)
    return (H3, Xb4) + lstm4fit.forward(Xb4, np.asarray(theta)[N_LSTM3:], T, C, act, dtype)


def batch_terms(Xin, y, theta, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64):
    """One batch -> (g [P]: the gradient of L, FitStats of the batch with steps = nonfinite = 0)."""
    return batch_terms_dx(Xin, y, theta, sc, sh, T, C, opts, act, dtype)[:2]


def batch_terms_dx(Xin, y, theta, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64, taps=None):
    """batch_terms and the data gradient behind it -> (g, FitStats, dXin [n][T][192]: the sum over both directions (forward
    first) and all steps of dz3 W3^T - the derivative of the batch's SUM of row losses, not divided by n).  signalfit.py goes on
    from its columns 128 .. 191.  taps: a dict that receives "bn_l3": (dXb4, the raw H3) - what bnaffine.py sums; nothing
    returned depends on it."""
    dt = np.dtype(dtype)
    theta = np.asarray(theta)
    Xin, H3, keep = lstm(Xin, theta, T, C, act, dt)
    n = Xin.shape[0]
    g4, st, dXb4 = lstm4fit.batch_terms_dx(bn(H3, sc, sh, dt), y, theta[N_LSTM3:], T, C, opts, act, dt)
    if taps is not None:
        taps["bn_l3"] = (dXb4, H3)
    dX3 = dXb4 * np.asarray(sc).astype(dt)
    parts = [a.astype(dt) for a in unpack(theta, T, C)[:6]]
    one = dt.type(1)
    grads = []
    dXin = np.zeros((n, T, D_X), dt)
    for d in range(2):
        W, U = parts[3 * d], parts[3 * d + 1]
        k = keep[d]
        gW, gU, gb = np.zeros((D_X, 4 * H), dt), np.zeros((H, 4 * H), dt), np.zeros(4 * H, dt)
        dz_next = np.zeros((n, 4 * H), dt)
        dcf = np.zeros((n, H), dt)                         # dc_{s+1} f_{s+1}
        for s in range(T - 1, -1, -1):
            t = T - 1 - s if d else s
            i, f, g, o, c = (k[q][:, s] for q in "ifgoc")
            c_prev = k["c"][:, s - 1] if s > 0 else np.zeros((n, H), dt)
            h_prev = H3[:, (t + 1 if d else t - 1), d * H:(d + 1) * H] if s > 0 else np.zeros((n, H), dt)
            dh = dX3[:, t, d * H:(d + 1) * H] + dz_next @ U.T
            tc = np.tanh(c)
            do = dh * tc
            dc = dh * o * (one - tc * tc) + dcf
            dz = np.concatenate([dc * g * _act_d(i, act), dc * c_prev * _act_d(f, act), dc * i * (one - g * g),
                                 do * _act_d(o, act)], axis=1)
            gW += Xin[:, t].T @ dz
            gU += h_prev.T @ dz
            gb += dz.sum(axis=0)
            dXin[:, t] += dz @ W.T
            dcf = dc * f
            dz_next = dz
        grads += [gW, gU, gb]
    g = np.concatenate([a.ravel() for a in grads]) / dt.type(n)
    return np.concatenate([g.astype(dt), g4]), st, dXin


def epoch(Xin, y, state: FitState, order, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64) -> FitStats:
    """tailfit.epoch's rule on lstm3 rows: consecutive batches of opts.B in the order of `order`, a batch with a non-finite
    gradient skipped and counted, statistics before each update."""
    dt = np.dtype(dtype)
    order = np.asarray(order, np.int64).reshape(-1)
    Xin, y = np.asarray(Xin).reshape(-1, T, D_X), np.asarray(y)
    tot = FitStats()
    for s in range(0, order.size, opts.B):
        idx = order[s:s + opts.B]
        with np.errstate(all="ignore"):
            g, st = batch_terms(Xin[idx], y[idx], state.theta, sc, sh, T, C, opts, act, dt)
        if not np.isfinite(g).all():
            tot.nonfinite += 1
            continue
        state.t += 1
        state.theta, state.m, state.v = adam_step(state.theta, state.m, state.v, g, opts, state.t, dt)
        st.steps = 1
        tot.add(st)
    return tot


def evaluate(Xin, y, theta, order, sc, sh, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64):
    """-> (p [n][C], FitStats): forward only."""
    order = np.asarray(order, np.int64).reshape(-1)
    Xin, y = np.asarray(Xin).reshape(-1, T, D_X)[order], np.asarray(y)[order]
    with np.errstate(all="ignore"):
        out = forward(Xin, theta, sc, sh, T, C, act, dtype)
        X4, p = out[2], out[5]
        st = FitStats()
        if order.size:
            st = headfit.batch_terms(X4, y, np.asarray(theta)[N_LSTM3 + lstm4fit.N_LSTM4:], T, C, opts, dtype)[1]
        return p, st


def fitted_model(m, theta, T: Optional[int] = None):
    """The model with tensors 34 .. 39 and 44 .. 59 replaced by theta's (0 .. 33 and the BatchNorm 40 .. 43 unchanged)."""
    from .weights import ModelWeights
    T = m.T if T is None else T
    parts = unpack(np.asarray(theta, np.float32), T, m.n_class)[:22]
    new = [a.astype(np.float32).copy() for a in parts]
    ts = list(m.tensors[:34]) + new[:6] + list(m.tensors[40:44]) + new[6:]
    return ModelWeights(ts, T, m.n_class, m.source + "+lstm3fit")
