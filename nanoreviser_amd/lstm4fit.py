"""Fitting the last Bi-LSTM with the head: the DEFINITION of what the engine's nrv_fit_* entry points compute at depth
NRV_FIT_LSTM4 (include/nanorev.h, csrc/nrv_lstm4fit.h).  NumPy only.

Fitted are lstm4 - the 256 -> 64 Bi-LSTM, tensors 44 .. 49: W [256][256], U [64][256], b [256] per direction, forward first,
gate columns in Keras order i, f, c, o - and everything headfit.py fits (tensors 50 .. 59 and the centres).  The 44 tensors in
front are frozen, so a window IS Xb [T][256]: the BatchNorm (tensors 40 .. 43) of its f32 lstm3 output, in input time order.
One parameter vector per model,
  [W4f | U4f | b4f | W4b | U4b | b4b | headfit's vector]          n_params(T, C) = 164352 + headfit.n_params(T, C) floats.
Everything behind X4 = [h_fw | h_bw] IS headfit's (and behind main_out, tailfit's): forward, loss, options, Adam step, epoch
order and files are used, not restated.

`act` is the handle's recurrent_act: 0 hard_sigmoid = clip(0.2 z + 0.5, 0, 1), 1 sigmoid.  Every function takes `dtype` as in
tailfit: float64 is the definition, float32 a restatement in the engine's number format.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import headfit, tailfit
from .tailfit import (FitOpts, FitState, FitStats, adam_step, default_opts, epoch_order, lr_t, val_split,  # noqa: F401
                      write_f32)

D_X, H = 256, 64
N_DIR = D_X * 4 * H + H * 4 * H + 4 * H                        # 82176
N_LSTM4 = 2 * N_DIR                                            # 164352
_DIR_SHAPES = ((D_X, 4 * H), (H, 4 * H), (4 * H,))
BN_EPS = 1e-3


def n_params(T: int, C: int) -> int:
    """NRV_FIT_PARAMS_LSTM4(T, C)."""
    return N_LSTM4 + headfit.n_params(T, C)


def pack(Wf, Uf, bf, Wb, Ub, bb, *head, dtype=np.float32) -> np.ndarray:
    """The six LSTM tensors, then headfit.pack's eleven."""
    return np.concatenate([np.asarray(a, dtype).ravel() for a in (Wf, Uf, bf, Wb, Ub, bb)] + [headfit.pack(*head, dtype=dtype)])


def unpack(theta, T: int, C: int):
    """-> [W4f, U4f, b4f, W4b, U4b, b4b, W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce] (views)."""
    theta = np.asarray(theta)
    if theta.size != n_params(T, C):
        raise ValueError(f"parameter vector of {theta.size} floats, expected {n_params(T, C)} for T={T}, C={C} at lstm4 depth")
    out, at = [], 0
    for _ in range(2):
        for s in _DIR_SHAPES:
            n = int(np.prod(s))
            out.append(theta[at:at + n].reshape(s))
            at += n
    return out + headfit.unpack(theta[at:], T, C)


def params_from_model(m, dtype=np.float32) -> np.ndarray:
    """A model's own tensors 44 .. 59 with zero centres: what nrv_fit_begin(params = NULL) starts from at lstm4 depth."""
    t = m.tensors
    return np.concatenate([np.asarray(t[i], dtype).ravel() for i in range(44, 50)] + [headfit.params_from_model(m, dtype)])


def with_head(theta, theta_head) -> np.ndarray:
    """theta with everything behind lstm4 replaced by a vector of headfit's layout."""
    out = np.array(theta, np.float32)
    out[N_LSTM4:] = np.asarray(theta_head, np.float32)
    return out


def bn_scale_shift(m):
    """(sc, sh) f32 [256] of the BatchNorm in front of lstm4, as the engine's bn_fold forms them."""
    g, be, mu, var = [np.asarray(m.tensors[i], np.float32) for i in range(40, 44)]
    sc = (g / np.sqrt(var + np.float32(BN_EPS))).astype(np.float32)
    sh = (be - mu * sc).astype(np.float32)
    return sc, sh


def xb_from_lstm3(x3, m) -> np.ndarray:
    """A row of the set from an lstm3 output [.][T][256] (f32): x * sc + sh, one multiply and one add."""
    sc, sh = bn_scale_shift(m)
    x = np.asarray(x3, np.float32)
    return ((x * sc).astype(np.float32) + sh).astype(np.float32)


# ---- forward, loss, gradient ---------------------------------------------------------------------------------------------
def _act(z, act: int):
    if act == 0:
        return np.clip(z.dtype.type(0.2) * z + z.dtype.type(0.5), 0, 1)
    return 1 / (1 + np.exp(-z))


def _act_d(a, act: int):
    """act' decided on the forward VALUE."""
    if act == 0:
        return np.where((a > 0) & (a < 1), a.dtype.type(0.2), a.dtype.type(0))
    return a * (1 - a)


def lstm(Xb, theta, T: int, C: int, act: int = 0, dtype=np.float64):
    """-> (Xb [n][T][256], X4 [n][T][128], per direction a dict of i f g o c [n][T][64] in STEP order and z [n][T][256])."""
    dt = np.dtype(dtype)
    parts = [a.astype(dt) for a in unpack(theta, T, C)[:6]]
    Xb = np.asarray(Xb).astype(dt).reshape(-1, T, D_X)
    n = Xb.shape[0]
    X4 = np.zeros((n, T, 2 * H), dt)
    keep = []
    for d in range(2):
        W, U, b = parts[3 * d:3 * d + 3]
        h, c = np.zeros((n, H), dt), np.zeros((n, H), dt)
        k = {q: np.zeros((n, T, H), dt) for q in "ifgoc"}
        k["z"] = np.zeros((n, T, 4 * H), dt)
        for s in range(T):
            t = T - 1 - s if d else s
            z = Xb[:, t] @ W + h @ U + b
            i, f, o = _act(z[:, :H], act), _act(z[:, H:2 * H], act), _act(z[:, 3 * H:], act)
            g = np.tanh(z[:, 2 * H:3 * H])
            c = f * c + i * g
            h = o * np.tanh(c)
            X4[:, t, d * H:(d + 1) * H] = h
            for q, v in zip("ifgocz", (i, f, g, o, c, z)):
                k[q][:, s] = v
        keep.append(k)
    return Xb, X4, keep


def forward(Xb, theta, T: int, C: int, act: int = 0, dtype=np.float64):
    """-> (X4 [n][T][128], mo [n][T][6], f [n][16], p [n][C])."""
    X4 = lstm(Xb, theta, T, C, act, dtype)[1]
    return (X4,) + headfit.forward(X4, np.asarray(theta)[N_LSTM4:], T, C, dtype)


def batch_terms(Xb, y, theta, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64):
    """One batch -> (g [P]: the gradient of L, FitStats of the batch with steps = nonfinite = 0)."""
    return batch_terms_dx(Xb, y, theta, T, C, opts, act, dtype)[:2]


def batch_terms_dx(Xb, y, theta, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64):
    """batch_terms and the data gradient behind it -> (g, FitStats, dXb [n][T][256]: the sum over both directions (forward
    first) and all steps of dz W^T - the derivative of the batch's SUM of row losses, not divided by n).  lstm3fit.py goes on
    from it."""
    dt = np.dtype(dtype)
    theta = np.asarray(theta)
    Xb, X4, keep = lstm(Xb, theta, T, C, act, dt)
    n = Xb.shape[0]
    gh, st, dX4 = headfit.batch_terms_dx(X4, y, theta[N_LSTM4:], T, C, opts, dt)
    parts = [a.astype(dt) for a in unpack(theta, T, C)[:6]]
    one = dt.type(1)
    grads = []
    dXb = np.zeros((n, T, D_X), dt)
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
            h_prev = X4[:, (t + 1 if d else t - 1), d * H:(d + 1) * H] if s > 0 else np.zeros((n, H), dt)
            dh = dX4[:, t, d * H:(d + 1) * H] + dz_next @ U.T
            tc = np.tanh(c)
            do = dh * tc
            dc = dh * o * (one - tc * tc) + dcf
            dz = np.concatenate([dc * g * _act_d(i, act), dc * c_prev * _act_d(f, act), dc * i * (one - g * g),
                                 do * _act_d(o, act)], axis=1)
            gW += Xb[:, t].T @ dz
            gU += h_prev.T @ dz
            gb += dz.sum(axis=0)
            dXb[:, t] += dz @ W.T
            dcf = dc * f
            dz_next = dz
        grads += [gW, gU, gb]
    g = np.concatenate([a.ravel() for a in grads]) / dt.type(n)
    return np.concatenate([g.astype(dt), gh]), st, dXb


def epoch(Xb, y, state: FitState, order, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64) -> FitStats:
    """tailfit.epoch's rule on lstm4 rows: consecutive batches of opts.B in the order of `order`, a batch with a non-finite
    gradient skipped and counted, statistics before each update."""
    dt = np.dtype(dtype)
    order = np.asarray(order, np.int64).reshape(-1)
    Xb, y = np.asarray(Xb).reshape(-1, T, D_X), np.asarray(y)
    tot = FitStats()
    for s in range(0, order.size, opts.B):
        idx = order[s:s + opts.B]
        with np.errstate(all="ignore"):
            g, st = batch_terms(Xb[idx], y[idx], state.theta, T, C, opts, act, dt)
        if not np.isfinite(g).all():
            tot.nonfinite += 1
            continue
        state.t += 1
        state.theta, state.m, state.v = adam_step(state.theta, state.m, state.v, g, opts, state.t, dt)
        st.steps = 1
        tot.add(st)
    return tot


def evaluate(Xb, y, theta, order, T: int, C: int, opts: FitOpts, act: int = 0, dtype=np.float64):
    """-> (p [n][C], FitStats): forward only."""
    order = np.asarray(order, np.int64).reshape(-1)
    Xb, y = np.asarray(Xb).reshape(-1, T, D_X)[order], np.asarray(y)[order]
    with np.errstate(all="ignore"):
        X4, _, _, p = forward(Xb, theta, T, C, act, dtype)
        st = FitStats()
        if order.size:
            st = headfit.batch_terms(X4, y, np.asarray(theta)[N_LSTM4:], T, C, opts, dtype)[1]
        return p, st


def fitted_model(m, theta, T: Optional[int] = None):
    """The model with tensors 44 .. 59 replaced by theta's (the 44 tensors in front unchanged)."""
    from .weights import ModelWeights
    T = m.T if T is None else T
    parts = unpack(np.asarray(theta, np.float32), T, m.n_class)[:16]
    ts = list(m.tensors[:44]) + [a.astype(np.float32).copy() for a in parts]
    return ModelWeights(ts, T, m.n_class, m.source + "+lstm4fit")
