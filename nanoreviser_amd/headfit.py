"""Fitting the whole head behind the frozen Bi-LSTMs: the DEFINITION of what the engine's nrv_fit_* entry points compute at
depth NRV_FIT_HEAD (include/nanorev.h, csrc/nrv_headfit.h).  NumPy only.

Fitted are the three per-timestep dense layers behind lstm4 - dense1 W1 [128][128] b1, dense2 W2 [128][32] b2, main_out
Wm [32][6] bm, every one behind a ReLU, tensors 50 .. 55 - and the per-window tail of tailfit.py (tensors 56 .. 59 and the
centres).  The 50 tensors in front are frozen, so a window IS its lstm4 output X [T][128] (forward and backward halves
concatenated as the head kernels read them).  One parameter vector per model,
  [W1 | b1 | W2 | b2 | Wm | bm | Wf | bf | Wo | bo | Ce]          n_params(T, C) = 20838 + tailfit.n_params(T, C) floats,
the last five in the tail's own layout.  Everything behind F[t * 6 + k] = mo_t[k] IS tailfit's: its forward, its loss, its
options, its Adam step, its epoch order and its files are used, not restated.

Every function takes `dtype` as in tailfit: float64 is the definition, float32 a restatement in the engine's number format.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import tailfit
from .tailfit import (FitOpts, FitState, FitStats, adam_step, default_opts, epoch_order, lr_t, val_split,  # noqa: F401
                      write_f32)

D_IN, D1, D2, DM = 128, 128, 32, 6
N_MLP = D_IN * D1 + D1 + D1 * D2 + D2 + D2 * DM + DM          # 20838
_MLP_SHAPES = ((D_IN, D1), (D1,), (D1, D2), (D2,), (D2, DM), (DM,))


def n_params(T: int, C: int) -> int:
    """NRV_FIT_PARAMS_HEAD(T, C)."""
    return N_MLP + tailfit.n_params(T, C)


def pack(W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce, dtype=np.float32) -> np.ndarray:
    return np.concatenate([np.asarray(a, dtype).ravel() for a in (W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce)])


def unpack(theta, T: int, C: int):
    """-> [W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce] (views)."""
    theta = np.asarray(theta)
    if theta.size != n_params(T, C):
        raise ValueError(f"parameter vector of {theta.size} floats, expected {n_params(T, C)} for T={T}, C={C} at head depth")
    out, at = [], 0
    for s in _MLP_SHAPES:
        n = int(np.prod(s))
        out.append(theta[at:at + n].reshape(s))
        at += n
    return out + tailfit.unpack(theta[at:], T, C)


def params_from_model(m, dtype=np.float32) -> np.ndarray:
    """A model's own tensors 50 .. 59 with zero centres: what nrv_fit_begin(params = NULL) starts from at head depth."""
    t = m.tensors
    return pack(*[t[i] for i in range(50, 60)], np.zeros((m.n_class, 16)), dtype)


def fresh_params(T: int, C: int, seed: int) -> np.ndarray:
    """Keras' Dense default for all five layers: Glorot-uniform kernels, zero biases; zero centres."""
    rng = np.random.default_rng(seed)

    def glorot(i, o):
        lim = np.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, (i, o))
    return pack(glorot(D_IN, D1), np.zeros(D1), glorot(D1, D2), np.zeros(D2), glorot(D2, DM), np.zeros(DM),
                glorot(6 * T, 16), np.zeros(16), glorot(16, C), np.zeros(C), np.zeros((C, 16)), np.float32)


def with_tail(theta_head, theta_tail) -> np.ndarray:
    """theta_head with its last five blocks replaced by a tail vector of tailfit's layout."""
    out = np.array(theta_head, np.float32)
    out[N_MLP:] = np.asarray(theta_tail, np.float32)
    return out


# ---- forward, loss, gradient ---------------------------------------------------------------------------------------------
def mlp(X, theta, T: int, C: int, dtype=np.float64):
    """The three per-timestep layers -> (X [n][T][128], h1 [n][T][128], h2 [n][T][32], mo [n][T][6]) in dtype."""
    dt = np.dtype(dtype)
    W1, b1, W2, b2, Wm, bm = [a.astype(dt) for a in unpack(theta, T, C)[:6]]
    X = np.asarray(X).astype(dt).reshape(-1, T, D_IN)
    h1 = np.maximum(X @ W1 + b1, 0)
    h2 = np.maximum(h1 @ W2 + b2, 0)
    mo = np.maximum(h2 @ Wm + bm, 0)
    return X, h1, h2, mo


def forward(X, theta, T: int, C: int, dtype=np.float64):
    """-> (mo [n][T][6], f [n][16], p [n][C])."""
    mo = mlp(X, theta, T, C, dtype)[3]
    f, p = tailfit.forward(mo.reshape(-1, 6 * T), np.asarray(theta)[N_MLP:], T, C, dtype)
    return mo, f, p


def batch_terms(X, y, theta, T: int, C: int, opts: FitOpts, dtype=np.float64):
    """One batch -> (g [P]: the gradient of L, FitStats of the batch with steps = nonfinite = 0)."""
    return batch_terms_dx(X, y, theta, T, C, opts, dtype)[:2]


def batch_terms_dx(X, y, theta, T: int, C: int, opts: FitOpts, dtype=np.float64):
    """batch_terms and the data gradient behind it -> (g, FitStats, dX [b][T][128] = dh1 W1^T: the derivative of the batch's
    SUM of row losses with respect to X - not divided by b, as dh1 is not).  lstm4fit.py goes on from it."""
    dt = np.dtype(dtype)
    theta = np.asarray(theta)
    parts = [a.astype(dt) for a in unpack(theta, T, C)]
    W1, W2, Wm, Wf, Wo, Ce = parts[0], parts[2], parts[4], parts[6], parts[8], parts[10]
    X, h1, h2, mo = mlp(X, theta, T, C, dt)
    y = np.asarray(y).astype(np.int64).reshape(-1)
    b = X.shape[0]
    F = mo.reshape(b, 6 * T)
    # the tail's terms, as tailfit.batch_terms states them (dz is needed on its own here)
    cw = np.asarray(opts.cw6(), dt)[y]
    lam = dt.type(np.float32(opts.lam))
    f, p = tailfit.forward(F, theta[N_MLP:], T, C, dt)
    rows = np.arange(b)
    onehot = np.zeros((b, C), dt)
    onehot[rows, y] = 1
    d = f - Ce[y]
    with np.errstate(divide="ignore"):
        ce = cw * -np.log(p[rows, y])
    cn = (d * d).sum(axis=1)
    dl = cw[:, None] * (p - onehot)
    df = dl @ Wo.T + dt.type(2) * lam * d
    dz = np.where(f > 0, df, dt.type(0))
    gCe = np.zeros((C, 16), dt)
    np.add.at(gCe, y, -dt.type(2) * lam * d)
    # back through the three per-timestep layers: a ReLU's derivative is 1 exactly where its output is > 0
    zero = dt.type(0)
    dF = dz @ Wf.T
    dmo = np.where(mo > 0, dF.reshape(b, T, DM), zero)
    dh2 = np.where(h2 > 0, dmo @ Wm.T, zero)
    dh1 = np.where(h1 > 0, dh2 @ W2.T, zero)
    flat = (lambda a: a.reshape(b * T, -1))
    g = pack(flat(X).T @ flat(dh1), flat(dh1).sum(axis=0), flat(h1).T @ flat(dh2), flat(dh2).sum(axis=0),
             flat(h2).T @ flat(dmo), flat(dmo).sum(axis=0),
             F.T @ dz, dz.sum(axis=0), f.T @ dl, dl.sum(axis=0), gCe, dt) / dt.type(b)
    st = FitStats(rows=b, correct=int((p.argmax(axis=1) == y).sum()), ce_sum=float(ce.astype(np.float64).sum()),
                  center_sum=float(cn.astype(np.float64).sum()))
    return g, st, dh1 @ W1.T


def epoch(X, y, state: FitState, order, T: int, C: int, opts: FitOpts, dtype=np.float64) -> FitStats:
    """tailfit.epoch's rule on head rows: consecutive batches of opts.B in the order of `order`, a batch with a non-finite
    gradient skipped and counted, statistics before each update."""
    dt = np.dtype(dtype)
    order = np.asarray(order, np.int64).reshape(-1)
    X, y = np.asarray(X).reshape(-1, T, D_IN), np.asarray(y)
    tot = FitStats()
    for s in range(0, order.size, opts.B):
        idx = order[s:s + opts.B]
        with np.errstate(all="ignore"):
            g, st = batch_terms(X[idx], y[idx], state.theta, T, C, opts, dt)
        if not np.isfinite(g).all():
            tot.nonfinite += 1
            continue
        state.t += 1
        state.theta, state.m, state.v = adam_step(state.theta, state.m, state.v, g, opts, state.t, dt)
        st.steps = 1
        tot.add(st)
    return tot


def evaluate(X, y, theta, order, T: int, C: int, opts: FitOpts, dtype=np.float64):
    """-> (p [n][C], FitStats): forward only."""
    order = np.asarray(order, np.int64).reshape(-1)
    X, y = np.asarray(X).reshape(-1, T, D_IN)[order], np.asarray(y)[order]
    with np.errstate(all="ignore"):
        _, st = batch_terms(X, y, theta, T, C, opts, dtype) if order.size else (None, FitStats())
        return forward(X, theta, T, C, dtype)[2], st


def fitted_model(m, theta, T: Optional[int] = None):
    """The model with tensors 50 .. 59 replaced by theta's (the 50 tensors in front unchanged)."""
    from .weights import ModelWeights
    T = m.T if T is None else T
    parts = unpack(np.asarray(theta, np.float32), T, m.n_class)[:10]
    ts = list(m.tensors[:50]) + [a.astype(np.float32).copy() for a in parts]
    return ModelWeights(ts, T, m.n_class, m.source + "+headfit")
