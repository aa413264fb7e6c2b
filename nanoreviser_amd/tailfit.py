"""Fitting the per-window tail: the DEFINITION of what the engine's nrv_fit_* entry points compute (include/nanorev.h,
csrc/nrv_tailfit.h).  NumPy only.

Only the layers behind Flatten(main_out) are fitted - tensors 56 .. 59 of a model: feature.kernel Wf [6T][16], feature.bias
bf [16], final_out.kernel Wo [16][C], final_out.bias bo [C] - together with the centres Ce [C][16] of the reference's centre
loss (lstmmodel.py:63-74).  The 56 tensors in front are frozen, so a window IS its 6T main_out values F (index t * 6 + k).

Every function takes `dtype`: float64 is the definition; float32 is a restatement of it in the engine's number format (same
formulas, NumPy's own summation order), used to size the floors the device is held to - it is not bit-exact with the device,
except `adam_step`, whose float32 form is elementwise and IS the device's update bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

CW1 = (3.0, 5.0, 1.0, 1.0, 1.0, 1.0)      # NanoReviser_train.py:167: {0: 3, 1: 5, 2 .. 5: 1} on model 1's six classes
CW2 = (5.0, 1.0, 1.0, 1.0, 1.0)           # model 2's five classes are model 1's 1 .. 5: "-" keeps its 5 (see README)
LAMBDA = 0.4
MAX_BATCH = 65536                          # NRV_FIT_MAX_BATCH


def n_params(T: int, C: int) -> int:
    """NRV_FIT_PARAMS(T, C)."""
    return 96 * T + 16 + 16 * C + C + 16 * C


@dataclass
class FitOpts:
    B: int = 512
    lr: float = 1e-3
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-7
    lam: float = LAMBDA
    cw: Sequence[float] = CW1

    def cw6(self):
        c = [float(x) for x in self.cw]
        return c + [0.0] * (6 - len(c))


def default_opts(model: int, **kw) -> FitOpts:
    return FitOpts(cw=CW1 if model == 0 else CW2, **kw)


@dataclass
class FitStats:
    rows: int = 0
    correct: int = 0
    ce_sum: float = 0.0
    center_sum: float = 0.0
    steps: int = 0
    nonfinite: int = 0

    def add(self, o: "FitStats"):
        self.rows += o.rows
        self.correct += o.correct
        self.ce_sum += o.ce_sum
        self.center_sum += o.center_sum
        self.steps += o.steps
        self.nonfinite += o.nonfinite

    def loss(self, lam: float = LAMBDA):
        """(loss, ce, center) per row, as a Keras history has them."""
        n = max(self.rows, 1)
        return (self.ce_sum + lam * self.center_sum) / n, self.ce_sum / n, self.center_sum / n

    def acc(self):
        return self.correct / max(self.rows, 1)


# ---- the parameter vector [Wf | bf | Wo | bo | Ce] ------------------------------------------------------------------------
def pack(Wf, bf, Wo, bo, Ce, dtype=np.float32) -> np.ndarray:
    return np.concatenate([np.asarray(a, dtype).ravel() for a in (Wf, bf, Wo, bo, Ce)])


def unpack(theta, T: int, C: int):
    theta = np.asarray(theta)
    K = 6 * T
    sizes, shapes = (16 * K, 16, 16 * C, C, 16 * C), ((K, 16), (16,), (16, C), (C,), (C, 16))
    if theta.size != sum(sizes):
        raise ValueError(f"parameter vector of {theta.size} floats, expected {sum(sizes)} for T={T}, C={C}")
    out, at = [], 0
    for n, s in zip(sizes, shapes):
        out.append(theta[at:at + n].reshape(s))
        at += n
    return out


def params_from_model(m, dtype=np.float32) -> np.ndarray:
    """A model's own tail (tensors 56 .. 59) with zero centres: what nrv_fit_begin(params = NULL) starts from."""
    t = m.tensors
    return pack(t[56], t[57], t[58], t[59], np.zeros((m.n_class, 16)), dtype)


def fresh_params(T: int, C: int, seed: int) -> np.ndarray:
    """Keras' Dense default: Glorot-uniform kernels, zero biases; zero centres."""
    rng = np.random.default_rng(seed)

    def glorot(i, o):
        lim = np.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, (i, o))
    return pack(glorot(6 * T, 16), np.zeros(16), glorot(16, C), np.zeros(C), np.zeros((C, 16)), np.float32)


# ---- labels -------------------------------------------------------------------------------------------------------------
def labelled_windows(labels, ev_len, T: int):
    """The labelled windows of a call, in window order: (w int64 [rows], y1 uint8, y2 uint8).  labels: one byte per event
    (nrv_align_labels' format, 0xFF = unlabelled); ev_len: events per read.  Read r has max(ev_len - T, 0) windows, its window
    i is window ev_off + i of the call and revises event (T - 1) / 2 + i; labelled: byte != 0xFF and code (bits 0 .. 2) 1 .. 5;
    y1 = 0 if bit 4 else code, y2 = code - 1 (the score block's rule)."""
    labels = np.asarray(labels, np.uint8).reshape(-1)
    o, off = (T - 1) // 2, 0
    ws, y1, y2 = [], [], []
    for el in np.asarray(ev_len, np.int64).reshape(-1):
        n_r = max(int(el) - T, 0)
        lb = labels[off + o:off + o + n_r].astype(np.int64)
        code = lb & 7
        ok = (lb != 0xFF) & (code >= 1) & (code <= 5)
        i = np.nonzero(ok)[0]
        ws.append(off + i)
        y1.append(np.where(lb[i] & 16, 0, code[i]))
        y2.append(code[i] - 1)
        off += int(el)
    cat = (lambda a, dt: np.concatenate(a).astype(dt) if a else np.zeros(0, dt))
    return cat(ws, np.int64), cat(y1, np.uint8), cat(y2, np.uint8)


# ---- forward, loss, gradient ---------------------------------------------------------------------------------------------
def forward(F, theta, T: int, C: int, dtype=np.float64):
    """-> (f [n][16], p [n][C])."""
    dt = np.dtype(dtype)
    Wf, bf, Wo, bo, _ = [a.astype(dt) for a in unpack(theta, T, C)]
    F = np.asarray(F).astype(dt).reshape(-1, 6 * T)
    f = np.maximum(F @ Wf + bf, 0)
    l = f @ Wo + bo
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return f, e / e.sum(axis=-1, keepdims=True)


def batch_terms(F, y, theta, T: int, C: int, opts: FitOpts, dtype=np.float64):
    """One batch -> (g [P]: the gradient of L, FitStats of the batch with steps = nonfinite = 0)."""
    dt = np.dtype(dtype)
    Wf, bf, Wo, bo, Ce = [a.astype(dt) for a in unpack(theta, T, C)]
    F = np.asarray(F).astype(dt).reshape(-1, 6 * T)
    y = np.asarray(y).astype(np.int64).reshape(-1)
    b = F.shape[0]
    cw = np.asarray(opts.cw6(), dt)[y]
    lam = dt.type(np.float32(opts.lam))                       # the options as the C-ABI carries them: f32
    f, p = forward(F, theta, T, C, dt)
    rows = np.arange(b)
    onehot = np.zeros((b, C), dt)
    onehot[rows, y] = 1
    d = f - Ce[y]
    with np.errstate(divide="ignore"):
        ce = cw * -np.log(p[rows, y])
    cn = (d * d).sum(axis=1)
    dl = cw[:, None] * (p - onehot)
    df = dl @ Wo.T + dt.type(2) * lam * d
    dz = np.where(f > 0, df, dt.type(0))                      # f = max(z, 0): z > 0 exactly where f > 0
    gCe = np.zeros((C, 16), dt)
    np.add.at(gCe, y, -dt.type(2) * lam * d)
    g = pack(F.T @ dz, dz.sum(axis=0), f.T @ dl, dl.sum(axis=0), gCe, dt) / dt.type(b)
    st = FitStats(rows=b, correct=int((p.argmax(axis=1) == y).sum()), ce_sum=float(ce.astype(np.float64).sum()),
                  center_sum=float(cn.astype(np.float64).sum()))
    return g, st


def lr_t(opts: FitOpts, t: int) -> float:
    """Keras 2.2.4 Adam: lr sqrt(1 - beta2^t) / (1 - beta1^t), t counting from 1; in f64, from the options AS THE C-ABI
    CARRIES THEM (nrv_fit_opts holds f32: 0.999 is 0.99900001287...)."""
    lr, b1, b2 = (float(np.float32(x)) for x in (opts.lr, opts.beta1, opts.beta2))
    return lr * float(np.sqrt(1.0 - b2 ** float(t))) / (1.0 - b1 ** float(t))


def adam_step(theta, m, v, g, opts: FitOpts, t: int, dtype=np.float64):
    """One update, t = the step's number (1 for the first).  At float32 every operation is rounded on its own, 1 - beta is
    formed in f32 and lr_t is the f64 value rounded once: the device's update bit for bit."""
    dt = np.dtype(dtype)
    b1, b2, eps = (dt.type(np.float32(x)) for x in (opts.beta1, opts.beta2, opts.eps))   # as the C-ABI carries them: f32
    lr = dt.type(lr_t(opts, t))
    one = dt.type(1)
    theta, m, v, g = (np.asarray(a, dt) for a in (theta, m, v, g))
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * (g * g)
    return theta - (lr * m) / (np.sqrt(v) + eps), m, v


@dataclass
class FitState:
    theta: np.ndarray
    m: np.ndarray = field(default=None)
    v: np.ndarray = field(default=None)
    t: int = 0

    def __post_init__(self):
        if self.m is None:
            self.m = np.zeros_like(self.theta)
        if self.v is None:
            self.v = np.zeros_like(self.theta)


def epoch(F, y, state: FitState, order, T: int, C: int, opts: FitOpts, dtype=np.float64) -> FitStats:
    """Rows in the order of `order`, consecutive batches of opts.B, the last one short and divided by its own size.  A batch
    whose gradient holds a non-finite value is skipped: no update, t does not advance, it counts in `nonfinite` alone.  The
    statistics are those before each batch's update."""
    dt = np.dtype(dtype)
    order = np.asarray(order, np.int64).reshape(-1)
    F, y = np.asarray(F), np.asarray(y)
    tot = FitStats()
    for s in range(0, order.size, opts.B):
        idx = order[s:s + opts.B]
        with np.errstate(all="ignore"):
            g, st = batch_terms(F[idx], y[idx], state.theta, T, C, opts, dt)
        if not np.isfinite(g).all():
            tot.nonfinite += 1
            continue
        state.t += 1
        state.theta, state.m, state.v = adam_step(state.theta, state.m, state.v, g, opts, state.t, dt)
        st.steps = 1
        tot.add(st)
    return tot


def evaluate(F, y, theta, order, T: int, C: int, opts: FitOpts, dtype=np.float64):
    """-> (p [n][C], FitStats): forward only."""
    order = np.asarray(order, np.int64).reshape(-1)
    F, y = np.asarray(F)[order], np.asarray(y)[order]
    _, st = batch_terms(F, y, theta, T, C, opts, dtype) if order.size else (None, FitStats())
    return forward(F, theta, T, C, dtype)[1], st


def val_split(n: int, fraction: float):
    """Keras' validation_split: the LAST fraction of the rows, in file order, before any shuffling -> (n_train, n_val)."""
    n_val = n - int(n * (1.0 - fraction))
    return n - n_val, n_val


def epoch_order(n_train: int, seed: int, ep: int) -> np.ndarray:
    return np.random.default_rng(seed + ep).permutation(n_train).astype(np.uint32)


def fitted_model(m, theta, T: Optional[int] = None):
    """The model with its tail replaced by theta's Wf, bf, Wo, bo (the 56 tensors in front unchanged)."""
    from .weights import ModelWeights
    T = m.T if T is None else T
    Wf, bf, Wo, bo, _ = unpack(np.asarray(theta, np.float32), T, m.n_class)
    ts = list(m.tensors[:56]) + [a.astype(np.float32).copy() for a in (Wf, bf, Wo, bo)]
    return ModelWeights(ts, T, m.n_class, m.source + "+tailfit")


def write_f32(m, stem: str):
    """`<stem>.f32` and the `<stem>.json` manifest weights.load_f32 reads."""
    import json
    flat = m.flat()
    flat.astype("<f4").tofile(stem + ".f32")
    with open(stem + ".json", "w") as f:
        json.dump({"n_f32": int(flat.size), "T": int(m.T), "n_class": int(m.n_class), "source": m.source}, f)
