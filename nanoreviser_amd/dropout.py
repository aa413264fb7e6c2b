"""The reference's Dropout(0.2) behind the identity block: the DEFINITION of what the engine's nrv_fit_* entry points drop while
nrv_fit_set_dropout is on (include/nanorev.h, csrc/nrv_dropout.h).  NumPy only.

The reference model is identity block -> Dropout(0.2) -> Flatten -> Dense(400 -> 64); signalfit.py's F [n][T][400] is that
Flatten's output (position-major, channel-minor: f = p * 8 + o), so the dropout acts on F.

THE RULE.  "The same calls give the same bytes" rules out a generator with a state, so the mask is a pure function of (seed, draw,
model, set row, t, element):
  * element f of F belongs to quad q = f // 4;
  * the four words of philox4x32_10(counter = (row, (model << 16) | (t * 100 + q), draw & 0xffffffff, draw >> 32),
    key = (seed & 0xffffffff, seed >> 32)) serve f = 4 q .. 4 q + 3 in order;
  * `row` is the row's index in the fit set - not its position in a batch or a chunk;
  * an element is kept iff its word u >= thr, thr = floor(rate * 2^32) with rate a double;
  * keepf = float32(1 - rate); forward Fd = F / keepf where kept, else 0; backward dF = dFd / keepf where kept, else 0 - both
    DIVISIONS, correctly rounded, as TF 1.12's nn.dropout divides by keep_prob.
t * 100 + q must fit 16 bits, so T <= 655.  `draw` counts batches: nrv_fit_begin sets it to 0, batch k of an nrv_fit_epoch call
uses draw + k and the call advances it by ceil(n / B) (skipped non-finite batches included), nrv_fit_grad drops at the current
draw and leaves it.  Evaluation and the BatchNorm re-estimation never drop.

signalfit.py and fullfit.py take the pair `drop = (mask, keepf)` of `terms` in batch_terms*, and a `Stream` in epoch.

LEFT OUT: the draw counter is not persisted in a written model (a continued run sets it through nrv_fit_set_dropout_draw);
dropout at depths whose signal branch is frozen (there is nothing to drop there); batch-statistics BatchNorm.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
N_FLAT, N_QUADS = 400, 100
MAX_T = 655
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key) -> np.ndarray:
    """The standard generator, ten rounds.  counter [..., 4], key [..., 2] (anything that broadcasts against counter's leading
    axes), both taken as uint32 -> uint32 [..., 4]."""
    c = np.asarray(counter, np.uint64) & _U32
    k = np.asarray(key, np.uint64) & _U32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    m0, m1 = np.uint64(M0), np.uint64(M1)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & _U32, (p0 >> sh) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + np.uint64(W0)) & _U32, (k1 + np.uint64(W1)) & _U32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def threshold(rate: float) -> int:
    """thr = floor(rate * 2^32), rate a double in [0, 1)."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"dropout rate {rate!r} outside [0, 1)")
    return int(np.floor(rate * 4294967296.0))


def keep_scale(rate: float) -> np.float32:
    """keepf = float32(1 - rate)."""
    return np.float32(1.0 - float(rate))


def words(seed: int, draw: int, model: int, rows, T: int) -> np.ndarray:
    """uint32 [len(rows)][T][400]: the word of every element of F."""
    if not 1 <= T <= MAX_T:
        raise ValueError(f"T = {T} outside 1 .. {MAX_T}: t * 100 + q would not fit the counter's 16 bits")
    if model not in (0, 1):
        raise ValueError("model must be 0 or 1")
    seed, draw = int(seed), int(draw)
    if not 0 <= seed < 1 << 64 or not 0 <= draw < 1 << 63:
        raise ValueError("seed must fit 64 bits and draw must lie in 0 .. 2^63 - 1")
    rows = np.asarray(rows, np.uint64).reshape(-1)
    c = np.empty((rows.size, T, N_QUADS, 4), np.uint64)
    c[..., 0] = rows[:, None, None]
    c[..., 1] = (model << 16) | (np.arange(T, dtype=np.uint64)[:, None] * np.uint64(N_QUADS) + np.arange(N_QUADS, dtype=np.uint64))
    c[..., 2] = draw & 0xFFFFFFFF
    c[..., 3] = draw >> 32
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    return philox4x32_10(c, key).reshape(rows.size, T, N_FLAT)


def keep_mask(seed: int, draw: int, model: int, rows, T: int, rate: float = 0.2) -> np.ndarray:
    """uint8 [len(rows)][T][400]: 1 where the element of F is kept.  nrv_fit_dropout_mask returns these bytes."""
    return (words(seed, draw, model, rows, T) >= np.uint32(threshold(rate))).astype(np.uint8)


def terms(seed: int, draw: int, model: int, rows, T: int, rate: float):
    """-> (mask, keepf): the `drop` argument of signalfit / fullfit batch_terms* for these set rows."""
    return keep_mask(seed, draw, model, rows, T, rate), keep_scale(rate)


def apply(x, drop, dt):
    """x [n][T][400] (F, or dFd) through the dropout in format dt: x / keepf where kept, else 0.  drop = None: x itself."""
    if drop is None:
        return x
    mask, keepf = drop
    dt = np.dtype(dt)
    x = np.asarray(x)
    mask = np.asarray(mask).reshape(x.shape)
    with np.errstate(all="ignore"):
        return np.where(mask != 0, (x / dt.type(keepf)).astype(dt), dt.type(0))


class Stream:
    """What nrv_fit_set_dropout holds for one model: rate, seed and the draw counter.  epoch(..., drop=stream) of signalfit /
    fullfit asks `batch(k, idx, T)` for batch k of the call and calls `advance(nb)` once at its end."""

    def __init__(self, rate: float, seed: int, model: int, draw: int = 0):
        self.rate, self.seed, self.model, self.draw = float(rate), int(seed), int(model), int(draw)
        threshold(self.rate)

    def batch(self, k: int, idx, T: int):
        return terms(self.seed, self.draw + k, self.model, idx, T, self.rate)

    def advance(self, nb: int):
        self.draw += int(nb)
