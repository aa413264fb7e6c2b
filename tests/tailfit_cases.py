"""Cases, restatements and floors shared by tests/test_tailfit_host.py (CPU) and tests/test_gpu_tailfit.py (MI355X).

nanoreviser_amd/tailfit.py at float64 is the definition of a fitting step.  Two independent float32 restatements run on the
CPU - tailfit.py at float32 (NumPy's summation order) and `torch_terms` at torch.float32 (autograd, torch's order) - and their
deviation from the definition is the f32 FLOOR a third f32 evaluation, the device's, is held to.
"""
import functools

import numpy as np

from nanoreviser_amd import tailfit as tf

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
TENSORS = ("Wf", "bf", "Wo", "bo", "Ce")
# (T, model, rows, kind): rows 1, 31, 32, 33 (one tile and its edges, two tiles), every T the engine accepts at its ends and
# at the shipped and the BASELINE value, both class counts, a batch without one class, rows of all-zero features
GRAD_CASES = [(11, 0, 1, "plain"), (11, 1, 31, "plain"), (11, 0, 32, "plain"), (11, 1, 33, "plain"), (1, 0, 33, "plain"),
              (1, 1, 32, "absent"), (13, 0, 33, "absent"), (13, 1, 31, "zeros"), (32, 0, 33, "zeros"), (32, 1, 1, "plain"),
              (11, 0, 512, "plain"), (13, 1, 76, "plain")]


def n_class(model):
    return 6 if model == 0 else 5


def spans(T, C):
    """Tensor name -> slice of the parameter vector."""
    K = 6 * T
    out, at = {}, 0
    for name, n in zip(TENSORS, (16 * K, 16, 16 * C, C, 16 * C)):
        out[name] = slice(at, at + n)
        at += n
    return out


def params(T, C, seed):
    """A tail that is neither the shipped one nor zero anywhere: Glorot kernels, small biases of both signs, centres near the
    features' scale (so that the centre term pulls on every tensor)."""
    rng = np.random.default_rng(seed)
    th = tf.fresh_params(T, C, seed)
    sp = spans(T, C)
    th[sp["bf"]] = rng.normal(0, 0.1, 16)
    th[sp["bo"]] = rng.normal(0, 0.1, C)
    th[sp["Ce"]] = np.abs(rng.normal(0, 0.5, 16 * C))
    return th.astype(np.float32)


@functools.lru_cache(maxsize=None)
def rows_case(T, model, n, kind="plain", seed=5):
    """(F f32 [n][6T], y uint8 [n], theta f32 [P]): features seeded N(0, 1) clipped at 0 (main_out is behind a ReLU)."""
    C = n_class(model)
    rng = np.random.default_rng(seed + 1000 * T + 100 * model + n)
    F = np.maximum(rng.normal(0, 1, (n, 6 * T)), 0).astype(np.float32)
    y = rng.integers(0, C, n).astype(np.uint8)
    if kind == "absent":
        y[y == 2] = 3
    if kind == "zeros":
        F[::3] = 0
    F.setflags(write=False)
    y.setflags(write=False)
    return F, y, params(T, C, seed + T)


def torch_terms(F, y, theta, T, C, opts, dtype):
    """The loss of one batch written with torch ops and differentiated by autograd -> (g [P], ce_sum, center_sum, correct).
    Independent of tailfit.batch_terms: no gradient formula appears here."""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    th = torch.tensor(np.asarray(theta, np.float64), dtype=tdt, requires_grad=True)
    sp = spans(T, C)
    K = 6 * T
    Wf, bf, Wo = th[sp["Wf"]].reshape(K, 16), th[sp["bf"]], th[sp["Wo"]].reshape(16, C)
    bo, Ce = th[sp["bo"]], th[sp["Ce"]].reshape(C, 16)
    Ft = torch.tensor(np.asarray(F, np.float64), dtype=tdt).reshape(-1, K)
    yt = torch.tensor(np.asarray(y, np.int64))
    cw = torch.tensor(opts.cw6(), dtype=tdt)[yt]
    f = torch.relu(Ft @ Wf + bf)
    logp = torch.log_softmax(f @ Wo + bo, dim=1)
    ce = cw * -logp[torch.arange(Ft.shape[0]), yt]
    cn = ((f - Ce[yt]) ** 2).sum(dim=1)
    b = Ft.shape[0]
    L = ce.sum() / b + float(np.float32(opts.lam)) * cn.sum() / b
    L.backward()
    return (th.grad.detach().numpy().astype(np.float64), float(ce.detach().double().sum()), float(cn.detach().double().sum()),
            int((logp.argmax(dim=1) == yt).sum()))


# ---- floors and grades ---------------------------------------------------------------------------------------------------
def deviations(x, ref, T, C):
    """Per tensor the largest |x - ref| over its elements."""
    d = np.abs(np.asarray(x, np.float64) - ref)
    return {k: float(d[s].max()) for k, s in spans(T, C).items()}


def grade_of(dev, floor, scale):
    """A deviation in units of a floor.  The floor is never below one f32 rounding of the tensor's largest element (a
    restatement can be exact by luck); where that is zero too - a tensor whose definition is exactly 0 - only 0 passes."""
    fl = max(floor, EPS32 * scale)
    if fl == 0.0:
        return 0.0 if dev == 0.0 else float("inf")
    return dev / fl


@functools.lru_cache(maxsize=None)
def grad_reference(T, model, n, kind="plain"):
    """Computed once per case and shared: the definition, the two f32 restatements' deviations from it per tensor, and the
    same for the two sums.  -> dict(g64, st64, dev_np, dev_torch, scale, sums64, sums_np, sums_torch)."""
    C = n_class(model)
    F, y, th = rows_case(T, model, n, kind)
    opts = tf.default_opts(model)
    g64, st64 = tf.batch_terms(F, y, th, T, C, opts, np.float64)
    g32, st32 = tf.batch_terms(F, y, th, T, C, opts, np.float32)
    gt, ce_t, cn_t, ok_t = torch_terms(F, y, th, T, C, opts, np.float32)
    sp = spans(T, C)
    return {"g64": g64, "st64": st64, "dev_np": deviations(g32, g64, T, C), "dev_torch": deviations(gt, g64, T, C),
            "scale": {k: float(np.abs(g64[s]).max()) for k, s in sp.items()},
            "sums64": (st64.ce_sum, st64.center_sum), "sums_np": (st32.ce_sum, st32.center_sum), "sums_torch": (ce_t, cn_t)}


def cpu_bound(cases=None):
    """The bound of the device's grade, sized on the CPU alone: the worst grade either f32 restatement gets against the
    floor formed by the OTHER one, over every case, tensor and sum - doubled, because the device sums in a third order.
    -> (K, the worst grade)."""
    worst = 1.0
    for c in (cases or GRAD_CASES):
        r = grad_reference(*c)
        for k in TENSORS:
            for a, b in ((r["dev_np"][k], r["dev_torch"][k]), (r["dev_torch"][k], r["dev_np"][k])):
                g = grade_of(a, b, r["scale"][k])
                if np.isfinite(g):
                    worst = max(worst, g)
        for i in range(2):
            a, b = abs(r["sums_np"][i] - r["sums64"][i]), abs(r["sums_torch"][i] - r["sums64"][i])
            worst = max(worst, grade_of(a, b, abs(r["sums64"][i])), grade_of(b, a, abs(r["sums64"][i])))
    return 2.0 * worst, worst


def device_grades(g_dev, ce_dev, cn_dev, ref, T, C):
    """The device's gradient and sums in units of the floor both restatements form -> {name: grade}."""
    dev = deviations(g_dev, ref["g64"], T, C)
    out = {k: grade_of(dev[k], max(ref["dev_np"][k], ref["dev_torch"][k]), ref["scale"][k]) for k in TENSORS}
    for i, (name, v) in enumerate((("ce_sum", ce_dev), ("center_sum", cn_dev))):
        fl = max(abs(ref["sums_np"][i] - ref["sums64"][i]), abs(ref["sums_torch"][i] - ref["sums64"][i]))
        out[name] = grade_of(abs(v - ref["sums64"][i]), fl, abs(ref["sums64"][i]))
    return out


# ---- Adam, written out -----------------------------------------------------------------------------------------------------
def adam_f32(theta, m, v, g, opts, t):
    """NumPy-f32 elementwise Adam, every operation rounded on its own: the device's update bit for bit (include/nanorev.h)."""
    f = np.float32
    b1, b2, eps = f(opts.beta1), f(opts.beta2), f(opts.eps)
    lr = f(float(f(opts.lr)) * np.sqrt(1.0 - float(b2) ** float(t)) / (1.0 - float(b1) ** float(t)))   # in f64, rounded once
    theta, m, v, g = (np.asarray(a, f) for a in (theta, m, v, g))
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * (g * g)
    return theta - (lr * m) / (np.sqrt(v) + eps), m, v
