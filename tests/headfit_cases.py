"""Cases, restatements and floors shared by tests/test_headfit_host.py (CPU) and tests/test_gpu_headfit.py (MI355X): the head
depth's twin of tests/tailfit_cases.py, whose grade_of and adam_f32 are used as they are.

nanoreviser_amd/headfit.py at float64 is the definition of a fitting step at depth NRV_FIT_HEAD.  Two independent float32
restatements run on the CPU - headfit.py at float32 (NumPy's summation order) and `torch_terms` at torch.float32 (autograd,
torch's order) - and their deviation from the definition is the f32 FLOOR a third f32 evaluation, the device's, is held to.

A CONDITION ON THE CASES: a gradient through four ReLUs is only continuous in the arithmetic while every evaluation takes the
same side at every ReLU.  `relu_sides` gives the sides and the smallest |pre-activation| of an evaluation; the seeds below are
ones for which the three CPU evaluations agree everywhere (tests/test_headfit_host.py asserts it).
"""
import functools

import numpy as np

import tailfit_cases as tc
from nanoreviser_amd import headfit as hf
from nanoreviser_amd import tailfit as tf

EPS32, EPS64 = tc.EPS32, tc.EPS64
TENSORS = ("W1", "b1", "W2", "b2", "Wm", "bm", "Wf", "bf", "Wo", "bo", "Ce")
# (T, model, rows, kind): rows 1, 31, 32, 33 (one tile and its edges, two tiles), T at both ends, at the shipped and the
# BASELINE value, both class counts, a batch without one class, rows of all-zero X, and one batch of the default size
GRAD_CASES = [(11, 0, 1, "plain"), (11, 1, 31, "plain"), (11, 0, 32, "plain"), (11, 1, 33, "plain"), (1, 0, 33, "plain"),
              (1, 1, 32, "absent"), (13, 0, 33, "absent"), (13, 1, 31, "zeros"), (32, 0, 33, "zeros"), (32, 1, 1, "plain"),
              (11, 0, 512, "plain")]
SEEDS = {}                                     # case -> seed where the default does not meet the condition above
DEFAULT_SEED = 5


def n_class(model):
    return 6 if model == 0 else 5


def spans(T, C):
    """Tensor name -> slice of the head's parameter vector."""
    sizes = (128 * 128, 128, 128 * 32, 32, 32 * 6, 6, 96 * T, 16, 16 * C, C, 16 * C)
    out, at = {}, 0
    for name, n in zip(TENSORS, sizes):
        out[name] = slice(at, at + n)
        at += n
    assert at == hf.n_params(T, C)
    return out


def params(T, C, seed):
    """A head that is neither the shipped one nor zero anywhere: Glorot kernels, small biases of both signs, centres near the
    features' scale."""
    rng = np.random.default_rng(seed)
    th = hf.fresh_params(T, C, seed)
    sp = spans(T, C)
    for k in ("b1", "b2", "bm", "bf", "bo"):
        th[sp[k]] = rng.normal(0, 0.1, sp[k].stop - sp[k].start)
    th[sp["Ce"]] = np.abs(rng.normal(0, 0.5, 16 * C))
    assert np.all(th != 0)
    return th.astype(np.float32)


@functools.lru_cache(maxsize=None)
def rows_case(T, model, n, kind="plain", seed=None):
    """(X f32 [n][T][128], y uint8 [n], theta f32 [P]): X seeded N(0, 0.5) clipped into (-1, 1), as an LSTM output is."""
    if seed is None:
        seed = SEEDS.get((T, model, n, kind), DEFAULT_SEED)
    C = n_class(model)
    rng = np.random.default_rng(seed + 1000 * T + 100 * model + n)
    X = np.clip(rng.normal(0, 0.5, (n, T, 128)), -0.999, 0.999).astype(np.float32)
    y = rng.integers(0, C, n).astype(np.uint8)
    if kind == "absent":
        y[y == 2] = 3
    if kind == "zeros":
        X[::3] = 0
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y, params(T, C, seed + T)


def _split(th, T, C, reshape):
    sp = spans(T, C)
    shapes = ((128, 128), (128,), (128, 32), (32,), (32, 6), (6,), (6 * T, 16), (16,), (16, C), (C,), (C, 16))
    return [reshape(th[sp[k]], s) for k, s in zip(TENSORS, shapes)]


def relu_sides(X, theta, T, C, how):
    """how: np.float64 / np.float32 (NumPy) or "torch32" -> (bool array of every ReLU's side: h1, h2, mo, f of every row and
    t, concatenated; the smallest |pre-activation|)."""
    if how == "torch32":
        import torch
        th = torch.tensor(np.asarray(theta, np.float32))
        W1, b1, W2, b2, Wm, bm, Wf, bf = _split(th, T, C, lambda a, s: a.reshape(s))[:8]
        x = torch.tensor(np.asarray(X, np.float32)).reshape(-1, T, 128)
        z1 = x @ W1 + b1
        z2 = torch.relu(z1) @ W2 + b2
        zm = torch.relu(z2) @ Wm + bm
        zf = torch.relu(zm).reshape(-1, 6 * T) @ Wf + bf
        zs = [z.numpy() for z in (z1, z2, zm, zf)]
    else:
        dt = np.dtype(how)
        W1, b1, W2, b2, Wm, bm, Wf, bf = [a.astype(dt) for a in hf.unpack(theta, T, C)[:8]]
        x = np.asarray(X).astype(dt).reshape(-1, T, 128)
        z1 = x @ W1 + b1
        z2 = np.maximum(z1, 0) @ W2 + b2
        zm = np.maximum(z2, 0) @ Wm + bm
        zf = np.maximum(zm, 0).reshape(-1, 6 * T) @ Wf + bf
        zs = [z1, z2, zm, zf]
    flat = np.concatenate([np.asarray(z, np.float64).ravel() for z in zs])
    return flat > 0, float(np.abs(flat).min())


def torch_terms(X, y, theta, T, C, opts, dtype):
    """The loss of one batch written with torch ops and differentiated by autograd -> (g [P], ce_sum, center_sum, correct).
    Independent of headfit.batch_terms: forward ops only, no gradient formula appears here."""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    th = torch.tensor(np.asarray(theta, np.float64), dtype=tdt, requires_grad=True)
    W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce = _split(th, T, C, lambda a, s: a.reshape(s))
    x = torch.tensor(np.asarray(X, np.float64), dtype=tdt).reshape(-1, T, 128)
    yt = torch.tensor(np.asarray(y, np.int64))
    cw = torch.tensor(opts.cw6(), dtype=tdt)[yt]
    mo = torch.relu(torch.relu(torch.relu(x @ W1 + b1) @ W2 + b2) @ Wm + bm)
    f = torch.relu(mo.reshape(-1, 6 * T) @ Wf + bf)
    logp = torch.log_softmax(f @ Wo + bo, dim=1)
    b = x.shape[0]
    ce = cw * -logp[torch.arange(b), yt]
    cn = ((f - Ce[yt]) ** 2).sum(dim=1)
    L = ce.sum() / b + float(np.float32(opts.lam)) * cn.sum() / b
    L.backward()
    return (th.grad.detach().numpy().astype(np.float64), float(ce.detach().double().sum()), float(cn.detach().double().sum()),
            int((logp.argmax(dim=1) == yt).sum()))


# ---- floors and grades ---------------------------------------------------------------------------------------------------
def deviations(x, ref, T, C):
    """Per tensor the largest |x - ref| over its elements."""
    d = np.abs(np.asarray(x, np.float64) - ref)
    return {k: float(d[s].max()) for k, s in spans(T, C).items()}


@functools.lru_cache(maxsize=None)
def grad_reference(T, model, n, kind="plain"):
    """Computed once per case and shared: the definition, the two f32 restatements' deviations from it per tensor, and the
    same for the two sums."""
    C = n_class(model)
    X, y, th = rows_case(T, model, n, kind)
    opts = tf.default_opts(model)
    g64, st64 = hf.batch_terms(X, y, th, T, C, opts, np.float64)
    g32, st32 = hf.batch_terms(X, y, th, T, C, opts, np.float32)
    gt, ce_t, cn_t, ok_t = torch_terms(X, y, th, T, C, opts, np.float32)
    sp = spans(T, C)
    return {"g64": g64, "st64": st64, "dev_np": deviations(g32, g64, T, C), "dev_torch": deviations(gt, g64, T, C),
            "scale": {k: float(np.abs(g64[s]).max()) for k, s in sp.items()},
            "sums64": (st64.ce_sum, st64.center_sum), "sums_np": (st32.ce_sum, st32.center_sum), "sums_torch": (ce_t, cn_t)}


def cpu_bound(cases=None):
    """The bound of the device's grade, sized on the CPU alone: the worst grade either f32 restatement gets against the
    floor formed by the OTHER one, over every case, the eleven tensors and the two sums - doubled, because the device sums in
    a third order.  -> (K, the worst grade)."""
    worst = 1.0
    for c in (cases or GRAD_CASES):
        r = grad_reference(*c)
        for k in TENSORS:
            for a, b in ((r["dev_np"][k], r["dev_torch"][k]), (r["dev_torch"][k], r["dev_np"][k])):
                g = tc.grade_of(a, b, r["scale"][k])
                if np.isfinite(g):
                    worst = max(worst, g)
        for i in range(2):
            a, b = abs(r["sums_np"][i] - r["sums64"][i]), abs(r["sums_torch"][i] - r["sums64"][i])
            worst = max(worst, tc.grade_of(a, b, abs(r["sums64"][i])), tc.grade_of(b, a, abs(r["sums64"][i])))
    return 2.0 * worst, worst


def device_grades(g_dev, ce_dev, cn_dev, ref, T, C):
    """The device's gradient and sums in units of the floor both restatements form -> {name: grade}."""
    dev = deviations(g_dev, ref["g64"], T, C)
    out = {k: tc.grade_of(dev[k], max(ref["dev_np"][k], ref["dev_torch"][k]), ref["scale"][k]) for k in TENSORS}
    for i, (name, v) in enumerate((("ce_sum", ce_dev), ("center_sum", cn_dev))):
        fl = max(abs(ref["sums_np"][i] - ref["sums64"][i]), abs(ref["sums_torch"][i] - ref["sums64"][i]))
        out[name] = tc.grade_of(abs(v - ref["sums64"][i]), fl, abs(ref["sums64"][i]))
    return out
