"""Cases, restatements and floors shared by tests/test_lstm4fit_host.py (CPU) and tests/test_gpu_lstm4fit.py (MI355X): the
lstm4 depth's twin of tests/headfit_cases.py; tests/tailfit_cases.py's grade_of and adam_f32 are used as they are.

nanoreviser_amd/lstm4fit.py at float64 is the definition of a fitting step at depth NRV_FIT_LSTM4.  Two independent float32
restatements run on the CPU - lstm4fit.py at float32 (NumPy's summation order) and `torch_terms` at torch.float32 (an explicit
step loop of forward ops, differentiated by autograd) - and their deviation from the definition is the f32 FLOOR a third f32
evaluation, the device's, is held to.

A CONDITION ON THE CASES (`condition`, asserted by tests/test_lstm4fit_host.py): the gradient is only continuous in the
arithmetic while every evaluation takes the same side at every ReLU and at every hard-sigmoid clip (z = -2.5 and z = +2.5 of
the i / f / o gates).  Asked for: the three CPU evaluations agree on every side; the fp64 distance of every i / f / o
pre-activation to +-2.5 is at least 8 x the largest f32 - f64 pre-activation difference of the case; both clipped sides and
the open side occur.
"""
import functools

import numpy as np

import headfit_cases as hc
import tailfit_cases as tc
from nanoreviser_amd import lstm4fit as lf
from nanoreviser_amd import tailfit as tf

EPS32, EPS64 = tc.EPS32, tc.EPS64
LSTM_TENSORS = ("W4f", "U4f", "b4f", "W4b", "U4b", "b4b")
TENSORS = LSTM_TENSORS + hc.TENSORS
# (T, model, rows, kind, act): one tile and its edges, two and three tiles, T = 1 (gU of both directions exactly zero), T = 2
# (the first recurrent term), the shipped and the BASELINE window lengths and the longest, a batch without one class, rows of
# all-zero Xb, both gate functions, one batch of the default size
GRAD_CASES = [(11, 0, 1, "plain", 0), (11, 1, 31, "plain", 0), (11, 0, 32, "plain", 0), (11, 1, 33, "plain", 0),
              (1, 0, 33, "plain", 0), (2, 1, 33, "plain", 0), (13, 0, 33, "absent", 0), (13, 1, 31, "zeros", 0),
              (32, 0, 33, "plain", 0), (32, 1, 1, "plain", 0), (11, 1, 33, "plain", 1), (11, 0, 96, "plain", 1),
              (11, 0, 512, "plain", 0)]
HARD_CASES = [c for c in GRAD_CASES if c[4] == 0]
SIGMOID_CASES = [c for c in GRAD_CASES if c[4] == 1]
DEFAULT_SEED = 5
# case -> seed where DEFAULT_SEED does not meet the condition above; found by `find_seed` (see its docstring)
SEEDS = {(11, 1, 33, "plain", 0): 6, (11, 0, 512, "plain", 0): 82}


def n_class(model):
    return 6 if model == 0 else 5


def spans(T, C):
    """Tensor name -> slice of the lstm4 depth's parameter vector."""
    out, at = {}, 0
    for name, n in zip(LSTM_TENSORS, (65536, 16384, 256) * 2):
        out[name] = slice(at, at + n)
        at += n
    for name, s in hc.spans(T, C).items():
        out[name] = slice(at + s.start, at + s.stop)
    assert at == lf.N_LSTM4 and out["Ce"].stop == lf.n_params(T, C)
    return out


def params(T, C, seed):
    """An lstm4 that is neither the shipped one nor zero anywhere - W Glorot-uniform, U ~ N(0, 1/8), small biases of both
    signs - in front of headfit_cases.params."""
    rng = np.random.default_rng(seed + 77)
    lim = np.sqrt(6.0 / (256 + 256))
    parts = []
    for _ in range(2):
        parts += [rng.uniform(-lim, lim, (256, 256)), rng.normal(0, 0.125, (64, 256)), rng.normal(0, 0.1, 256)]
    th = np.concatenate([np.asarray(a, np.float32).ravel() for a in parts] + [hc.params(T, C, seed)])
    assert np.all(th != 0)
    return th.astype(np.float32)


@functools.lru_cache(maxsize=None)
def rows_case(T, model, n, kind="plain", act=0, seed=None):
    """(Xb f32 [n][T][256], y uint8 [n], theta f32 [P]): Xb seeded N(0, 1), as a BatchNorm's output is."""
    if seed is None:
        seed = SEEDS.get((T, model, n, kind, act), DEFAULT_SEED)
    C = n_class(model)
    rng = np.random.default_rng(seed + 1000 * T + 100 * model + n)
    X = rng.normal(0, 1, (n, T, 256)).astype(np.float32)
    y = rng.integers(0, C, n).astype(np.uint8)
    if kind == "absent":
        y[y == 2] = 3
    if kind == "zeros":
        X[::3] = 0
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y, params(T, C, seed + T)


# ---- the torch restatement: forward ops only ---------------------------------------------------------------------------------
def _torch_lstm(x, parts, T, act):
    """x [n][T][256], parts the six LSTM tensors (torch) -> (X4 [n][T][128], the i / f / o pre-activations of every step)."""
    import torch
    n = x.shape[0]
    halves, pre = [], []
    for d in range(2):
        W, U, b = parts[3 * d:3 * d + 3]
        h = torch.zeros((n, 64), dtype=x.dtype)
        c = torch.zeros((n, 64), dtype=x.dtype)
        hs = [None] * T
        for s in range(T):
            t = T - 1 - s if d else s
            z = x[:, t] @ W + h @ U + b
            zi, zf, zg, zo = z[:, :64], z[:, 64:128], z[:, 128:192], z[:, 192:]
            if act == 0:
                i, f, o = (torch.clamp(0.2 * v + 0.5, 0.0, 1.0) for v in (zi, zf, zo))
            else:
                i, f, o = (torch.sigmoid(v) for v in (zi, zf, zo))
            c = f * c + i * torch.tanh(zg)
            h = o * torch.tanh(c)
            hs[t] = h
            pre.append(torch.cat([zi, zf, zo], dim=1))
        halves.append(torch.stack(hs, dim=1))
    return torch.cat(halves, dim=2), pre


def _torch_split(th, T, C):
    sp = spans(T, C)
    lstm = [th[sp[k]].reshape(s) for k, s in zip(LSTM_TENSORS, ((256, 256), (64, 256), (256,)) * 2)]
    return lstm, th[lf.N_LSTM4:]


def torch_terms(Xb, y, theta, T, C, opts, act, dtype):
    """The loss of one batch written with torch forward ops - an explicit step loop, torch.clamp for the hard sigmoid - and
    differentiated by autograd -> (g [P], ce_sum, center_sum, correct).  No gradient formula appears here."""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    th = torch.tensor(np.asarray(theta, np.float64), dtype=tdt, requires_grad=True)
    lstm, thh = _torch_split(th, T, C)
    W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce = hc._split(thh, T, C, lambda a, s: a.reshape(s))
    x = torch.tensor(np.asarray(Xb, np.float64), dtype=tdt).reshape(-1, T, 256)
    x4 = _torch_lstm(x, lstm, T, act)[0]
    yt = torch.tensor(np.asarray(y, np.int64))
    cw = torch.tensor(opts.cw6(), dtype=tdt)[yt]
    mo = torch.relu(torch.relu(torch.relu(x4 @ W1 + b1) @ W2 + b2) @ Wm + bm)
    f = torch.relu(mo.reshape(-1, 6 * T) @ Wf + bf)
    logp = torch.log_softmax(f @ Wo + bo, dim=1)
    b = x.shape[0]
    ce = cw * -logp[torch.arange(b), yt]
    cn = ((f - Ce[yt]) ** 2).sum(dim=1)
    L = ce.sum() / b + float(np.float32(opts.lam)) * cn.sum() / b
    L.backward()
    return (th.grad.detach().numpy().astype(np.float64), float(ce.detach().double().sum()), float(cn.detach().double().sum()),
            int((logp.argmax(dim=1) == yt).sum()))


# ---- the condition on the cases ----------------------------------------------------------------------------------------------
def sides(Xb, theta, T, C, act, how):
    """how: np.float64 / np.float32 (NumPy) or "torch32" -> (every ReLU's side behind this evaluation's own X4, the smallest
    |ReLU pre-activation|, the i / f / o pre-activations of every row and step as float64 [steps x 2][n][192])."""
    if how == "torch32":
        import torch
        th = torch.tensor(np.asarray(theta, np.float32))
        x = torch.tensor(np.asarray(Xb, np.float32)).reshape(-1, T, 256)
        x4, pre = _torch_lstm(x, _torch_split(th, T, C)[0], T, act)
        x4 = x4.numpy()
        pre = np.stack([p.numpy() for p in pre]).astype(np.float64)
    else:
        _, x4, keep = lf.lstm(Xb, theta, T, C, act, how)
        pre = np.stack([k["z"][:, s][:, np.r_[0:128, 192:256]] for k in keep for s in range(T)]).astype(np.float64)
    relu, zmin = hc.relu_sides(x4, np.asarray(theta)[lf.N_LSTM4:], T, C, how)
    return relu, zmin, pre


def clip_side(pre):
    """-1 / 0 / +1: clipped low, open, clipped high."""
    return (pre >= 2.5).astype(np.int8) - (pre <= -2.5).astype(np.int8)


@functools.lru_cache(maxsize=None)
def condition(T, model, n, kind="plain", act=0, seed=None):
    """-> dict(same: the three CPU evaluations agree at every ReLU and clip, kink: the smallest fp64 distance of an i / f / o
    pre-activation to +-2.5, diff: the largest f32 - f64 pre-activation difference, shares: the share of gates clipped low /
    open / clipped high, ok)."""
    C = n_class(model)
    X, y, th = rows_case(T, model, n, kind, act, seed)
    r64, _, p64 = sides(X, th, T, C, act, np.float64)
    r32, _, p32 = sides(X, th, T, C, act, np.float32)
    rt, _, pt = sides(X, th, T, C, act, "torch32")
    same = bool(np.array_equal(r64, r32) and np.array_equal(r64, rt))
    kink = float(np.abs(np.abs(p64) - 2.5).min())
    diff = float(max(np.abs(p32 - p64).max(), np.abs(pt - p64).max()))
    s64 = clip_side(p64)
    shares = tuple(float((s64 == v).mean()) for v in (-1, 0, 1))
    ok = same
    if act == 0:
        same_clip = bool(np.array_equal(s64, clip_side(p32)) and np.array_equal(s64, clip_side(pt)))
        ok = same and same_clip and kink >= 8 * diff and all(v > 0 for v in shares)
    return {"same": same, "kink": kink, "diff": diff, "shares": shares, "ok": bool(ok)}


def find_seed(T, model, n, kind, act, tries=100):
    """The seed search behind SEEDS: the first seed in DEFAULT_SEED, DEFAULT_SEED + 1, ... whose case meets `condition`.  With
    these distributions a gate is beyond each clip with probability of about 0.7 %, the f32 - f64 pre-activation difference is
    about 3e-6, and the nearest kink of 33 rows lies 1e-5 .. 1e-3 away - so most seeds pass for the small cases; of n x T x 384
    pre-activations of the 512-row case one lands within 8 x 3e-6 of +-2.5 for roughly every other seed, which is why that
    case's seed had to be searched for (seed 82 is the first of 5 .. 82 that passes).  Run on the CPU; nothing of the device enters."""
    for seed in range(DEFAULT_SEED, DEFAULT_SEED + tries):
        if condition(T, model, n, kind, act, seed)["ok"]:
            return seed
    raise AssertionError(f"no seed for {(T, model, n, kind, act)}")


# ---- floors and grades -------------------------------------------------------------------------------------------------------
def deviations(x, ref, T, C):
    """Per tensor the largest |x - ref| over its elements."""
    d = np.abs(np.asarray(x, np.float64) - ref)
    return {k: float(d[s].max()) for k, s in spans(T, C).items()}


@functools.lru_cache(maxsize=None)
def grad_reference(T, model, n, kind="plain", act=0):
    """Computed once per case and shared: the definition, the two f32 restatements' deviations from it per tensor, and the
    same for the two sums."""
    C = n_class(model)
    X, y, th = rows_case(T, model, n, kind, act)
    opts = tf.default_opts(model)
    g64, st64 = lf.batch_terms(X, y, th, T, C, opts, act, np.float64)
    g32, st32 = lf.batch_terms(X, y, th, T, C, opts, act, np.float32)
    gt, ce_t, cn_t, ok_t = torch_terms(X, y, th, T, C, opts, act, np.float32)
    sp = spans(T, C)
    return {"g64": g64, "st64": st64, "dev_np": deviations(g32, g64, T, C), "dev_torch": deviations(gt, g64, T, C),
            "scale": {k: float(np.abs(g64[s]).max()) for k, s in sp.items()},
            "sums64": (st64.ce_sum, st64.center_sum), "sums_np": (st32.ce_sum, st32.center_sum), "sums_torch": (ce_t, cn_t)}


def cpu_bound(cases=None):
    """The bound of the device's grade, sized on the CPU alone: the worst grade either f32 restatement gets against the
    floor formed by the OTHER one, over every case, the seventeen tensors and the two sums - doubled, because the device sums
    in a third order.  -> (K, the worst grade)."""
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
