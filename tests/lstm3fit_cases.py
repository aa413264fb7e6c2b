"""Cases, restatements and floors shared by tests/test_lstm3fit_host.py (CPU) and tests/test_gpu_lstm3fit.py (MI355X): the
lstm3 depth's twin of tests/lstm4fit_cases.py; tests/tailfit_cases.py's grade_of and adam_f32 are used as they are.

nanoreviser_amd/lstm3fit.py at float64 is the definition of a fitting step at depth NRV_FIT_LSTM3.  Two independent float32
restatements run on the CPU - lstm3fit.py at float32 (NumPy's summation order) and `torch_terms` at torch.float32 (an explicit
step loop of forward ops through BOTH Bi-LSTMs and the frozen BatchNorm between them, differentiated by autograd) - and their
deviation from the definition is the f32 FLOOR a third f32 evaluation, the device's, is held to.

sc and sh of the frozen BatchNorm are those of the shipped ecoli model (of the case's model number).

A CONDITION ON THE CASES (`condition`, asserted by tests/test_lstm3fit_host.py): lstm4fit_cases.condition's, over the gates of
BOTH LSTMs and every ReLU: the three CPU evaluations agree on every side; the fp64 distance of every i / f / o
pre-activation to +-2.5 is at least 8 x the largest f32 - f64 pre-activation difference of the case (per layer); both clipped
sides and the open side occur in each layer.
"""
import functools

import numpy as np

import headfit_cases as hc
import lstm4fit_cases as l4c
import tailfit_cases as tc
from nanoreviser_amd import lstm3fit as lf
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import tailfit as tf

EPS32, EPS64 = tc.EPS32, tc.EPS64
LSTM_TENSORS = ("W3f", "U3f", "b3f", "W3b", "U3b", "b3b")
TENSORS = LSTM_TENSORS + l4c.TENSORS                        # 23
_SHAPES = ((192, 512), (128, 512), (512,)) * 2
# (T, model, rows, kind, act): one tile and its edges, three tiles, T = 1 (gU3 and gU4 of both directions exactly zero), T = 2
# (the first recurrent term), the shipped and the BASELINE window lengths and the longest, a batch without one class, rows of
# all-zero Xin, both gate functions, one large batch (256 rows, not the default 512: see SEEDS)
GRAD_CASES = [(11, 0, 1, "plain", 0), (11, 1, 31, "plain", 0), (11, 0, 32, "plain", 0), (11, 1, 33, "plain", 0),
              (1, 0, 33, "plain", 0), (2, 1, 33, "plain", 0), (13, 0, 33, "absent", 0), (13, 1, 31, "zeros", 0),
              (32, 0, 33, "plain", 0), (32, 1, 1, "plain", 0), (11, 1, 33, "plain", 1), (11, 0, 96, "plain", 1),
              (11, 0, 256, "plain", 0)]
CHUNK_CASE = (2, 0, 4130, "plain", 1)                       # one batch of more than one scratch chunk
HARD_CASES = [c for c in GRAD_CASES if c[4] == 0]
SIGMOID_CASES = [c for c in GRAD_CASES if c[4] == 1]
DEFAULT_SEED = 5
# case -> seed where DEFAULT_SEED does not meet the condition above; found by `find_seed` (see its docstring).
# THE LARGE CASE.  With two LSTMs a 512-row batch at T = 11 has 6.5 million i / f / o pre-activations, and about 11 of them
# are expected within 8 x 3e-6 of +-2.5: (11, 0, 512, "plain", 0) has NO passing seed among the first 200 (5 .. 204), nor has
# any multiple of 32 rows from 288 to 480.  256 rows is the largest multiple of 32 that has one (seed 16); 224 has seed 50,
# 192 seed 7, 160 seed 18, 128 seed 12, 96 seed 8.  So the large case has 256 rows.
SEEDS = {(11, 1, 31, "plain", 0): 6, (11, 1, 33, "plain", 0): 6, (32, 0, 33, "plain", 0): 6, (11, 0, 256, "plain", 0): 16}


def n_class(model):
    return 6 if model == 0 else 5


@functools.lru_cache(maxsize=None)
def bn(model):
    """(sc, sh) f32 [256] of the shipped ecoli model's BatchNorm between lstm3 and lstm4 (tensors 40 .. 43)."""
    from nanoreviser_amd.weights import load_species
    sc, sh = l4.bn_scale_shift(load_species("ecoli")[model])
    sc.setflags(write=False)
    sh.setflags(write=False)
    return sc, sh


def spans(T, C):
    """Tensor name -> slice of the lstm3 depth's parameter vector."""
    out, at = {}, 0
    for name, s in zip(LSTM_TENSORS, _SHAPES):
        n = int(np.prod(s))
        out[name] = slice(at, at + n)
        at += n
    for name, s in l4c.spans(T, C).items():
        out[name] = slice(at + s.start, at + s.stop)
    assert at == lf.N_LSTM3 and out["Ce"].stop == lf.n_params(T, C)
    return out


def params(T, C, seed):
    """An lstm3 that is neither the shipped one nor zero anywhere - W uniform with the limit at which a pre-activation of N(0, 1)
    rows has a standard deviation of about 1 (so that both clips are met even by one row), U ~ N(0, 0.09), small biases of both
    signs - in front of lstm4fit_cases.params (with lstm4's input kernels rescaled, below)."""
    rng = np.random.default_rng(seed + 177)
    lim = 0.115
    parts = []
    for _ in range(2):
        parts += [rng.uniform(-lim, lim, (192, 512)), rng.normal(0, 0.09, (128, 512)), rng.normal(0, 0.1, 512)]
    th4 = l4c.params(T, C, seed)
    for d in range(2):                                     # lstm4's input here is BatchNorm(lstm3), of a standard deviation of about
        at = d * l4.N_DIR                                  # 0.4, not N(0, 1): its input kernels x 2.4, so that lstm4 meets both clips
        th4[at:at + 256 * 256] *= np.float32(2.4)
    th = np.concatenate([np.asarray(a, np.float32).ravel() for a in parts] + [th4])
    assert np.all(th != 0)
    return th.astype(np.float32)


@functools.lru_cache(maxsize=None)
def rows_case(T, model, n, kind="plain", act=0, seed=None):
    """(Xin f32 [n][T][192], y uint8 [n], theta f32 [P]): Xin seeded N(0, 1)."""
    if seed is None:
        seed = SEEDS.get((T, model, n, kind, act), DEFAULT_SEED)
    C = n_class(model)
    rng = np.random.default_rng(seed + 1000 * T + 100 * model + n + 31)
    X = rng.normal(0, 1, (n, T, 192)).astype(np.float32)
    y = rng.integers(0, C, n).astype(np.uint8)
    if kind == "absent":
        y[y == 2] = 3
    if kind == "zeros":
        X[::3] = 0
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y, params(T, C, seed + T)


# ---- the torch restatement: forward ops only ---------------------------------------------------------------------------------
def _torch_lstm3(x, parts, T, act):
    """x [n][T][192], parts the six lstm3 tensors (torch) -> (H3 [n][T][256], the i / f / o pre-activations of every step)."""
    import torch
    n = x.shape[0]
    halves, pre = [], []
    for d in range(2):
        W, U, b = parts[3 * d:3 * d + 3]
        h = torch.zeros((n, 128), dtype=x.dtype)
        c = torch.zeros((n, 128), dtype=x.dtype)
        hs = [None] * T
        for s in range(T):
            t = T - 1 - s if d else s
            z = x[:, t] @ W + h @ U + b
            zi, zf, zg, zo = z[:, :128], z[:, 128:256], z[:, 256:384], z[:, 384:]
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
    return [th[sp[k]].reshape(s) for k, s in zip(LSTM_TENSORS, _SHAPES)], th[lf.N_LSTM3:]


def _torch_forward(x, th, sc, sh, T, C, act):
    """-> (x4, pre3, pre4, the head's vector): both step loops and the BatchNorm as one multiply and one add."""
    l3, th4 = _torch_split(th, T, C)
    h3, pre3 = _torch_lstm3(x, l3, T, act)
    xb4 = h3 * sc + sh
    l4p, thh = l4c._torch_split(th4, T, C)
    x4, pre4 = l4c._torch_lstm(xb4, l4p, T, act)
    return x4, pre3, pre4, thh


def torch_terms(Xin, y, theta, sc, sh, T, C, opts, act, dtype):
    """The loss of one batch written with torch forward ops - explicit step loops through both Bi-LSTMs, the BatchNorm between
    them, torch.clamp for the hard sigmoid - and differentiated by autograd -> (g [P], ce_sum, center_sum, correct).  No
    gradient formula appears here."""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    th = torch.tensor(np.asarray(theta, np.float64), dtype=tdt, requires_grad=True)
    x = torch.tensor(np.asarray(Xin, np.float64), dtype=tdt).reshape(-1, T, 192)
    sct, sht = torch.tensor(np.asarray(sc, np.float64), dtype=tdt), torch.tensor(np.asarray(sh, np.float64), dtype=tdt)
    x4, _, _, thh = _torch_forward(x, th, sct, sht, T, C, act)
    W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce = hc._split(thh, T, C, lambda a, s: a.reshape(s))
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
def _pre(keep, T, Hn):
    return np.stack([k["z"][:, s][:, np.r_[0:2 * Hn, 3 * Hn:4 * Hn]] for k in keep for s in range(T)]).astype(np.float64)


def sides(Xin, theta, sc, sh, T, C, act, how):
    """how: np.float64 / np.float32 (NumPy) or "torch32" -> (every ReLU's side behind this evaluation's own X4, the i / f / o
    pre-activations of lstm3 as float64 [steps x 2][n][384], those of lstm4 [steps x 2][n][192])."""
    if how == "torch32":
        import torch
        th = torch.tensor(np.asarray(theta, np.float32))
        x = torch.tensor(np.asarray(Xin, np.float32)).reshape(-1, T, 192)
        x4, pre3, pre4, _ = _torch_forward(x, th, torch.tensor(np.asarray(sc, np.float32)), torch.tensor(np.asarray(sh, np.float32)),
                                           T, C, act)
        x4 = x4.numpy()
        pre3 = np.stack([p.numpy() for p in pre3]).astype(np.float64)
        pre4 = np.stack([p.numpy() for p in pre4]).astype(np.float64)
    else:
        _, h3, keep3 = lf.lstm(Xin, theta, T, C, act, how)
        _, x4, keep4 = l4.lstm(lf.bn(h3, sc, sh, how), np.asarray(theta)[lf.N_LSTM3:], T, C, act, how)
        pre3, pre4 = _pre(keep3, T, 128), _pre(keep4, T, 64)
    relu, _ = hc.relu_sides(x4, np.asarray(theta)[lf.N_LSTM3 + l4.N_LSTM4:], T, C, how)
    return relu, pre3, pre4


clip_side = l4c.clip_side


@functools.lru_cache(maxsize=None)
def condition(T, model, n, kind="plain", act=0, seed=None):
    """-> dict(same: the three CPU evaluations agree at every ReLU and clip, kink / diff / shares: per layer (lstm3, lstm4) the
    smallest fp64 distance of an i / f / o pre-activation to +-2.5, the largest f32 - f64 pre-activation difference and the
    share of gates clipped low / open / clipped high, ok)."""
    C = n_class(model)
    X, y, th = rows_case(T, model, n, kind, act, seed)
    sc, sh = bn(model)
    r64, *p64 = sides(X, th, sc, sh, T, C, act, np.float64)
    r32, *p32 = sides(X, th, sc, sh, T, C, act, np.float32)
    rt, *pt = sides(X, th, sc, sh, T, C, act, "torch32")
    same = bool(np.array_equal(r64, r32) and np.array_equal(r64, rt))
    kink, diff, shares, same_clip = [], [], [], True
    for a64, a32, at in zip(p64, p32, pt):
        kink.append(float(np.abs(np.abs(a64) - 2.5).min()))
        diff.append(float(max(np.abs(a32 - a64).max(), np.abs(at - a64).max())))
        s64 = clip_side(a64)
        shares.append(tuple(float((s64 == v).mean()) for v in (-1, 0, 1)))
        same_clip = same_clip and bool(np.array_equal(s64, clip_side(a32)) and np.array_equal(s64, clip_side(at)))
    ok = same
    if act == 0:
        ok = same and same_clip and all(k >= 8 * d for k, d in zip(kink, diff)) and all(v > 0 for s in shares for v in s)
    return {"same": same, "kink": tuple(kink), "diff": tuple(diff), "shares": tuple(shares), "ok": bool(ok)}


def find_seed(T, model, n, kind, act, tries=200):
    """The seed search behind SEEDS: the first seed in DEFAULT_SEED, DEFAULT_SEED + 1, ... whose case meets `condition`.  Run
    on the CPU; nothing of the device enters.  (python -c "import lstm3fit_cases as c; print({k: c.find_seed(*k) for k in
    c.GRAD_CASES})" from tests/.)"""
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
    sc, sh = bn(model)
    opts = tf.default_opts(model)
    g64, st64 = lf.batch_terms(X, y, th, sc, sh, T, C, opts, act, np.float64)
    g32, st32 = lf.batch_terms(X, y, th, sc, sh, T, C, opts, act, np.float32)
    gt, ce_t, cn_t, ok_t = torch_terms(X, y, th, sc, sh, T, C, opts, act, np.float32)
    sp = spans(T, C)
    return {"g64": g64, "st64": st64, "dev_np": deviations(g32, g64, T, C), "dev_torch": deviations(gt, g64, T, C),
            "scale": {k: float(np.abs(g64[s]).max()) for k, s in sp.items()},
            "sums64": (st64.ce_sum, st64.center_sum), "sums_np": (st32.ce_sum, st32.center_sum), "sums_torch": (ce_t, cn_t)}


def cpu_bound(cases=None):
    """The bound of the device's grade, sized on the CPU alone exactly as lstm4fit_cases.cpu_bound sizes it: the worst grade
    either f32 restatement gets against the floor formed by the OTHER one, over every case, the twenty-three tensors and the
    two sums - doubled, because the device sums in a third order.  -> (K, the worst grade).
    K is sized where the test runs, so it depends on that machine's f32 summation order: the condition gives the clips a
    margin but asks of the ReLUs only that the three evaluations agree where the seeds were found, and a restatement that
    lands on the other side of one ReLU on another machine raises the floor it forms.  Seen: K = 16.1 on the machine of the
    seed search, 4.6e4 on an MI355X host; the device's own grades were below 3.3 on both.  Giving the ReLUs the clips' margin
    was tried: it leaves the T = 32 and the larger cases without a seed among the first 80."""
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
