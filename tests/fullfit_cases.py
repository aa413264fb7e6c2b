"""Cases, restatements and floors shared by tests/test_fullfit_host.py (CPU) and tests/test_gpu_fullfit.py (MI355X): the full
depth's twin of tests/signalfit_cases.py; tests/tailfit_cases.py's grade_of and adam_f32 are used as they are.

nanoreviser_amd/fullfit.py at float64 is the definition of a fitting step at depth NRV_FIT_FULL.  Two independent float32
restatements run on the CPU - fullfit.py at float32 (NumPy's summation order) and `torch_terms` at torch.float32 (forward ops
only: lstm4fit_cases' step loop with the width as an argument for lstm1 and lstm2, the two frozen BatchNorms as one multiply and
one add each, then signalfit_cases._torch_branch and lstm3fit_cases' step loops, differentiated by autograd) - and their
deviation from the definition is the f32 FLOOR a third f32 evaluation, the device's, is held to.

The frozen scales and shifts of the five BatchNorms are those of the shipped ecoli model (of the case's model number).

A CONDITION ON THE CASES (`condition`, asserted by tests/test_fullfit_host.py): signalfit_cases.condition's over the
evaluation's own Xin = [X2b | S], plus, for lstm1 and lstm2, what lstm3fit_cases.condition asks per LSTM at act 0: the three
CPU evaluations agree on every clip side; every i / f / o pre-activation is at least 8 x the case's largest f32 - f64
difference (per layer) away from +-2.5; all three clip regions occur.
"""
import functools

import numpy as np

import headfit_cases as hc
import lstm3fit_cases as l3c
import signalfit_cases as sc_
import tailfit_cases as tc
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import lstm3fit as l3
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf

EPS32, EPS64 = tc.EPS32, tc.EPS64
READ_TENSORS = ("W1f", "U1f", "b1f", "W1b", "U1b", "b1b", "W2f", "U2f", "b2f", "W2b", "U2b", "b2b")
TENSORS = READ_TENSORS + sc_.TENSORS                        # 12 + 29
U_TENSORS = ("U1f", "U1b", "U2f", "U2b", "U3f", "U3b", "U4f", "U4b")
# (T, model, rows, kind, act): one tile and its edges and three tiles at T = 11, T = 1 (gU1 .. gU4 bytes of zero), T = 2, 13 and
# 32, both models and both gate functions, a batch without one class, every third row all-zero feat and sig, `edges` (sig
# non-zero only at samples 0 and 49), one large batch (see SEEDS)
LARGE_ROWS = 160
GRAD_CASES = [(11, 0, 1, "plain", 0), (11, 1, 31, "plain", 0), (11, 0, 32, "plain", 0), (11, 1, 33, "plain", 0),
              (1, 0, 33, "plain", 0), (2, 1, 33, "plain", 0), (13, 0, 33, "absent", 0), (13, 1, 31, "zeros", 0),
              (32, 0, 33, "plain", 0), (11, 0, 33, "edges", 0), (11, 1, 33, "plain", 1), (11, 0, 96, "plain", 1),
              (11, 0, LARGE_ROWS, "plain", 0)]
CHUNK_CASE = (2, 0, 4130, "plain", 1)                       # one batch of two scratch chunks, the last tile short
DEFAULT_SEED = 5
# case -> seed where DEFAULT_SEED does not meet the condition above; found by `find_seed` over the first 200 seeds (5 .. 204).
# THE LARGE CASE has the largest row count among 160, 128, 96 and 64 that has a passing seed: 160 has seed 7 (128 passes at
# DEFAULT_SEED, 96 at 7, 64 at DEFAULT_SEED; no size was without one - see `params` for why).  CHUNK_CASE (8260 pairs, sigmoid
# gates) is asked only that the three CPU evaluations agree on every side, which they do at DEFAULT_SEED.
SEEDS = {(11, 1, 31, "plain", 0): 8, (32, 0, 33, "plain", 0): 12, (11, 0, 96, "plain", 1): 7, (11, 0, 160, "plain", 0): 7}
# K_RECORDED: what cpu_bound() gave over GRAD_CASES on the machine of the seed search (x86-64, NumPy and torch CPU builds with
# their default f32 summation orders): 2 x 31.41, the worst restatement grade, met by case (11, 1, 33, "plain", 0); every other
# case's worst grade is below 15.  The device is held to BOTH this constant and cpu_bound() where the test runs: see cpu_bound.
K_RECORDED = 62.82


def n_class(model):
    return 6 if model == 0 else 5


bn, conv_bn = sc_.bn, sc_.conv_bn


@functools.lru_cache(maxsize=None)
def read_bn(model):
    """(s_l1, h_l1 f32 [32], s_l2, h_l2 f32 [128]) of the shipped ecoli model's bn_l1 and bn_l2 (tensors 18 .. 21, 28 .. 31)."""
    from nanoreviser_amd.weights import load_species
    rb = ff.read_bn(load_species("ecoli")[model])
    for a in rb:
        a.setflags(write=False)
    return rb


def spans(T, C):
    """Tensor name -> slice of the full depth's parameter vector."""
    out, at = {}, 0
    for name, s in zip(READ_TENSORS, ff._SHAPES):
        n = int(np.prod(s))
        out[name] = slice(at, at + n)
        at += n
    for name, s in sc_.spans(T, C).items():
        out[name] = slice(at + s.start, at + s.stop)
    assert at == ff.N_READ == 52608 and out["Ce"].stop == ff.n_params(T, C)
    return out


X2_GAIN = {6: 0.7, 5: 0.3}                                 # by class count: model 1, model 2
W1_LIM, W2_LIM, DEEP_GAIN, CLIP_BIAS = 0.42, 0.021, 0.6, 4.0


def params(T, C, seed):
    """A read branch that is neither the shipped one nor zero anywhere, in front of signalfit_cases.params.

    The condition below asks two things of the i / f / o pre-activations of FOUR LSTMs at once that pull against each other:
    both clips and the open side must occur even in one row, and none of up to a million pre-activations may lie within 8 f32
    differences of +-2.5.  With pre-activations of a standard deviation near 1 - what lstm3fit_cases.params is sized for - the
    T = 32 case has no passing seed among the first 200.  So here the bulk is NARROW and the clips are met by design: every
    LSTM's pre-activations have a standard deviation near 0.6 (lstm1's W uniform with limit W1_LIM on N(0, 1) features; lstm2's
    input is BatchNorm(lstm1) of the shipped statistics, a standard deviation near 10, hence W2_LIM; the input kernels of lstm3
    and lstm4 x DEEP_GAIN), and in each direction of each LSTM the biases of units 0 and 1 of the gates i, f and o are
    +CLIP_BIAS and -CLIP_BIAS: those two units sit in the clipped regions, the others in the open one.  lstm3's input kernels
    of the 128 read columns are further rescaled by X2_GAIN because X2b is BatchNorm(lstm2) of the shipped statistics - a root
    mean square near 1.4 in model 1 and 3.5 in model 2 - not N(0, 1).  U ~ N(0, 0.2) and N(0, 0.1), small biases of both
    signs elsewhere."""
    rng = np.random.default_rng(seed + 377)
    parts = []
    for _ in range(2):
        parts += [rng.uniform(-W1_LIM, W1_LIM, (6, 64)), rng.normal(0, 0.2, (16, 64)), rng.normal(0, 0.1, 64)]
    for _ in range(2):
        parts += [rng.uniform(-W2_LIM, W2_LIM, (32, 256)), rng.normal(0, 0.1, (64, 256)), rng.normal(0, 0.1, 256)]
    th = np.concatenate([np.asarray(a, np.float32).ravel() for a in parts] + [sc_.params(T, C, seed)]).astype(np.float32)
    sp = spans(T, C)
    for d in "fb":
        th[sp["W3" + d]] *= np.float32(DEEP_GAIN)
        th[sp["W3" + d]][:128 * 512] *= np.float32(X2_GAIN[C])
        th[sp["W4" + d]] *= np.float32(DEEP_GAIN)
        for layer, H in (("1", 16), ("2", 64), ("3", 128), ("4", 64)):
            b = th[sp["b" + layer + d]]
            for gate in (0, 1, 3):
                b[gate * H] = CLIP_BIAS
                b[gate * H + 1] = -CLIP_BIAS
    assert np.all(th != 0)
    return th


@functools.lru_cache(maxsize=None)
def rows_case(T, model, n, kind="plain", act=0, seed=None):
    """(feat f32 [n][T][6], sig f32 [n][T][50], y uint8 [n], theta f32 [P]): feat and sig seeded N(0, 1)."""
    if seed is None:
        seed = SEEDS.get((T, model, n, kind, act), DEFAULT_SEED)
    C = n_class(model)
    rng = np.random.default_rng(seed + 1000 * T + 100 * model + n + 59)
    feat = rng.normal(0, 1, (n, T, 6)).astype(np.float32)
    sig = rng.normal(0, 1, (n, T, 50)).astype(np.float32)
    y = rng.integers(0, C, n).astype(np.uint8)
    if kind == "absent":
        y[y == 2] = 3
    if kind == "zeros":
        feat[::3] = 0
        sig[::3] = 0
    if kind == "edges":
        sig[:, :, 1:49] = 0
    for a in (feat, sig, y):
        a.setflags(write=False)
    return feat, sig, y, params(T, C, seed + T)


# ---- the torch restatement: forward ops only ---------------------------------------------------------------------------------
def _torch_bilstm(x, parts, H, T, act):
    """lstm4fit_cases._torch_lstm with the width as an argument: x [n][T][D], parts the six tensors (torch) -> ([h_fw | h_bw]
    [n][T][2H], the i / f / o pre-activations of every step)."""
    import torch
    n = x.shape[0]
    halves, pre = [], []
    for d in range(2):
        W, U, b = parts[3 * d:3 * d + 3]
        h = torch.zeros((n, H), dtype=x.dtype)
        c = torch.zeros((n, H), dtype=x.dtype)
        hs = [None] * T
        for s in range(T):
            t = T - 1 - s if d else s
            z = x[:, t] @ W + h @ U + b
            zi, zf, zg, zo = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
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


def _torch_read(feat, th, rbt, T, act):
    """feat [n][T][6], th the vector (torch), rbt four torch tensors -> (X2b [n][T][128], pre1, pre2)."""
    parts, at = [], 0
    for s in ff._SHAPES:
        n = int(np.prod(s))
        parts.append(th[at:at + n].reshape(s))
        at += n
    h1, pre1 = _torch_bilstm(feat, parts[:6], 16, T, act)
    h2, pre2 = _torch_bilstm(h1 * rbt[0] + rbt[1], parts[6:], 64, T, act)
    return h2 * rbt[2] + rbt[3], pre1, pre2


def _t(a, tdt):
    import torch
    return torch.tensor(np.asarray(a, np.float64), dtype=tdt)


def torch_terms(feat, sig, y, theta, rb, cb, sc, sh, T, C, opts, act, dtype):
    """The loss of one batch written with torch forward ops and differentiated by autograd -> (g [P], ce_sum, center_sum,
    correct).  No gradient formula appears here."""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    th = torch.tensor(np.asarray(theta, np.float64), dtype=tdt, requires_grad=True)
    ft, s = _t(feat, tdt).reshape(-1, T, 6), _t(sig, tdt).reshape(-1, T, 50)
    rbt, cbt, sct, sht = [_t(a, tdt) for a in rb], [_t(a, tdt) for a in cb], _t(sc, tdt), _t(sh, tdt)
    x2, _, _ = _torch_read(ft, th, rbt, T, act)
    ths = th[ff.N_READ:]
    S, _, _ = sc_._torch_branch(s, ths, cbt, T)
    x4, _, _, thh = l3c._torch_forward(torch.cat([x2, S], dim=2), ths[sf.N_SIGNAL:], sct, sht, T, C, act)
    W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce = hc._split(thh, T, C, lambda a, s_: a.reshape(s_))
    yt = torch.tensor(np.asarray(y, np.int64))
    cw = torch.tensor(opts.cw6(), dtype=tdt)[yt]
    mo = torch.relu(torch.relu(torch.relu(x4 @ W1 + b1) @ W2 + b2) @ Wm + bm)
    f = torch.relu(mo.reshape(-1, 6 * T) @ Wf + bf)
    logp = torch.log_softmax(f @ Wo + bo, dim=1)
    b = ft.shape[0]
    ce = cw * -logp[torch.arange(b), yt]
    cn = ((f - Ce[yt]) ** 2).sum(dim=1)
    L = ce.sum() / b + float(np.float32(opts.lam)) * cn.sum() / b
    L.backward()
    return (th.grad.detach().numpy().astype(np.float64), float(ce.detach().double().sum()), float(cn.detach().double().sum()),
            int((logp.argmax(dim=1) == yt).sum()))


# ---- the condition on the cases ----------------------------------------------------------------------------------------------
def read_pre(feat, theta, rb, T, C, act, how):
    """how: np.float64 / np.float32 (NumPy) or "torch32" -> (this evaluation's own X2b [n][T][128] in its own format, the
    i / f / o pre-activations of lstm1 as float64 [steps x 2][n][48], those of lstm2 [steps x 2][n][192])."""
    if how == "torch32":
        import torch
        x2, pre1, pre2 = _torch_read(_t(feat, torch.float32).reshape(-1, T, 6), _t(theta, torch.float32),
                                     [_t(a, torch.float32) for a in rb], T, act)
        return (x2.numpy(), np.stack([p.numpy() for p in pre1]).astype(np.float64),
                np.stack([p.numpy() for p in pre2]).astype(np.float64))
    k = ff.read_branch(feat, theta, rb, T, C, act, how)
    return k["X2b"], l3c._pre(k["k1"], T, 16), l3c._pre(k["k2"], T, 64)


@functools.lru_cache(maxsize=None)
def condition(T, model, n, kind="plain", act=0, seed=None):
    """-> dict(signal: signalfit_cases.condition's terms over each evaluation's own Xin; kink / diff / shares: per new LSTM
    (lstm1, lstm2) the smallest fp64 distance of an i / f / o pre-activation to +-2.5, the largest f32 - f64 pre-activation
    difference and the share of gates clipped low / open / clipped high; same_clip; ok; sides_ok: the three evaluations agree on
    every side - all CHUNK_CASE is asked)."""
    C = n_class(model)
    feat, sig, y, th = rows_case(T, model, n, kind, act, seed)
    rb, cb = read_bn(model), conv_bn(model)
    sc, sh = bn(model)
    hows = (np.float64, np.float32, "torch32")
    rd = [read_pre(feat, th, rb, T, C, act, how) for how in hows]
    kink, diff, shares, same_clip = [], [], [], True
    for i in (1, 2):
        a64 = rd[0][i]
        kink.append(float(np.abs(np.abs(a64) - 2.5).min()))
        diff.append(float(max(np.abs(r[i] - a64).max() for r in rd[1:])))
        s64 = l3c.clip_side(a64)
        shares.append(tuple(float((s64 == v).mean()) for v in (-1, 0, 1)))
        same_clip = same_clip and all(np.array_equal(s64, l3c.clip_side(r[i])) for r in rd[1:])
    # signalfit_cases.condition's body over this depth's Xin: its own function draws its rows itself
    ths = th[ff.N_READ:]
    ev = [sc_.conv_pre(r[0], sig, ths, cb, T, C, how) for r, how in zip(rd, hows)]
    same = all(np.array_equal(ev[0][i] > 0, e[i] > 0) for e in ev[1:] for i in range(2))
    ckink = tuple(float(np.abs(ev[0][i]).min()) for i in range(2))
    cdiff = tuple(float(max(np.abs(e[i] - ev[0][i]).max() for e in ev[1:])) for i in range(2))
    cshares = tuple(float((ev[0][i] > 0).mean()) for i in range(2))
    th3 = ths[sf.N_SIGNAL:]
    sd = [l3c.sides(e[2], th3, sc, sh, T, C, act, how) for e, how in zip(ev, hows)]
    same = bool(same and np.array_equal(sd[0][0], sd[1][0]) and np.array_equal(sd[0][0], sd[2][0]))
    skink, sdiff, sshares, s_clip = [], [], [], True
    for i in (1, 2):
        a64 = sd[0][i]
        skink.append(float(np.abs(np.abs(a64) - 2.5).min()))
        sdiff.append(float(max(np.abs(r[i] - a64).max() for r in sd[1:])))
        s64 = l3c.clip_side(a64)
        sshares.append(tuple(float((s64 == v).mean()) for v in (-1, 0, 1)))
        s_clip = s_clip and all(np.array_equal(s64, l3c.clip_side(r[i])) for r in sd[1:])
    sig_ok = same and all(k >= 8 * d for k, d in zip(ckink, cdiff)) and all(0 < v < 1 for v in cshares)
    sides_ok = bool(same and (act != 0 or (same_clip and s_clip)))
    ok = sig_ok
    if act == 0:
        ok = (ok and s_clip and all(k >= 8 * d for k, d in zip(skink, sdiff)) and all(v > 0 for s in sshares for v in s)
              and same_clip and all(k >= 8 * d for k, d in zip(kink, diff)) and all(v > 0 for s in shares for v in s))
    return {"same": same, "same_clip": bool(same_clip and s_clip), "sides_ok": sides_ok, "kink": tuple(kink), "diff": tuple(diff),
            "shares": tuple(shares),
            "signal": {"conv_kink": ckink, "conv_diff": cdiff, "conv_shares": cshares, "kink": tuple(skink), "diff": tuple(sdiff),
                       "shares": tuple(sshares)}, "ok": bool(ok)}


def find_seed(T, model, n, kind, act, tries=200):
    """The seed search behind SEEDS: the first seed in DEFAULT_SEED, DEFAULT_SEED + 1, ... whose case meets `condition`, or
    None.  Run on the CPU; nothing of the device enters.  (python -c "import fullfit_cases as c; print({k: c.find_seed(*k)
    for k in c.GRAD_CASES})" from tests/.)"""
    for seed in range(DEFAULT_SEED, DEFAULT_SEED + tries):
        if condition(T, model, n, kind, act, seed)["ok"]:
            return seed
    return None


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
    feat, sig, y, th = rows_case(T, model, n, kind, act)
    rb, cb = read_bn(model), conv_bn(model)
    sc, sh = bn(model)
    opts = tf.default_opts(model)
    g64, st64 = ff.batch_terms(feat, sig, y, th, rb, cb, sc, sh, T, C, opts, act, np.float64)
    g32, st32 = ff.batch_terms(feat, sig, y, th, rb, cb, sc, sh, T, C, opts, act, np.float32)
    gt, ce_t, cn_t, ok_t = torch_terms(feat, sig, y, th, rb, cb, sc, sh, T, C, opts, act, np.float32)
    sp = spans(T, C)
    return {"g64": g64, "st64": st64, "dev_np": deviations(g32, g64, T, C), "dev_torch": deviations(gt, g64, T, C),
            "scale": {k: float(np.abs(g64[s]).max()) for k, s in sp.items()},
            "sums64": (st64.ce_sum, st64.center_sum), "sums_np": (st32.ce_sum, st32.center_sum), "sums_torch": (ce_t, cn_t)}


def cpu_bound(cases=None):
    """The bound of the device's grade, sized on the CPU alone exactly as signalfit_cases.cpu_bound sizes it, with its margin:
    the worst grade either f32 restatement gets against the floor formed by the OTHER one, over every case, the forty-one
    tensors and the two sums - doubled, because the device sums in a third order.  -> (K, the worst grade).
    K is sized where the test runs and depends on that machine's f32 summation order (lstm3fit_cases.cpu_bound's docstring: 16
    and 4.6e4 seen), so the device is ALSO held to K_RECORDED, the value this function gave on the machine of the seed search.  A
    restatement that lands on the other side of a ReLU on another host only raises the floor, which lowers the device's grade:
    the recorded bound cannot fail for the host's sake."""
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
