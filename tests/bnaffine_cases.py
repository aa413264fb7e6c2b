"""Cases, restatements and floors shared by tests/test_bnaffine_host.py (CPU) and tests/test_gpu_bnaffine.py (MI355X).

nanoreviser_amd/bnaffine.py at float64 is the definition of a fitting step with gamma and beta of the BatchNorms inside the fitted
section as parameters.  Two independent float32 restatements of the gamma / beta sums run on the CPU - bnaffine.py at float32
(NumPy's summation order) and `torch_terms` at torch.float32: forward ops only, the step loops and the conv block of
fullfit_cases / signalfit_cases / lstm3fit_cases, every BatchNorm inside written as (x - mean) (gamma r) + beta so that autograd
forms the sums in the definition's pivoted form - and their deviation from the definition is the f32 FLOOR a third f32
evaluation, the device's, is held to.

Rows and the depth's own parameters come from the three depths' generators (bnfit_cases.rows_case); gamma, beta and the
statistics are the shipped ecoli model's (of the case's model number), with one variant that zeroes a gamma channel of every
BatchNorm inside and one that zeroes every beta.
"""
import functools

import numpy as np

import bnfit_cases as bc
import fullfit_cases as fc
import headfit_cases as hc
import lstm3fit_cases as l3c
import lstm4fit_cases as l4c
import signalfit_cases as sc_
import tailfit_cases as tc
from nanoreviser_amd import bnaffine as ba
from nanoreviser_amd import bnfit
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import lstm3fit as l3
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.lstm4fit import BN_EPS

EPS32 = tc.EPS32
DEPTHS = bc.DEPTHS
N_BLOCK = {"lstm3": 512, "signal": 544, "full": 864}
# (T, model, rows, act, variant): one row at T = 1; a short last tile at T = 3; two tiles at the shipped window length with both
# models and both gate functions; gamma of channel 1 zero in every BatchNorm inside; every beta zero
SHAPES = [(1, 0, 1, 0, "plain"), (3, 0, 33, 0, "plain"), (11, 0, 64, 0, "plain"), (11, 1, 64, 0, "plain"), (11, 0, 64, 1, "plain"),
          (11, 1, 64, 1, "plain"), (11, 0, 33, 0, "gamma0"), (11, 1, 33, 0, "beta0")]
CHUNK = (2, 0, 4130, 1, "plain")                            # one batch of a full scratch chunk and a short tile (the depths' CHUNK_CASE)
CASES = [(d,) + s for d in DEPTHS for s in SHAPES]
CHUNK_CASES = [(d,) + CHUNK for d in DEPTHS]
CD_CASES = [(d, T, m, 3, a, "plain") for d in DEPTHS for T in (1, 3) for m in (0, 1) for a in (0, 1)]      # central differences
IDS = lambda c: "%s-T%d-m%d-n%d-act%d-%s" % c      # noqa: E731
# K_RECORDED: what cpu_bound() gave over CASES on the machine the cases were written on (x86-64, NumPy and torch CPU builds with
# their default f32 summation orders): 2 x 19.04, the worst restatement grade, met by case ("full", 11, 0, 33, 0, "gamma0"); at lstm3
# depth no case is above 3.8, at signal depth none above 14.5.  The device is held to BOTH this constant and cpu_bound() where the
# test runs (fullfit_cases.cpu_bound says why).
K_RECORDED = 38.08


def n_class(model):
    return 6 if model == 0 else 5


def names(depth):
    """The graded tensors: gamma and beta of every BatchNorm inside, in the block's order."""
    return tuple(f"{k}.{w}" for k in bnfit.inside(depth) for w in ("gamma", "beta"))


def spans(depth):
    return {f"{k}.{w}": s for k, pair in ba.spans(depth).items() for w, s in zip(("gamma", "beta"), pair)}


@functools.lru_cache(maxsize=None)
def block(depth, model, variant="plain"):
    """name -> (gamma, beta) f32 of the BatchNorms inside: the shipped model's, or a variant of them."""
    _, bn = bc.loaded(model)
    out = {}
    for k in bnfit.inside(depth):
        g, b = bn[k][0].copy(), bn[k][1].copy()
        if variant == "gamma0":
            g[1] = 0.0
        if variant == "beta0":
            b[:] = 0.0
        out[k] = (g, b)
    return out


@functools.lru_cache(maxsize=None)
def rows_case(depth, T, model, n, act, variant="plain"):
    """(x, sig | None, y, the vector with the block in front, stats: name -> (mean, var))."""
    x, sig, y, th = bc.rows_case(depth, T, model, n, act)
    vec = ba.pack(depth, block(depth, model, variant), th)
    vec.setflags(write=False)
    return x, sig, y, vec, ba.stats_of(bc.loaded(model)[0])


# ---- the torch restatement: forward ops only ---------------------------------------------------------------------------------
def torch_terms(depth, x, sig, y, vec, stats, T, C, opts, act, dtype):
    """The loss of one batch written with torch forward ops and differentiated by autograd -> (g [block + P], ce_sum, center_sum,
    correct).  No gradient formula appears here."""
    import torch
    import torch.nn.functional as tnf
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=tdt)      # noqa: E731
    v = torch.tensor(np.asarray(vec, np.float64), dtype=tdt, requires_grad=True)
    sp = ba.spans(depth)

    def bn(k, a, axis=-1):
        """(a - mean) (gamma r) + beta over channel axis `axis` of a."""
        shape = [1] * a.dim()
        shape[axis] = -1
        mean, var = (t(s).reshape(shape) for s in stats[k])
        return (a - mean) * (v[sp[k][0]].reshape(shape) / torch.sqrt(var + BN_EPS)) + v[sp[k][1]].reshape(shape)

    th = v[N_BLOCK[depth]:]
    if depth == "lstm3":
        xin, th3 = t(x).reshape(-1, T, 192), th
    else:
        ths = th[ff.N_READ:] if depth == "full" else th
        if depth == "full":
            parts, at = [], 0
            for s in ff._SHAPES:
                k = int(np.prod(s))
                parts.append(th[at:at + k].reshape(s))
                at += k
            h1 = fc._torch_bilstm(t(x).reshape(-1, T, 6), parts[:6], 16, T, act)[0]
            x2 = bn("bn_l2", fc._torch_bilstm(bn("bn_l1", h1), parts[6:], 64, T, act)[0])
        else:
            x2 = t(x).reshape(-1, T, 128)
        w1, b1 = ths[0:24].reshape(3, 1, 8).permute(2, 1, 0), ths[24:32]          # Keras [k][in][out] -> conv1d's [out][in][k]
        w2, b2 = ths[32:224].reshape(3, 8, 8).permute(2, 1, 0), ths[224:232]
        Ws, bs = ths[232:25832].reshape(400, 64), ths[25832:25896]
        s = t(sig).reshape(-1, 1, 50)
        c1 = bn("bn_c1", torch.relu(tnf.conv1d(s, w1, b1, padding=1)), 1)
        f = bn("bn_c2", torch.relu(tnf.conv1d(c1, w2, b2, padding=1)), 1) + s
        S = f.permute(0, 2, 1).reshape(-1, T, 400) @ Ws + bs
        xin, th3 = torch.cat([x2, S], dim=2), ths[sf.N_SIGNAL:]
    p3, th4 = l3c._torch_split(th3, T, C)
    l4p, thh = l4c._torch_split(th4, T, C)
    x4 = l4c._torch_lstm(bn("bn_l3", l3c._torch_lstm3(xin, p3, T, act)[0]), l4p, T, act)[0]
    W1, b1_, W2, b2_, Wm, bm, Wf, bf, Wo, bo, Ce = hc._split(thh, T, C, lambda a, s_: a.reshape(s_))
    yt = torch.tensor(np.asarray(y, np.int64))
    cw = torch.tensor(opts.cw6(), dtype=tdt)[yt]
    mo = torch.relu(torch.relu(torch.relu(x4 @ W1 + b1_) @ W2 + b2_) @ Wm + bm)
    f = torch.relu(mo.reshape(-1, 6 * T) @ Wf + bf)
    logp = torch.log_softmax(f @ Wo + bo, dim=1)
    b = xin.shape[0]
    ce = cw * -logp[torch.arange(b), yt]
    cn = ((f - Ce[yt]) ** 2).sum(dim=1)
    L = ce.sum() / b + float(np.float32(opts.lam)) * cn.sum() / b
    L.backward()
    return (v.grad.detach().numpy().astype(np.float64), float(ce.detach().double().sum()), float(cn.detach().double().sum()),
            int((logp.argmax(dim=1) == yt).sum()))


# ---- floors and grades -------------------------------------------------------------------------------------------------------
def deviations(g, ref, depth):
    """Per gamma / beta tensor the largest |g - ref| over its channels."""
    d = np.abs(np.asarray(g, np.float64)[:N_BLOCK[depth]] - ref[:N_BLOCK[depth]])
    return {k: float(d[s].max()) for k, s in spans(depth).items()}


@functools.lru_cache(maxsize=None)
def reference(depth, T, model, n, act, variant="plain"):
    """Computed once per case and shared: the definition at float64 and the two f32 restatements' deviations from it, per gamma /
    beta tensor."""
    C = n_class(model)
    x, sig, y, vec, stats = rows_case(depth, T, model, n, act, variant)
    opts = tf.default_opts(model)
    g64, st64 = ba.batch_terms(depth, x, sig, y, vec, stats, T, C, opts, act, np.float64)
    g32, _ = ba.batch_terms(depth, x, sig, y, vec, stats, T, C, opts, act, np.float32)
    gt = torch_terms(depth, x, sig, y, vec, stats, T, C, opts, act, np.float32)[0]
    return {"g64": g64, "st64": st64, "dev_np": deviations(g32, g64, depth), "dev_torch": deviations(gt, g64, depth),
            "scale": {k: float(np.abs(g64[s]).max()) for k, s in spans(depth).items()}}


def cpu_bound(cases=None):
    """The bound of the device's grade, sized on the CPU alone by fullfit_cases.cpu_bound's scheme: the worst grade either f32
    restatement gets against the floor formed by the OTHER one, over every case and gamma / beta tensor - doubled, because the
    device sums in a third order.  -> (K, the worst grade)."""
    worst = 1.0
    for c in (cases or CASES):
        r = reference(*c)
        for k in names(c[0]):
            for a, b in ((r["dev_np"][k], r["dev_torch"][k]), (r["dev_torch"][k], r["dev_np"][k])):
                g = tc.grade_of(a, b, r["scale"][k])
                if np.isfinite(g):
                    worst = max(worst, g)
    return 2.0 * worst, worst


def device_grades(g_dev, ref, depth):
    """The device's gamma / beta gradient in units of the floor both restatements form -> {name: grade}."""
    dev = deviations(g_dev, ref["g64"], depth)
    return {k: tc.grade_of(dev[k], max(ref["dev_np"][k], ref["dev_torch"][k]), ref["scale"][k]) for k in names(depth)}
