"""Cases, restatements and floors shared by tests/test_dropout_host.py (CPU) and tests/test_gpu_dropout.py (MI355X).

nanoreviser_amd/dropout.py is the definition of the mask; signalfit.py / fullfit.py / bnaffine.py at float64 with
`drop = dropout.terms(...)` are the definition of a fitting step under it.  Two independent float32 restatements run on the CPU -
the same modules at float32 (NumPy's summation order) and `torch_terms` at torch.float32: forward ops only, the step loops and the
conv block of fullfit_cases / signalfit_cases / lstm3fit_cases with the flattened identity block output multiplied out as
where(mask, F / keepf, 0), differentiated by autograd - and their deviation from the definition is the f32 FLOOR a third f32
evaluation, the device's, is held to.  The mask itself is not restated: it is integer arithmetic with known answers
(tests/test_dropout_host.py) and the device's bytes are compared with it bit for bit.

Rows and parameters come from the depths' own generators (bnfit_cases.rows_case).  THE BATCH of a case is the set's rows in
DESCENDING order, so a row's index in the set is never its position in the batch (nor, in the chunk case, in its scratch chunk):
a mask formed from the position is a shifted mask, which `test_a_shifted_mask_or_a_missing_division_is_far_outside` shows to be
orders of magnitude outside the bound.
"""
import functools

import numpy as np

import bnaffine_cases as bac
import bnfit_cases as bc
import fullfit_cases as fc
import headfit_cases as hc
import lstm3fit_cases as l3c
import lstm4fit_cases as l4c
import signalfit_cases as sc_
import tailfit_cases as tc
from nanoreviser_amd import bnaffine as ba
from nanoreviser_amd import dropout as dr
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.lstm4fit import BN_EPS

DEPTHS = ("signal", "full")
RATE = 0.2
SEED = 0x1234_0000_9ABC_DEF1                                # a non-zero high word
DRAW = (1 << 32) + 3                                        # above 2^32
# (T, model, rows): T 1, 3 and 11 x 1, 33 and 64 rows (33 x 11 pairs are no multiple of the 32-pair workgroup), the models
# alternating, and the largest shape with the other model too.  A DELIBERATE THINNING of the cross product T x rows x model x
# depth (36 gradients with their CPU references) to 20: every T and every row count meets both models and both depths.  The
# model enters the dropout only as a bit of the counter word, which the mask test compares bit for bit at every shape with both
# models; everything else a model changes (C, the class weights) is the depths' own suites' ground.
SHAPES = [(T, (i + j) % 2, n) for i, T in enumerate((1, 3, 11)) for j, n in enumerate((1, 33, 64))] + [(11, 1, 64)]
CHUNK = (2, 0, 4130)                                        # the depths' chunk case: a second scratch chunk of 34 rows; sigmoid gates (act_of)
CASES = [(d,) + s for d in DEPTHS for s in SHAPES]
CHUNK_CASES = [(d,) + CHUNK for d in DEPTHS]
AFFINE_CASES = [(d, T, m, n) for d in DEPTHS for T, m, n in ((3, 1, 33), (11, 0, 64))]      # with nrv_fit_set_bn_affine as well
CD_CASES = [(d, T, m, 3) for d in DEPTHS for T in (1, 3) for m in (0, 1)]                   # central differences
IDS = lambda c: "%s-T%d-m%d-n%d" % c      # noqa: E731
ACT = 0


def act_of(n):
    """The gate function of a case: hard_sigmoid, and sigmoid for the 4130-row batch, which is the depths' own chunk case
    (signalfit_cases.CHUNK_CASE = (2, 0, 4130, "plain", 1)).  See CHUNK_CASE's note in signalfit_cases: among 8260 pairs x
    thousands of hard_sigmoid gates some pre-activation lies within an f32 rounding of a clip and no seed keeps them apart.
    Here, with hard_sigmoid gates and the mask, the nearest of 9.5 million i / f / o pre-activations lies 2.5e-6 from a clip while
    f32 and f64 pre-activations differ by up to 3.3e-6: any f32 evaluation may land on the other side of one, and at full depth
    the two CPU restatements with hard_sigmoid gates are already 7.8e3 floors off EACH OTHER, so no bound sized from them would
    say anything about a third.  Both figures are the CPU's.  With sigmoid gates nothing clips, the case is graded like the
    others, and the dropout's own arithmetic - the mask of the second chunk's rows, the divisions - is what is left to differ."""
    return 1 if n == CHUNK[2] else ACT
# K_RECORDED / K_RECORDED_AFFINE: what cpu_bound() / cpu_bound_affine() gave over CASES / AFFINE_CASES on the machine the cases
# were written on (x86-64, NumPy and torch CPU builds with their default f32 summation orders); the device is held to BOTH the
# constant and the function's value where the test runs (fullfit_cases.cpu_bound says why).  K_RECORDED is 2 x 17.78, the worst
# restatement grade, met by case ("full", 11, 1, 64); at signal depth no case is above 10.6.  K_RECORDED_AFFINE is 2 x 13.04.
K_RECORDED = 35.57
K_RECORDED_AFFINE = 26.09


def n_class(model):
    return 6 if model == 0 else 5


def tensors(depth):
    return fc.TENSORS if depth == "full" else sc_.TENSORS


def spans(depth, T, C):
    return fc.spans(T, C) if depth == "full" else sc_.spans(T, C)


def order_of(n):
    """The batch: the set's rows in descending order."""
    return np.arange(n - 1, -1, -1)


def frozen(depth, model):
    """The BatchNorm arguments of the depth's functions: [rb,] cb, sc, sh."""
    return ((fc.read_bn(model),) if depth == "full" else ()) + (sc_.conv_bn(model),) + tuple(sc_.bn(model))


@functools.lru_cache(maxsize=None)
def batch_case(depth, T, model, n, affine=False):
    """(x, sig, y of the BATCH - the set's rows in order_of(n) -, the vector, the set rows, drop = (mask, keepf), stats | None)."""
    if affine:
        x, sig, y, vec, stats = bac.rows_case(depth, T, model, n, act_of(n), "plain")
    else:
        x, sig, y, vec = bc.rows_case(depth, T, model, n, act_of(n))
        stats = None
    rows = order_of(n)
    drop = dr.terms(SEED, DRAW, model, rows, T, RATE)
    drop[0].setflags(write=False)
    return x[rows], sig[rows], y[rows], vec, rows, drop, stats


def definition(depth, x, sig, y, vec, T, model, drop, dtype, stats=None, act=ACT):
    """The depth's batch_terms (bnaffine's with `stats`) -> (g, FitStats)."""
    C, opts = n_class(model), tf.default_opts(model)
    if stats is not None:
        return ba.batch_terms(depth, x, sig, y, vec, stats, T, C, opts, act, dtype, drop=drop)
    fit = ff if depth == "full" else sf
    return fit.batch_terms(x, sig, y, vec, *frozen(depth, model), T, C, opts, act, dtype, drop=drop)


# ---- the torch restatement: forward ops only ---------------------------------------------------------------------------------
def torch_terms(depth, x, sig, y, vec, T, model, drop, dtype, stats=None, act=ACT):
    """The loss of one batch written with torch forward ops and differentiated by autograd -> (g, ce_sum, center_sum, correct).
    stats = None: vec is the depth's vector and every BatchNorm is a * s + h on the frozen pairs; with stats vec has the gamma /
    beta block in front and every BatchNorm is (a - mean) (gamma r) + beta, as bnaffine_cases writes it.  drop = (mask, keepf) or
    None.  No gradient formula appears here."""
    import torch
    import torch.nn.functional as tnf
    C, opts = n_class(model), tf.default_opts(model)
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=tdt)      # noqa: E731
    v = torch.tensor(np.asarray(vec, np.float64), dtype=tdt, requires_grad=True)
    fz = frozen(depth, model)
    pairs = {"bn_c1": fz[-3][:2], "bn_c2": fz[-3][2:], "bn_l3": fz[-2:]}
    if depth == "full":
        pairs.update(bn_l1=fz[0][:2], bn_l2=fz[0][2:])
    sp = ba.spans(depth) if stats is not None else None

    def bn(k, a, axis=-1):
        shape = [1] * a.dim()
        shape[axis] = -1
        if stats is None:
            return a * t(pairs[k][0]).reshape(shape) + t(pairs[k][1]).reshape(shape)
        mean, var = (t(s).reshape(shape) for s in stats[k])
        return (a - mean) * (v[sp[k][0]].reshape(shape) / torch.sqrt(var + BN_EPS)) + v[sp[k][1]].reshape(shape)

    th = v[ba.n_block(depth):] if stats is not None else v
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
    flat = f.permute(0, 2, 1).reshape(-1, T, 400)          # index p * 8 + o
    if drop is not None:
        keep = torch.tensor(np.asarray(drop[0]).reshape(-1, T, 400) != 0)
        flat = torch.where(keep, flat / float(drop[1]), torch.zeros((), dtype=tdt))
    S = flat @ Ws + bs
    p3, th4 = l3c._torch_split(ths[sf.N_SIGNAL:], T, C)
    l4p, thh = l4c._torch_split(th4, T, C)
    x4 = l4c._torch_lstm(bn("bn_l3", l3c._torch_lstm3(torch.cat([x2, S], dim=2), p3, T, act)[0]), l4p, T, act)[0]
    W1, b1_, W2, b2_, Wm, bm, Wf, bf, Wo, bo, Ce = hc._split(thh, T, C, lambda a, s_: a.reshape(s_))
    yt = torch.tensor(np.asarray(y, np.int64))
    cw = torch.tensor(opts.cw6(), dtype=tdt)[yt]
    mo = torch.relu(torch.relu(torch.relu(x4 @ W1 + b1_) @ W2 + b2_) @ Wm + bm)
    fo = torch.relu(mo.reshape(-1, 6 * T) @ Wf + bf)
    logp = torch.log_softmax(fo @ Wo + bo, dim=1)
    b = x2.shape[0]
    ce = cw * -logp[torch.arange(b), yt]
    cn = ((fo - Ce[yt]) ** 2).sum(dim=1)
    L = ce.sum() / b + float(np.float32(opts.lam)) * cn.sum() / b
    L.backward()
    return (v.grad.detach().numpy().astype(np.float64), float(ce.detach().double().sum()), float(cn.detach().double().sum()),
            int((logp.argmax(dim=1) == yt).sum()))


# ---- floors and grades -------------------------------------------------------------------------------------------------------
def deviations(g, ref, sp):
    d = np.abs(np.asarray(g, np.float64) - ref)
    return {k: float(d[s].max()) for k, s in sp.items()}


@functools.lru_cache(maxsize=None)
def reference(depth, T, model, n, affine=False):
    """Computed once per case and shared: the definition under keep_mask's mask, the two f32 restatements' deviations from it per
    tensor, and the same for the two sums.  affine: the tensors are the gamma / beta of the block in front (bnaffine_cases.spans)."""
    x, sig, y, vec, rows, drop, stats = batch_case(depth, T, model, n, affine)
    act = act_of(n)
    g64, st64 = definition(depth, x, sig, y, vec, T, model, drop, np.float64, stats, act)
    g32, st32 = definition(depth, x, sig, y, vec, T, model, drop, np.float32, stats, act)
    gt, ce_t, cn_t, _ = torch_terms(depth, x, sig, y, vec, T, model, drop, np.float32, stats, act)
    sp = bac.spans(depth) if affine else spans(depth, T, n_class(model))
    return {"g64": g64, "st64": st64, "dev_np": deviations(g32, g64, sp), "dev_torch": deviations(gt, g64, sp),
            "scale": {k: float(np.abs(g64[s]).max()) for k, s in sp.items()},
            "sums64": (st64.ce_sum, st64.center_sum), "sums_np": (st32.ce_sum, st32.center_sum), "sums_torch": (ce_t, cn_t)}


def _worst(cases, affine):
    worst = 1.0
    for c in cases:
        r = reference(*c, affine)
        for k in r["scale"]:
            for a, b in ((r["dev_np"][k], r["dev_torch"][k]), (r["dev_torch"][k], r["dev_np"][k])):
                g = tc.grade_of(a, b, r["scale"][k])
                if np.isfinite(g):
                    worst = max(worst, g)
        if not affine:
            for i in range(2):
                a, b = abs(r["sums_np"][i] - r["sums64"][i]), abs(r["sums_torch"][i] - r["sums64"][i])
                worst = max(worst, tc.grade_of(a, b, abs(r["sums64"][i])), tc.grade_of(b, a, abs(r["sums64"][i])))
    return worst


def cpu_bound(cases=None):
    """The bound of the device's grade, sized on the CPU alone exactly as fullfit_cases.cpu_bound sizes it: the worst grade
    either f32 restatement, with the mask, gets against the floor formed by the OTHER one, over every case, the depth's tensors
    and the two sums - doubled, because the device sums in a third order.  -> (K, the worst grade)."""
    w = _worst(cases or CASES, False)
    return 2.0 * w, w


def cpu_bound_affine(cases=None):
    """bnaffine_cases.cpu_bound's procedure over AFFINE_CASES with the masked dF in the definition -> (K, the worst grade)."""
    w = _worst(cases or AFFINE_CASES, True)
    return 2.0 * w, w


def grades(g, ce, cn, ref):
    """A gradient and the two sums in units of the floor both restatements form -> {name: grade}."""
    dev = {k: float(np.abs(np.asarray(g, np.float64)[s] - ref["g64"][s]).max()) for k, s in ref["spans"].items()}
    out = {k: tc.grade_of(dev[k], max(ref["dev_np"][k], ref["dev_torch"][k]), ref["scale"][k]) for k in dev}
    if ce is not None:
        for i, (name, v) in enumerate((("ce_sum", ce), ("center_sum", cn))):
            fl = max(abs(ref["sums_np"][i] - ref["sums64"][i]), abs(ref["sums_torch"][i] - ref["sums64"][i]))
            out[name] = tc.grade_of(abs(v - ref["sums64"][i]), fl, abs(ref["sums64"][i]))
    return out


def graded(case, affine=False):
    """reference(case) with the spans it was formed over."""
    depth, T, model, n = case
    r = dict(reference(depth, T, model, n, affine))
    r["spans"] = bac.spans(depth) if affine else spans(depth, T, n_class(model))
    return r
