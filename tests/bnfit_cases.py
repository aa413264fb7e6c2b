"""Cases, restatements and floors shared by tests/test_bnfit_host.py (CPU) and tests/test_gpu_bnfit.py (MI355X).

nanoreviser_amd/bnfit.py at float64 is the definition of a re-estimation.  Two independent float32 restatements run on the CPU -
bnfit.py at float32 (NumPy's order of operations) and `torch_activations` at torch.float32 (the step loops and the conv block of
fullfit_cases / signalfit_cases / lstm3fit_cases) - both through bnfit.reestimate's own stage loop and f64 sums, so that only the
ACTIVATIONS are restated.  Their deviation from the definition is the f32 floor the device, a third f32 evaluation, is held to.

Parameters and sets come from the three depths' own generators (rows_case of fullfit_cases, signalfit_cases, lstm3fit_cases) with
their own seed tables; the loaded BatchNorms are the shipped ecoli model's.

WHAT IS GRADED.  Per BatchNorm, over its channels: dmean = max |mean - mean64| / sqrt(var64 + eps) and dvar = max |var - var64| /
(var64 + eps), each in units of the floor max(the two restatements' own figure, one f32 rounding of the largest |mean64| / sigma64,
respectively of 1).  Mean and var are f32 tensors, so a last-place difference of one channel is a grade near 1 by itself.

THE SEEDS.  A case's generator seed is the depth's own table's (DEFAULT_SEED 5 or the case's entry in SEEDS); with those every one
of the 24 cases keeps both restatements inside K_RECORDED, so no case needed a seed of its own.  Of the first ten seeds (5 .. 14) of
case ("full", 11, 0, 33, 0) EIGHT do (`seed_search`: worst restatement grades 1.15 .. 1.83; seeds 10 and 12 give 3.43 and 3.65, whose
double is above the bound).
"""
import functools

import numpy as np

import fullfit_cases as fc
import lstm3fit_cases as l3c
import signalfit_cases as sc_
import tailfit_cases as tc
from nanoreviser_amd import bnfit
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd.lstm4fit import BN_EPS

EPS32 = tc.EPS32
DEPTHS = ("lstm3", "signal", "full")
# (T, rows): one row, one tile and one row, five tiles; T = 32; CHUNK: two scratch chunks of 4096 + 34 rows, the last tile short
SHAPES = ((11, 1), (11, 33), (11, 160), (32, 33))
CHUNK = (2, 4130)
# (depth, T, model, rows, act): every depth with both models and both gate functions at one tile and one row, the other shapes with
# model 1 and hard_sigmoid, the two-chunk case with sigmoid gates
CASES = [(d, 11, m, 33, a) for d in DEPTHS for m in (0, 1) for a in (0, 1)] + \
        [(d, T, 0, n, 0) for d in DEPTHS for T, n in SHAPES if (T, n) != (11, 33)] + [(d,) + (CHUNK[0], 0, CHUNK[1], 1) for d in DEPTHS]
IDS = lambda c: "%s-T%d-m%d-n%d-act%d" % c      # noqa: E731
# K_RECORDED: what cpu_bound() gave over CASES on the machine of the seed search (x86-64, NumPy and torch CPU builds with their
# default f32 orders): 2 x 3.25, the worst restatement grade, met by case ("signal", 11, 0, 1, 0); the device is held to BOTH this
# constant and cpu_bound() where the test runs (fullfit_cases.cpu_bound says why)
K_RECORDED = 6.5


def n_class(model):
    return 6 if model == 0 else 5


@functools.lru_cache(maxsize=None)
def loaded(model):
    """(the shipped ecoli model, bnfit.bn_of it)."""
    from nanoreviser_amd.weights import load_species
    m = load_species("ecoli")[model]
    return m, bnfit.bn_of(m)


@functools.lru_cache(maxsize=None)
def rows_case(depth, T, model, n, act, seed=None):
    """(x, sig | None, y, theta) of the depth's own generator: x is feat (full), x2 (signal) or Xin (lstm3)."""
    if depth == "full":
        feat, sig, y, th = fc.rows_case(T, model, n, "plain", act, seed)
        return feat, sig, y, th
    if depth == "signal":
        return sc_.rows_case(T, model, n, "plain", act, seed)
    X, y, th = l3c.rows_case(T, model, n, "plain", act, seed)
    return X, None, y, th


# ---- the torch restatement of the activations ---------------------------------------------------------------------------------
def torch_activations(depth, names, x, sig, theta, pairs, T, C, act=0, dtype=np.float32):
    """bnfit.activations with torch.float32 forward ops: fullfit_cases._torch_bilstm for lstm1 / lstm2, signalfit_cases._torch_branch
    for the conv block, lstm3fit_cases._torch_lstm3."""
    import torch
    t32 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float32)      # noqa: E731
    th = t32(theta)
    out = {}
    if depth == "lstm3":
        parts = l3c._torch_split(th, T, C)[0]
        return {"bn_l3": l3c._torch_lstm3(t32(x).reshape(-1, T, 192), parts, T, act)[0].numpy().reshape(-1, 256)}
    ths = th[ff.N_READ:] if depth == "full" else th
    if depth == "full":
        parts, at = [], 0
        for s in ff._SHAPES:
            k = int(np.prod(s))
            parts.append(th[at:at + k].reshape(s))
            at += k
        s1, h1, s2, h2 = [t32(a) for a in pairs["bn_l1"] + pairs["bn_l2"]]
        H1 = fc._torch_bilstm(t32(x).reshape(-1, T, 6), parts[:6], 16, T, act)[0]
        H2 = fc._torch_bilstm(H1 * s1 + h1, parts[6:], 64, T, act)[0]
        out["bn_l1"], out["bn_l2"] = H1.numpy().reshape(-1, 32), H2.numpy().reshape(-1, 128)
        x2 = H2 * s2 + h2
    else:
        x2 = t32(x).reshape(-1, T, 128)
    S, z1, z2 = sc_._torch_branch(t32(sig).reshape(-1, T, 50), ths, [t32(a) for a in pairs["bn_c1"] + pairs["bn_c2"]], T)
    out["bn_c1"] = torch.relu(z1).permute(0, 2, 1).numpy().reshape(-1, 8)
    out["bn_c2"] = torch.relu(z2).permute(0, 2, 1).numpy().reshape(-1, 8)
    if "bn_l3" in names:
        parts = l3c._torch_split(ths[sf.N_SIGNAL:], T, C)[0]
        out["bn_l3"] = l3c._torch_lstm3(torch.cat([x2, S], dim=2), parts, T, act)[0].numpy().reshape(-1, 256)
    return {k: out[k] for k in names}


# ---- floors and grades -------------------------------------------------------------------------------------------------------
def deviations(stats, ref):
    """name -> (dmean, dvar): the largest normalised deviation over the channels (see WHAT IS GRADED)."""
    out = {}
    for k, r in ref.items():
        v64 = r["var"].astype(np.float64) + BN_EPS
        out[k] = (float(np.max(np.abs(stats[k]["mean"].astype(np.float64) - r["mean"].astype(np.float64)) / np.sqrt(v64))),
                  float(np.max(np.abs(stats[k]["var"].astype(np.float64) - r["var"].astype(np.float64)) / v64)))
    return out


@functools.lru_cache(maxsize=None)
def reference(depth, T, model, n, act, seed=None):
    """Computed once per case and shared: the definition at float64 (`ref`), the two restatements' deviations from it, and the
    scales of the two graded figures."""
    x, sig, y, th = rows_case(depth, T, model, n, act, seed)
    _, bn = loaded(model)
    C, rows = n_class(model), np.arange(n)
    ref = bnfit.reestimate(depth, x, sig, th, bn, rows, T, C, act, np.float64)
    r_np = bnfit.reestimate(depth, x, sig, th, bn, rows, T, C, act, np.float32)
    r_t = bnfit.reestimate(depth, x, sig, th, bn, rows, T, C, act, np.float32, acts=torch_activations)
    scale = {k: (float(np.max(np.abs(r["mean"].astype(np.float64)) / np.sqrt(r["var"].astype(np.float64) + BN_EPS))), 1.0)
             for k, r in ref.items()}
    return {"ref": ref, "dev_np": deviations(r_np, ref), "dev_torch": deviations(r_t, ref), "scale": scale}


def grades(stats, r):
    """The figures of `stats` in units of the floor both restatements form -> {(name, "mean" | "var"): grade}."""
    dev = deviations(stats, r["ref"])
    return {(k, what): tc.grade_of(dev[k][i], max(r["dev_np"][k][i], r["dev_torch"][k][i]), r["scale"][k][i])
            for k in dev for i, what in enumerate(("mean", "var"))}


def restatement_worst(r):
    """The worst grade either restatement gets against the floor formed by the OTHER one."""
    worst = 1.0
    for k in r["ref"]:
        for i in range(2):
            for a, b in ((r["dev_np"][k][i], r["dev_torch"][k][i]), (r["dev_torch"][k][i], r["dev_np"][k][i])):
                g = tc.grade_of(a, b, r["scale"][k][i])
                if np.isfinite(g):
                    worst = max(worst, g)
    return worst


def cpu_bound(cases=None):
    """The bound of the device's grade, sized on the CPU alone by fullfit_cases.cpu_bound's scheme: the worst grade either f32
    restatement gets against the floor formed by the other one, over every case, BatchNorm and figure - doubled, because the device
    is a third evaluation.  -> (K, the worst grade)."""
    worst = max(restatement_worst(reference(*c)) for c in (cases or CASES))
    return 2.0 * worst, worst


def seed_search(case=("full", 11, 0, 33, 0), seeds=range(5, 15)):
    """How many of `seeds` keep both restatements of `case` inside K_RECORDED -> (count, {seed: worst grade}).  CPU only."""
    got = {s: restatement_worst(reference(*case, seed=s)) for s in seeds}
    return sum(2.0 * g <= K_RECORDED for g in got.values()), got


# ---- the exact case of test 1 ------------------------------------------------------------------------------------------------
def dyadic_case(T, n, model=0, seed=3):
    """A signal-depth case whose conv stage 1 is EXACT in f64 in any order: w1 = the identity tap, b1 = 0, so a1 = relu(sig); sig
    multiples of 2^-3 in [-4, 4]; bn_c1's loaded moving_mean multiples of 2^-3 in [0, 2].  Every x - p is then a multiple of 2^-3
    below 8 and its square a multiple of 2^-6 below 64: sums of up to 2^40 of them are exact.
    -> (the model with that moving_mean, x2, sig, y, theta)."""
    from nanoreviser_amd.weights import ModelWeights
    m, _ = loaded(model)
    rng = np.random.default_rng(seed + 1000 * T + n)
    ts = list(m.tensors)
    ts[4] = (rng.integers(0, 17, 8) / 8.0).astype(np.float32).reshape(np.asarray(m.tensors[4]).shape)
    md = ModelWeights(ts, m.T, m.n_class, m.source + "+dyadic")
    C = n_class(model)
    th = sc_.params(T, C, seed).copy()
    sp = sc_.spans(T, C)
    w1 = np.zeros((3, 8), np.float32)
    w1[1] = 1.0
    th[sp["cw1"]] = w1.ravel()
    th[sp["cb1"]] = 0.0
    x2 = rng.normal(0, 1, (n, T, 128)).astype(np.float32)
    sig = (rng.integers(-32, 33, (n, T, 50)) / 8.0).astype(np.float32)
    y = rng.integers(0, C, n).astype(np.uint8)
    return md, x2, sig, y, th
