"""Weights outside the shipped range, shared by tests/test_weight_cases_host.py and tests/test_gpu_weight_range.py (no test here).

`reparam(m, site, c)` moves a model along one of the graph's exact symmetries: a producer's output is scaled by c and the
rows of its consumer that read it by 1 / c.  BatchNorm and the linear dense layer allow it directly, the ReLU layers because
ReLU is positively homogeneous.  With c a power of two every f32 and f64 operation of the graph commutes with the scaling, so
the oracle's result does not move by one bit - what moves is every magnitude the f16x2 scale planner (nrv_api.hip upload_model)
derives its exponents from.  `lstm3_perm` renumbers the 128 hidden units of lstm3 (exact up to the summation order of its
consumers).  `degenerate(m, name)` zeroes or shrinks whole tensors: NOT function preserving, the oracle is recomputed for them.
`plan_terms(m)` mirrors the f16x2 exponent plan; `plan_case(m, name)` starves input rows until another term of that plan binds
and `unseen(m, other, name)` builds weights of other families (hybrids of the two species, jitter, pruning, outliers, a fresh
initialisation): live oracle for both.  `extreme_windows()` are the inputs of tests/test_gpu_parity.py's extreme-input test.

Tensor numbers are positions in nanoreviser_amd.weights.ROLES; every product is formed in f32."""
import numpy as np

from nanoreviser_amd.weights import ModelWeights

# site -> (tensors x c, [(tensor, row slice or None = whole tensor)] x 1 / c), in the order `all` applies them
SITES = {
    "bn_l1": ((18, 19), ((22, None), (25, None))),
    "bn_l2": ((28, 29), ((34, slice(0, 128)), (37, slice(0, 128)))),
    "sig_dense": ((32, 33), ((34, slice(128, 192)), (37, slice(128, 192)))),
    "bn_l3": ((40, 41), ((44, None), (47, None))),
    "dense1": ((50, 51), ((52, None),)),
    "dense2": ((52, 53), ((54, None),)),
    "main_out": ((54, 55), ((56, None),)),
    "conv1": ((0, 1, 4), ((2, None),)),
    "bn1": ((2, 3), ((6, None),)),
    "conv2": ((6, 7, 10), ((8, None),)),
}
REPARAM_CASES = list(SITES) + ["all", "lstm3_perm"]
DEGENERATE_CASES = ["lstm2_rec0", "sig_dense0", "bn_l2_gamma0", "dense1_0", "conv2_0", "conv1_ch0", "lstm4_tiny"]
SIGNAL_SITES = ("sig_dense", "conv1", "bn1", "conv2", "all")     # the cases that touch a tensor of the signal branch
PERM_SEED = 3128


def _copy(m):
    return [np.array(t, np.float32, copy=True) for t in m.tensors]


def _apply_site(ts, site, c):
    up, down = SITES[site]
    c, r = np.float32(c), np.float32(1.0) / np.float32(c)
    for i in up:
        ts[i] = (ts[i] * c).astype(np.float32)
    for i, rows in down:
        if rows is None:
            ts[i] = (ts[i] * r).astype(np.float32)
        else:
            ts[i][rows] = ts[i][rows] * r


def _lstm3_perm(ts):
    H = 128
    perm = np.random.default_rng(PERM_SEED).permutation(H)
    cols = np.concatenate([g * H + perm for g in range(4)])       # the same renumbering inside each gate block
    for d, base in enumerate((34, 37)):                           # fw, bw
        ts[base] = np.ascontiguousarray(ts[base][:, cols])
        ts[base + 1] = np.ascontiguousarray(ts[base + 1][perm][:, cols])
        ts[base + 2] = np.ascontiguousarray(ts[base + 2][cols])
    out = np.concatenate([perm, H + perm])                        # the layer's 256 outputs: [fw 128 | bw 128]
    for i in (40, 41, 42, 43):
        ts[i] = np.ascontiguousarray(ts[i][out])
    for i in (44, 47):
        ts[i] = np.ascontiguousarray(ts[i][out])


def reparam(m, site, c=1.0):
    """The model `m` with the reparametrisation `site` at factor c (a power of two); `all`: every site at once, alternately
    at c and 1 / c in table order; `lstm3_perm` ignores c."""
    if float(c) <= 0 or np.frexp(float(c))[0] != 0.5:
        raise ValueError("c must be a positive power of two")
    ts = _copy(m)
    if site == "lstm3_perm":
        _lstm3_perm(ts)
    elif site == "all":
        for k, s in enumerate(SITES):
            _apply_site(ts, s, c if k % 2 == 0 else 1.0 / c)
    else:
        _apply_site(ts, site, c)
    return ModelWeights(ts, m.T, m.n_class, f"{m.source}+{site}@{c:g}")


def degenerate(m, name):
    ts = _copy(m)
    if name == "lstm2_rec0":
        ts[23][...] = 0
        ts[26][...] = 0
    elif name == "sig_dense0":
        ts[32][...] = 0
        ts[33][...] = 0
    elif name == "bn_l2_gamma0":
        ts[28][::4] = 0
    elif name == "dense1_0":
        ts[50][...] = 0
    elif name == "conv2_0":
        ts[6][...] = 0
    elif name == "conv1_ch0":
        ts[0][:, :, 0] = 0
        ts[1][0] = 0
    elif name == "lstm4_tiny":
        for i in range(44, 50):
            ts[i] = (ts[i] * np.float32(2.0 ** -20)).astype(np.float32)
    else:
        raise ValueError(name)
    return ModelWeights(ts, m.T, m.n_class, f"{m.source}+{name}")


def case_windows(reads, key="ch10_read5252", lo=1000, n=256, T=11):
    """The 256 windows every weight-range test runs on (the slice of tests/test_gpu_range.py)."""
    from nanoreviser_amd import hoststage as hs
    _, _, rt = reads(key)
    sw, fw = hs.sliding_windows(rt.sig_ev, rt.feat_ev, T)
    return np.ascontiguousarray(sw[lo:lo + n]), np.ascontiguousarray(fw[lo:lo + n])


def conv1_sample_bound(m):
    """The engine's static bound (nrv_api.hip upload_model, cnn_r_kernel's ep[24]): below it no conv1 + BatchNorm
    output can leave the f16 range of the f16x2 signal branch (|c1| x 2^6 <= 65504)."""
    w, b, g, be, mu, var = [np.asarray(x, np.float64) for x in m.tensors[:6]]
    inv = g / np.sqrt(var + 1e-3)
    sh = be - mu * inv
    return float((((1000.0 - np.abs(sh)) / np.abs(inv) - np.abs(b)) / np.abs(w[:, 0, :]).sum(0)).min())


# ---- the f16x2 exponent plan, mirrored ------------------------------------------------------------------------------------
# What nrv_api.hip derives from the weights at nrv_create, restated so that a test can PROVE which branch of the plan a case
# reaches (like conv1_sample_bound above).  Never the expected output of anything.
LAYERS = ("lstm2", "lstm3", "lstm4")                             # the 32->64, 192->128 and 256->64 Bi-LSTM layers
_LBASE = {"lstm2": 22, "lstm3": 34, "lstm4": 44}
SIGNAL_EXP = 6                                                   # the signal branch's output travels x 2^6 (upload_model sS)


def room(bound):
    """pow2_room: the largest s with bound x 2^s <= 2^14."""
    bound = float(bound)
    return 14 if not bound > 0 else 14 - int(np.frexp(bound)[1])


def _bn_fold(ts, base):
    g, be, mu, var = (np.asarray(ts[base + i], np.float32) for i in range(4))
    inv = (g / np.sqrt(var + np.float32(1e-3))).astype(np.float32)
    return inv, (be - mu * inv).astype(np.float32)


def plan_terms(m):
    """{"lstm2" | "lstm3" | "lstm4": {"input", "signal" (None where the layer has no signal rows), "recurrent", "E"},
    "head": {"u1", "u2", "u3", "s1", "s2"}, "bn": (sX1, sX2, sX3)} as upload_model computes them: bn_fold with eps 1e-3 in
    f32; lstm2 reads the BatchNorm'd buffer x 2^sX1, the two layers behind it read h x 2^13 with their BatchNorm folded into
    the input rows (W x scale in f32) before pow2_room; every candidate is the minimum over both directions."""
    ts = [np.asarray(t, np.float32) for t in m.tensors]
    folds = {b: _bn_fold(ts, b) for b in (18, 28, 40)}
    bn = tuple(room(float((np.abs(sc) + np.abs(sh)).max())) for sc, sh in folds.values())
    out = {"bn": bn}
    for name in LAYERS:
        base = _LBASE[name]
        cin, csig, crec = [], [], []
        for d in range(2):
            W, U = ts[base + 3 * d], ts[base + 3 * d + 1]
            if name == "lstm2":
                cin.append(bn[0] + room(np.abs(W).max()))
            else:
                K0 = 128 if name == "lstm3" else 256
                sc = folds[28 if name == "lstm3" else 40][0]
                cin.append(13 + room(np.abs((W[:K0] * sc[:, None]).astype(np.float32)).max()))
                if name == "lstm3":
                    csig.append(SIGNAL_EXP + room(np.abs(W[K0:]).max()))
            crec.append(13 + room(np.abs(U).max()))
        t = {"input": min(cin), "signal": min(csig) if csig else None, "recurrent": min(crec)}
        t["E"] = min(v for v in t.values() if v is not None)
        out[name] = t
    W1, B1, W2, B2, W3 = (np.asarray(ts[i], np.float64) for i in (50, 51, 52, 53, 54))
    bound1 = float((np.abs(W1).sum(0) + np.abs(B1)).max())
    bound2 = float((np.abs(W2).sum(0) * bound1 + np.abs(B2)).max())
    out["head"] = {"u1": room(np.abs(W1).max()), "u2": room(np.abs(W2).max()), "u3": room(np.abs(W3).max()),
                   "s1": room(bound1), "s2": room(bound2)}
    return out


def binding(t):
    """(the term of one layer's plan_terms entry that sets E, its distance in binades to the next candidate)."""
    c = sorted((v, k) for k, v in t.items() if k != "E" and v is not None)
    return c[0][1], c[1][0] - c[0][0]


# ---- cases that move the binding term (NOT function preserving: live oracle) ----------------------------------------------
# name -> [(layer, rows of its input kernels, shift)]: those rows x 2^-shift in both directions.  The shifts of the rec_binds
# family are the smallest that put 13 + room(U) at least REC_GAP binades below every other candidate in all four shipped
# models (tests/test_weight_cases_host.py asserts the gap, and that one binade less misses it somewhere); pow2_room leaves two
# binades of head-room, so a plan that ignored U would still fit f16 at a gap of one or two.
REC_GAP = 3
_REC = {"lstm2": [("lstm2", slice(0, 32), 8)],
        "lstm3": [("lstm3", slice(0, 128), 8), ("lstm3", slice(128, 192), 10)],
        "lstm4": [("lstm4", slice(0, 256), 6)]}
PLAN_CASES = {"lstm2_rec_binds": _REC["lstm2"], "lstm3_rec_binds": _REC["lstm3"], "lstm4_rec_binds": _REC["lstm4"],
              "all_rec_bind": _REC["lstm2"] + _REC["lstm3"] + _REC["lstm4"],
              "lstm3_in_binds": [("lstm3", slice(128, 192), 8)]}


# Which term sets E per layer, the same in all four shipped models; PLAN_BINDING: what each plan case makes of it
SHIPPED_BINDING = {"lstm2": "input", "lstm3": "signal", "lstm4": "input"}
PLAN_BINDING = {"lstm2_rec_binds": {"lstm2": "recurrent"}, "lstm3_rec_binds": {"lstm3": "recurrent"},
                "lstm4_rec_binds": {"lstm4": "recurrent"},
                "all_rec_bind": {"lstm2": "recurrent", "lstm3": "recurrent", "lstm4": "recurrent"},
                "lstm3_in_binds": {"lstm3": "input"}}


def plan_case(m, name):
    ts = _copy(m)
    for layer, rows, shift in PLAN_CASES[name]:
        for d in range(2):
            i = _LBASE[layer] + 3 * d
            ts[i][rows] = ts[i][rows] * np.float32(2.0 ** -shift)
    return ModelWeights(ts, m.T, m.n_class, f"{m.source}+{name}")


# ---- weights the engine has never seen (NOT function preserving: live oracle) ---------------------------------------------
# Every case is a seeded function of the shipped tensors of the model and of the OTHER species' model of the same number.
UNSEEN_SEED = 5150
VARIANCES = (5, 11, 21, 31, 43)
BILSTM_KERNELS = (22, 23, 25, 26, 34, 35, 37, 38, 44, 45, 47, 48)    # input and recurrent kernels of layers 2-4
RECURRENT_KERNELS = (23, 26, 35, 38, 45, 48)
_HYBRID = {"hybrid_lstm3": tuple(range(34, 44)), "hybrid_lstm4": tuple(range(44, 50)),
           "hybrid_signal": tuple(range(0, 12)) + (32, 33), "hybrid_head": tuple(range(50, 56))}
UNSEEN_CASES = list(_HYBRID) + ["mean_species", "jitter20", "prune50", "outlier", "recgain20", "bn_shift", "bn_neg_gamma",
                                "random_init"]
# The admitted (case, species): the reference ALONE shows 0 of the 256 case windows with an f32 floor above BAR / 2 (the GPU
# policy keeps max_ill = 0.01; its two windows are left for another BLAS).  A table, pinned by tests/test_weight_cases_host.py,
# not computed at test time; DESIGN.md 5 lists what is left out and its counts.  mean_species is one model: run once.
UNSEEN_ADMITTED = {"ecoli": list(UNSEEN_CASES),
                   "human": ["hybrid_signal", "hybrid_head", "jitter20", "prune50", "outlier", "random_init"]}
# the same rule with recurrent_activation="sigmoid" (floors: f32_floor_act below) for the two cases run in that variant too
SIGMOID_ADMITTED = {"all_rec_bind": ["ecoli", "human"], "outlier": ["ecoli"]}


def _glorot(rng, shape):
    rf = int(np.prod(shape[:-2]))                                    # (taps, in, out) for a convolution, else (in, out)
    lim = np.sqrt(6.0 / (rf * (shape[-2] + shape[-1])))
    return rng.uniform(-lim, lim, shape).astype(np.float32)


def unseen(m, other, name):
    ts = _copy(m)
    rng = np.random.default_rng([UNSEEN_SEED, UNSEEN_CASES.index(name), m.n_class])
    if name in _HYBRID:
        for i in _HYBRID[name]:
            ts[i] = np.array(other.tensors[i], np.float32, copy=True)
    elif name == "mean_species":
        ts = [((a + np.asarray(b, np.float32)) * np.float32(0.5)).astype(np.float32) for a, b in zip(ts, other.tensors)]
    elif name == "jitter20":
        for i in range(len(ts)):
            if i not in VARIANCES:
                ts[i] = (ts[i] * (1.0 + 0.2 * rng.standard_normal(ts[i].shape))).astype(np.float32)
    elif name == "prune50":
        for i in BILSTM_KERNELS:
            ts[i][np.abs(ts[i]) < np.median(np.abs(ts[i]))] = 0
    elif name == "outlier":
        for i in BILSTM_KERNELS:
            k = np.unravel_index(np.abs(ts[i]).argmax(), ts[i].shape)
            ts[i][k] *= np.float32(32.0)
    elif name == "recgain20":
        for i in RECURRENT_KERNELS:
            ts[i] = (ts[i] * np.float32(2.0)).astype(np.float32)
    elif name == "bn_shift":
        for b in (18, 28, 40):
            ts[b + 2] = (ts[b + 2] * np.float32(4.0)).astype(np.float32)
            ts[b + 3] = (ts[b + 3] / np.float32(16.0)).astype(np.float32)
    elif name == "bn_neg_gamma":
        for b in (2, 8, 18, 28, 40):
            ts[b][::3] *= np.float32(-1.0)
    elif name == "random_init":
        # Keras' defaults for a fresh model, Glorot-uniform recurrent kernels instead of orthogonal ones
        for i, t in enumerate(ts):
            if t.ndim >= 2:
                ts[i] = _glorot(rng, t.shape)
            else:
                ts[i] = np.zeros_like(t)
        for b in (2, 8, 18, 28, 40):
            ts[b][...] = 1                                           # gamma; beta 0, mean 0
            ts[b + 3][...] = 1                                       # variance
        for b in (14, 17, 24, 27, 36, 39, 46, 49):                   # unit_forget_bias
            H = ts[b].shape[0] // 4
            ts[b][H:2 * H] = 1
    else:
        raise ValueError(name)
    return ModelWeights(ts, m.T, m.n_class, f"{m.source}+{name}")


def f32_floor_act(m1, m2, sig, rd, p64_1, p64_2, recurrent_act="hard_sigmoid", T=11):
    """parity_policy.f32_floor for either recurrent activation: per window, the larger deviation of the C port and of
    NumPy-f32 from the fp64 arbiter."""
    from oracle import c_oracle as CO
    from oracle import nrv_oracle as O
    act = {"hard_sigmoid": 0, "sigmoid": 1}[recurrent_act]
    c1, _ = CO.predict(m1.flat(), T, 6, sig, rd, act=act, threads=8)
    c2, _ = CO.predict(m2.flat(), T, 5, sig, rd, act=act, threads=8)
    q1, q2, _, _ = O.predict_pair(m1.tensors, m2.tensors, sig, rd, np.float32, recurrent_act=recurrent_act)
    return (np.maximum(np.abs(c1 - p64_1).max(-1), np.abs(q1 - p64_1).max(-1)),
            np.maximum(np.abs(c2 - p64_2).max(-1), np.abs(q2 - p64_2).max(-1)))


def f16x2_must_not_rerun(k1, k2, sw):
    """The CPU preconditions under which the fixed scales of the f16x2 signal branch hold every value of these windows:
    |S| < 1000 (kept x 2^6 as an f16 pair), every sample below the conv1 guard's static bound, and the 400 -> 64 dense
    weights x 2^10 inside the f16 range."""
    from oracle import nrv_oracle as O
    ev = np.asarray(sw, np.float64).reshape(-1, 50)
    xmax = float(np.abs(ev).max())
    for k in (k1, k2):
        w = [np.asarray(t, np.float64) for t in k.tensors]
        if not float(np.abs(O.signal_branch(w, ev)).max()) < 1000.0:
            return False
        if not xmax < conv1_sample_bound(k):
            return False
        if not float(np.abs(k.tensors[32]).max()) * 1024.0 < 65504.0:
            return False
    return True


def extreme_windows():
    """96 extreme windows (zero signal; features x 50; samples alternating between the rails) and 160 ordinary synthetic ones
    behind them, so that the policy's 1 % of ill-conditioned windows is two windows and not none."""
    from oracle import nrv_oracle as O
    sig, rd = O.synth_windows(96, 11, seed=3)
    sig[:32] = 0.0
    rd[32:64] *= 50.0
    sig[64:] = np.where(np.arange(50) % 2 == 0, 4.8, -8.4)
    s2, r2 = O.synth_windows(160, 11, seed=4)
    return np.concatenate([sig, s2]), np.concatenate([rd, r2])
