"""Weights outside the shipped range, shared by tests/test_weight_cases_host.py and tests/test_gpu_weight_range.py (no test here).

`reparam(m, site, c)` moves a model along one of the graph's exact symmetries: a producer's output is scaled by c and the
rows of its consumer that read it by 1 / c.  BatchNorm and the linear dense layer allow it directly, the ReLU layers because
ReLU is positively homogeneous.  With c a power of two every f32 and f64 operation of the graph commutes with the scaling, so
the oracle's result does not move by one bit - what moves is every magnitude the f16x2 scale planner (nrv_api.hip upload_model)
derives its exponents from.  `lstm3_perm` renumbers the 128 hidden units of lstm3 (exact up to the summation order of its
consumers).  `degenerate(m, name)` zeroes or shrinks whole tensors: NOT function preserving, the oracle is recomputed for them.

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
