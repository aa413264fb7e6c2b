"""The definition of the full fit (nanoreviser_amd/fullfit.py, depth NRV_FIT_FULL), on the CPU:
  1. the vector's layout and length against weights.tensor_shapes; pack / unpack; params_from_model and fitted_model on the
     shipped models: the 40 fitted tensors are replaced, the 20 BatchNorm tensors keep their bytes;
  2. forward at a shipped model's tensors, on windows of a fixture read, gives the fp64 oracle's probabilities;
  3. a float64 directional finite-difference check of batch_terms per tensor block;
  4. the float64 gradient is autograd's float64 gradient to 1e-9 of each tensor's scale, in every case; T = 1 gives gU exactly zero;
  5. the condition on tests/fullfit_cases.py holds for every case; cpu_bound is finite (its value is printed next to K_RECORDED);
  6. epoch skips and counts a non-finite batch, and its update is tailfit's Adam step;
  7. signalfit.batch_terms returns its old bytes, and batch_terms_dx's data gradient is autograd's;
  8. NanoReviser_train.py --fit_depth full: accepted, lstm3 and body refused with the pinned words, and a run through the stand-in
     engine writes files weights.load_model reads, with the depth in _summary.json."""
import json
import math
import os

import numpy as np
import pytest

import fullfit_cases as fc
import signalfit_cases as sc_
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import lstm3fit as l3
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd import train_cli
from nanoreviser_amd.weights import load_model

IDS = lambda c: "T%d-m%d-n%d-%s-act%d" % c      # noqa: E731
BN_IDS = [2, 3, 4, 5, 8, 9, 10, 11, 18, 19, 20, 21, 28, 29, 30, 31, 40, 41, 42, 43]
FITTED = list(range(12, 18)) + list(range(22, 28)) + [0, 1, 6, 7, 32, 33] + list(range(34, 40)) + list(range(44, 60))
FROZEN = [i for i in range(60) if i not in FITTED]


def _frozen(model):
    return (fc.read_bn(model), fc.conv_bn(model)) + tuple(fc.bn(model))


# ---- 1. plumbing -----------------------------------------------------------------------------------------------------------
def test_layout_pack_unpack_and_fitted_model(species_models, tmp_path):
    assert FROZEN == BN_IDS and len(FITTED) == 40
    for T, C in ((1, 5), (11, 6), (32, 6)):
        th = np.arange(ff.n_params(T, C), dtype=np.float32)
        parts = ff.unpack(th, T, C)
        assert [a.shape for a in parts[:12]] == [(6, 64), (16, 64), (64,), (6, 64), (16, 64), (64,), (32, 256), (64, 256), (256,),
                                                 (32, 256), (64, 256), (256,)] and len(parts) == 41
        assert np.array_equal(ff.pack(*parts), th) and ff.n_params(T, C) == 52608 + sf.n_params(T, C) and ff.N_READ == 52608
        assert ff.N_LSTM1 == 2944 and ff.N_LSTM2 == 49664
        assert all(np.array_equal(a, b) for a, b in zip(parts[12:], sf.unpack(th[ff.N_READ:], T, C)))
        sp = fc.spans(T, C)
        assert len(sp) == 41 == len(fc.TENSORS) and all(np.array_equal(th[sp[k]], a.ravel()) for k, a in zip(fc.TENSORS, parts))
    with pytest.raises(ValueError, match="full depth"):
        ff.unpack(np.zeros(sf.n_params(11, 6)), 11, 6)
    for k, m in enumerate(species_models["ecoli"]):
        # the vector's blocks have the shapes of the weight file's tensors, in its order
        th = ff.params_from_model(m)
        parts = ff.unpack(th, m.T, m.n_class)
        assert all(a.shape == np.asarray(m.tensors[i]).shape or a.size == np.asarray(m.tensors[i]).size for i, a in zip(FITTED, parts[:40]))
        assert all(parts[j].shape == np.asarray(m.tensors[i]).shape for j, i in enumerate(FITTED[:12]))
        assert all(np.array_equal(a.ravel(), np.asarray(m.tensors[i]).ravel()) for i, a in zip(FITTED, parts[:40])) and not parts[40].any()
        assert np.array_equal(th[ff.N_READ:], sf.params_from_model(m))
        theta = fc.params(11, m.n_class, 9 + k)
        fitted = ff.fitted_model(m, theta)
        assert fitted.source.endswith("+fullfit")
        assert len(fitted.tensors) == 60 and all(np.asarray(a).shape == np.asarray(b).shape for a, b in zip(fitted.tensors, m.tensors))
        stem = str(tmp_path / f"m{k}")
        ff.write_f32(fitted, stem)
        back = load_model(stem + ".f32")
        assert all(back.tensors[i].tobytes() == m.tensors[i].tobytes() for i in BN_IDS)           # the BatchNorms keep their bytes
        for i, b in zip(FITTED, ff.unpack(theta, 11, m.n_class)[:40]):
            assert np.array_equal(back.tensors[i].ravel(), b.ravel()) and not np.array_equal(back.tensors[i], m.tensors[i]), i
        assert np.array_equal(ff.with_signal(th, theta[ff.N_READ:])[ff.N_READ:], theta[ff.N_READ:])
        assert np.array_equal(ff.with_signal(th, theta[ff.N_READ:])[:ff.N_READ], th[:ff.N_READ])
        rb = ff.read_bn(m)
        assert [a.shape for a in rb] == [(32,), (32,), (128,), (128,)] and all(a.dtype == np.float32 for a in rb)
    assert ff.adam_step is tf.adam_step and ff.FitOpts is tf.FitOpts and ff.write_f32 is tf.write_f32      # reused, not copied
    assert "moving statistics" in ff.__doc__ and "DEVIATIONS" in ff.__doc__ and "Dropout" in ff.__doc__


# ---- 2. forward ------------------------------------------------------------------------------------------------------------
def test_forward_at_a_shipped_model_gives_the_oracles_probabilities(species_models, reads):
    from oracle import nrv_oracle as O
    _, rd, _ = reads(reads.keys[0])
    rt = hs.read_tensors(rd)
    sw, fw = hs.sliding_windows(rt.sig_ev, rt.feat_ev, 11)
    sw, fw = np.ascontiguousarray(sw[100:148]), np.ascontiguousarray(fw[100:148])
    q = O.predict_pair(species_models["ecoli"][0].tensors, species_models["ecoli"][1].tensors, sw, fw, np.float64)
    for k, m in enumerate(species_models["ecoli"]):
        w = [np.asarray(t, np.float64) for t in m.tensors]
        want_x2 = O._bn(O.bilstm(O._bn(O.bilstm(fw.astype(np.float64), w[12:18], O.hard_sigmoid), *w[18:22]), w[22:28], O.hard_sigmoid),
                        *w[28:32])
        fold = []                                          # every BatchNorm in the oracle's own form: scale and shift at float64
        for base in (18, 28, 2, 8, 40):
            g, be, mu, var = w[base:base + 4]
            s = g / np.sqrt(var + l4.BN_EPS)
            fold += [s, be - mu * s]
        out = ff.forward(fw, sw.reshape(48, 11, 50), ff.params_from_model(m), fold[:4], fold[4:8], fold[8], fold[9], 11, m.n_class, 0,
                         np.float64)
        assert out[0].shape == (48, 11, 128) and np.abs(out[0] - want_x2).max() <= 1e-6 * max(1.0, np.abs(want_x2).max())
        assert np.abs(out[7] - q[k]).max() <= 1e-6, (k, np.abs(out[7] - q[k]).max())
        rb32 = ff.read_bn(m)
        assert all(np.abs(a - b).max() <= 1e-5 * max(np.abs(b).max(), 1) for a, b in zip(rb32, fold[:4]))
        p32 = ff.forward(fw, sw.reshape(48, 11, 50), ff.params_from_model(m), rb32, sf.conv_bn(m), *l4.bn_scale_shift(m), 11, m.n_class,
                         0, np.float64)[7]
        assert np.abs(p32 - q[k]).max() <= 1e-4


# ---- 3, 4. gradient --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(11, 1, 31, "plain", 0), (2, 1, 33, "plain", 0), (11, 1, 33, "plain", 1)], ids=IDS)
def test_directional_differences_agree_per_tensor_block(case):
    """For each tensor block a seeded direction v of unit length inside the block: (L(theta + h v) - L(theta - h v)) / 2h against
    g . v at float64.  L is piecewise smooth and the step 1e-6 is far inside a piece (the condition keeps every kink 8 f32
    differences, about 1e-5, away in pre-activation, and a step of 1e-6 on weights moves a pre-activation by less)."""
    T, model, n, kind, act = case
    C = fc.n_class(model)
    feat, sig, y, th = fc.rows_case(*case)
    fz = _frozen(model)
    opts = tf.default_opts(model)
    g, _ = ff.batch_terms(feat, sig, y, th, *fz, T, C, opts, act, np.float64)

    def loss(theta):
        st = ff.evaluate(feat, sig, y, theta, np.arange(n), *fz, T, C, opts, act, np.float64)[1]
        return (st.ce_sum + float(np.float32(opts.lam)) * st.center_sum) / n
    rng = np.random.default_rng(1)
    th64 = th.astype(np.float64)
    sp = fc.spans(T, C)
    for k in fc.READ_TENSORS + sc_.SIG_TENSORS + ("W3f", "U3b", "b3f", "W4b", "U4f"):
        s = sp[k]
        v = np.zeros_like(th64)
        v[s] = rng.normal(0, 1, s.stop - s.start)
        v /= np.linalg.norm(v)
        h = 1e-6
        num = (loss(th64 + h * v) - loss(th64 - h * v)) / (2 * h)
        want = float(g @ v)
        assert abs(num - want) <= 1e-5 * max(abs(want), np.linalg.norm(g[s])) + 1e-10, (k, num, want)


@pytest.mark.parametrize("case", fc.GRAD_CASES, ids=IDS)
def test_gradient_is_autograds_in_float64(case):
    T, model, n, kind, act = case
    C = fc.n_class(model)
    feat, sig, y, th = fc.rows_case(*case)
    fz = _frozen(model)
    opts = tf.default_opts(model)
    g, st = ff.batch_terms(feat, sig, y, th, *fz, T, C, opts, act, np.float64)
    gt, ce, cn, ok = fc.torch_terms(feat, sig, y, th, *fz, T, C, opts, act, np.float64)
    sp = fc.spans(T, C)
    for k in fc.TENSORS:
        scale = np.abs(gt[sp[k]]).max()
        assert np.abs(g[sp[k]] - gt[sp[k]]).max() <= 1e-9 * scale, (k, np.abs(g[sp[k]] - gt[sp[k]]).max(), scale)
        assert scale > 0 or (T == 1 and k in fc.U_TENSORS), k
    if T == 1:                                             # no step has a step before it: gU is exactly zero, at every format
        g32 = ff.batch_terms(feat, sig, y, th, *fz, T, C, opts, act, np.float32)[0]
        assert not any(g[sp[k]].any() or g32[sp[k]].any() for k in fc.U_TENSORS)
    assert st.correct == ok and abs(st.ce_sum - ce) <= 1e-9 * ce and abs(st.center_sum - cn) <= 1e-9 * cn
    # everything behind Xin is signalfit.batch_terms' gradient on the definition's own X2b
    x2 = ff.forward(feat, sig, th, *fz, T, C, act, np.float64)[0]
    gs, sts = sf.batch_terms(x2, sig, y, th[ff.N_READ:], *fz[1:], T, C, opts, act, np.float64)
    assert np.array_equal(g[ff.N_READ:], gs) and sts.correct == st.correct


# ---- 5. the cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.GRAD_CASES + [fc.CHUNK_CASE], ids=IDS)
def test_the_condition_on_the_cases_holds(case):
    c = fc.condition(*case)
    s = c["signal"]
    print(f"{case}: lstm1, lstm2: nearest kink {c['kink']}, largest f32 - f64 difference {c['diff']}, shares {c['shares']}; conv: "
          f"{s['conv_kink']}, {s['conv_diff']}, open {s['conv_shares']}; lstm3, lstm4: {s['kink']}, {s['diff']}, {s['shares']}")
    assert c["sides_ok"] and c["same"], case               # the three evaluations agree on every side: all CHUNK_CASE is asked
    assert all(0 < v < 1 for v in s["conv_shares"]), c
    if case != fc.CHUNK_CASE:
        assert c["ok"] and all(k >= 8 * d for k, d in zip(s["conv_kink"], s["conv_diff"])), c
        if case[4] == 0:
            for part in (c, s):
                assert all(k >= 8 * d for k, d in zip(part["kink"], part["diff"])), c
                assert all(v > 0 for sh in part["shares"] for v in sh), c
            assert c["same_clip"]
    feat, sig, y, th = fc.rows_case(*case)
    assert np.all(th != 0) and feat.shape == (case[2], case[0], 6) and sig.shape == (case[2], case[0], 50)
    assert feat.dtype == sig.dtype == th.dtype == np.float32
    if case[3] == "zeros":
        assert not sig[0].any() and not feat[0].any() and sig[1].any() and feat[1].any() and not feat[3].any()
    if case[3] == "edges":
        assert not sig[:, :, 1:49].any() and sig[:, :, 0].all() and sig[:, :, 49].all()
    if case[3] == "absent":
        assert not (y == 2).any()


def test_the_cases_are_the_listed_ones_and_none_is_the_shipped_model(species_models):
    want = [(11, 0, 1), (11, 1, 31), (11, 0, 32), (11, 1, 33), (1, 0, 33), (2, 1, 33), (13, 0, 33), (13, 1, 31), (32, 0, 33), (11, 0, 33),
            (11, 1, 33), (11, 0, 96), (11, 0, fc.LARGE_ROWS)]
    assert [c[:3] for c in fc.GRAD_CASES] == want and fc.CHUNK_CASE == (2, 0, 4130, "plain", 1)
    assert fc.LARGE_ROWS in (160, 128, 96, 64) and fc.GRAD_CASES[-1][3:] == ("plain", 0)
    assert all(k in fc.GRAD_CASES for k in fc.SEEDS)
    m = species_models["ecoli"][0]
    assert not np.array_equal(fc.params(11, 6, 5)[:ff.N_READ], ff.params_from_model(m)[:ff.N_READ])


def test_cpu_bound_of_the_device_grade_is_finite():
    K, worst = fc.cpu_bound(fc.GRAD_CASES[:6])
    print(f"full depth, six cases: gradient bound sized on the CPU: K = {K:.4g} (worst restatement grade {worst:.4g}); recorded over "
          f"every case on the machine of the seed search: {fc.K_RECORDED}")
    assert K == 2 * worst and math.isfinite(K) and K >= 2.0
    assert math.isfinite(fc.K_RECORDED) and fc.K_RECORDED >= 2.0


# ---- 6. epoch --------------------------------------------------------------------------------------------------------------
def test_epoch_skips_a_nonfinite_batch_and_steps_by_tailfits_adam():
    T, model, C, n = 11, 1, 5, 76
    feat, sig, y, th = fc.rows_case(T, model, 33, "plain", 0)
    fz = _frozen(model)
    feat = np.concatenate([feat, feat[:10] * 0.5, feat])[:n]
    sig = np.concatenate([sig, sig[:10] * 0.5, sig])[:n]
    y = np.concatenate([y, y[:10], y])[:n]
    opts = tf.default_opts(model, B=32)
    fn = feat.copy()
    fn[40, 3, 2] = np.inf                                  # lands in the second batch of 32
    s = tf.FitState(th.astype(np.float32))
    st = ff.epoch(fn, sig, y, s, np.arange(n), *fz, T, C, opts, 0, np.float32)
    assert (st.rows, st.steps, st.nonfinite, s.t) == (44, 2, 1, 2) and np.isfinite(s.theta).all()
    r = tf.FitState(th.astype(np.float32))
    ff.epoch(fn, sig, y, r, np.concatenate([np.arange(32), np.arange(64, 76)]), *fz, T, C, opts, 0, np.float32)
    assert np.array_equal(s.theta, r.theta) and r.t == 2 and not np.array_equal(s.theta[:ff.N_READ], th[:ff.N_READ])
    # one batch: the update is tailfit.adam_step on batch_terms' gradient
    one = tf.FitState(th.astype(np.float32))
    ff.epoch(feat, sig, y, one, np.arange(32), *fz, T, C, opts, 0, np.float32)
    g = ff.batch_terms(feat[:32], sig[:32], y[:32], th, *fz, T, C, opts, 0, np.float32)[0]
    want = tf.adam_step(th.astype(np.float32), np.zeros_like(th), np.zeros_like(th), g, opts, 1, np.dtype(np.float32))[0]
    assert one.t == 1 and np.array_equal(one.theta, want)
    p, se = ff.evaluate(feat, sig, y, th, np.arange(n), *fz, T, C, opts, 0, np.float32)
    assert p.shape == (n, C) and se.rows == n and np.allclose(p.sum(1), 1, atol=1e-6)


# ---- 7. signalfit keeps its bytes ------------------------------------------------------------------------------------------
def _signal_batch_terms_before(x2, sig, y, theta, cb, sc, sh, T, C, opts, act, dtype):
    """signalfit.batch_terms as it stood before batch_terms_dx was split off it."""
    from nanoreviser_amd.signalfit import N_CH, N_FLAT, N_S, N_SIG_IN, N_SIGNAL, branch, lstm3fit, unpack, xin
    dt = np.dtype(dtype)
    theta = np.asarray(theta)
    k = branch(sig, theta, cb, T, C, dt)
    n = k["sig"].shape[0]
    g3, st, dXin = lstm3fit.batch_terms_dx(xin(x2, k["S"], T, dt), y, theta[N_SIGNAL:], sc, sh, T, C, opts, act, dt)
    w1, b1, w2, b2, Ws, bs = [a.astype(dt) for a in unpack(theta, T, C)[:6]]
    s1, s2 = np.asarray(cb[0]).astype(dt), np.asarray(cb[2]).astype(dt)
    dS = dXin[..., 128:]
    gWs = k["F"].reshape(-1, N_FLAT).T @ dS.reshape(-1, N_S)
    gbs = dS.reshape(-1, N_S).sum(axis=0)
    dF = (dS @ Ws.T).reshape(n, T, N_SIG_IN, N_CH)
    da2 = np.where(k["a2"] > 0, dF * s2, dt.type(0))
    cp = np.pad(k["c1"], ((0, 0), (0, 0), (1, 1), (0, 0)))
    dp = np.pad(da2, ((0, 0), (0, 0), (1, 1), (0, 0)))
    gw2 = np.stack([np.einsum("ntpc,ntpo->co", cp[..., kk:kk + N_SIG_IN, :], da2) for kk in range(3)])
    gb2 = da2.sum(axis=(0, 1, 2))
    dc1 = sum(dp[..., 2 - kk:2 - kk + N_SIG_IN, :] @ w2[kk].T for kk in range(3))
    da1 = np.where(k["a1"] > 0, dc1 * s1, dt.type(0))
    sp = np.pad(k["sig"], ((0, 0), (0, 0), (1, 1)))
    gw1 = np.stack([np.einsum("ntp,ntpo->o", sp[..., kk:kk + N_SIG_IN], da1) for kk in range(3)])
    gb1 = da1.sum(axis=(0, 1, 2))
    g = np.concatenate([a.ravel() for a in (gw1, gb1, gw2, gb2, gWs, gbs)]) / dt.type(n)
    return np.concatenate([g.astype(dt), g3]), st


@pytest.mark.parametrize("case", [(11, 1, 33, "plain", 0), (1, 0, 33, "plain", 0), (11, 1, 33, "plain", 1)], ids=IDS)
def test_signalfit_batch_terms_keeps_its_bytes_and_dx_is_autograds(case):
    import torch
    T, model, n, kind, act = case
    C = sc_.n_class(model)
    x2, sig, y, th = sc_.rows_case(*case)
    cb, (sc, sh) = sc_.conv_bn(model), sc_.bn(model)
    opts = tf.default_opts(model)
    for dt in (np.float64, np.float32):
        g, st = sf.batch_terms(x2, sig, y, th, cb, sc, sh, T, C, opts, act, dt)
        g2, st2, dx2 = sf.batch_terms_dx(x2, sig, y, th, cb, sc, sh, T, C, opts, act, dt)
        assert g.tobytes() == g2.tobytes() and st == st2 and dx2.shape == (n, T, 128) and dx2.dtype == dt
        g0, st0 = _signal_batch_terms_before(x2, sig, y, th, cb, sc, sh, T, C, opts, act, dt)
        assert g.tobytes() == g0.tobytes() and st == st0                                       # its old bytes
    # autograd's derivative of the batch's SUM of row losses with respect to x2
    tdt = torch.float64
    tht = torch.tensor(th.astype(np.float64))
    x = torch.tensor(x2.astype(np.float64), requires_grad=True)
    S, _, _ = sc_._torch_branch(torch.tensor(sig.astype(np.float64)), tht, [torch.tensor(np.asarray(a, np.float64)) for a in cb], T)
    x4, _, _, thh = sc_.l3c._torch_forward(torch.cat([x, S], dim=2), tht[sf.N_SIGNAL:], torch.tensor(sc.astype(np.float64)),
                                           torch.tensor(sh.astype(np.float64)), T, C, act)
    W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce = sc_.hc._split(thh, T, C, lambda a, s: a.reshape(s))
    yt = torch.tensor(np.asarray(y, np.int64))
    cw = torch.tensor(opts.cw6(), dtype=tdt)[yt]
    mo = torch.relu(torch.relu(torch.relu(x4 @ W1 + b1) @ W2 + b2) @ Wm + bm)
    f = torch.relu(mo.reshape(-1, 6 * T) @ Wf + bf)
    logp = torch.log_softmax(f @ Wo + bo, dim=1)
    L = (cw * -logp[torch.arange(n), yt]).sum() + float(np.float32(opts.lam)) * ((f - Ce[yt]) ** 2).sum()
    L.backward()
    want = x.grad.numpy()
    dx2 = sf.batch_terms_dx(x2, sig, y, th, cb, sc, sh, T, C, opts, act, np.float64)[2]
    assert np.abs(dx2 - want).max() <= 1e-9 * np.abs(want).max() and np.abs(want).max() > 0


# ---- 8. command line -------------------------------------------------------------------------------------------------------
def test_fit_depth_full_argument_checks(tmp_path, capsys):
    d = str(tmp_path)
    base = ["-d", d, "-S", "ecoli", "-M", str(tmp_path / "out"), "--labels_from", d]
    boom = lambda *a: pytest.fail("no engine may be made for a refused command line")        # noqa: E731
    for bad in ("lstm3", "body"):
        assert train_cli.main(base + ["--fit_depth", bad], reviser_factory=boom) == 2
        err = capsys.readouterr().err
        assert all(w in err for w in ("--fit_depth", "tail or head", "lstm4", repr(bad), "signal", "full")), err
    for init in ("transfer", "fresh", "fresh_head"):
        assert train_cli.check_args(train_cli.get_args(base + ["--fit_depth", "full", "--fit_init", init])) is None
    assert "--fit_depth full" in train_cli.__doc__ and "--fit_depth lstm3 is not" in train_cli.__doc__
    assert train_cli._DEPTHS["full"] is ff


def test_train_cli_at_full_depth_writes_a_model_directory(tmp_path, monkeypatch, species_models):
    import __graft_entry__ as g
    from fullfit_engine import FullEcho
    from nanoreviser_amd import hostlib
    from test_accuracy_host import _clean_env, _many
    from test_infix_host import _memoised as _memoised_infix
    from test_score_cli_host import _labels_dir
    g.build_host()
    _clean_env(monkeypatch)
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib, "_lib", None)
    assert hostlib.load() is not None
    _memoised_infix(monkeypatch)
    src = _many(tmp_path, 2)
    names = sorted(os.listdir(src))
    lab = _labels_dir(tmp_path, names, (), ())
    made = []

    def factory(a, m1, m2):
        made.append(FullEcho(m1.T, (m1, m2)))
        return made[-1]
    m1, m2 = species_models["ecoli"]
    T = m1.T
    out = str(tmp_path / "model")
    argv = ["-d", src, "-S", "ecoli", "-M", out, "-e", "1", "-b", "2048", "--labels_from", lab, "--validation_split", "0.1",
            "--seed", "7", "--fit_depth", "full", "--model_type", "model2"]
    assert train_cli.main(argv, reviser_factory=factory) == 0
    eng = made[0]
    assert eng.closed and eng.depth_calls == [32]
    n = eng.fit_count()
    n_train, n_val = tf.val_split(n, 0.1)
    stem = train_cli.stem(out, "ecoli", 2)
    back = load_model(stem + ".f32")
    assert back.T == T and all(back.tensors[i].tobytes() == m2.tensors[i].tobytes() for i in BN_IDS)
    theta, t = eng.fit_params(1)
    assert theta.size == ff.n_params(T, 5) and t == math.ceil(n_train / 2048)
    for i, b in zip(FITTED, ff.unpack(theta, T, 5)[:40]):
        assert np.array_equal(back.tensors[i].ravel(), b.ravel()) and not np.array_equal(back.tensors[i], m2.tensors[i]), i
    assert np.array_equal(np.fromfile(stem + "_centers.f32", "<f4"), theta[-80:])
    s = json.load(open(stem + "_summary.json"))
    assert s["options"]["fit_depth"] == "full" and s["options"]["init"] == "transfer" and s["rows"] == n and s["val_rows"] == n_val
    # the start: the four LSTMs and the signal branch are always the model's own; --fit_init acts on the layers behind lstm4
    base = ["-d", src, "--labels_from", lab, "--fit_depth", "full", "--seed", "7"]
    own = ff.params_from_model(m1)
    front = ff.N_READ + sf.N_SIGNAL + l3.N_LSTM3 + l4.N_LSTM4
    th, how = train_cli._start(train_cli.get_args(base), 0, m1, T)
    assert how == "transfer" and np.array_equal(th, own)
    th, how = train_cli._start(train_cli.get_args(base + ["--fit_init", "fresh"]), 0, m1, T)
    assert how == "fresh" and np.array_equal(th[:front], own[:front]) and np.array_equal(th[-tf.n_params(T, 6):], tf.fresh_params(T, 6, 7))
    th, how = train_cli._start(train_cli.get_args(base + ["--model2_train_dir", stem + ".f32"]), 1, m2, T)
    assert how == "continued" and np.array_equal(th, theta)
