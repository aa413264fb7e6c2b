"""The definition of the lstm3 fit (nanoreviser_amd/lstm3fit.py, depth NRV_FIT_LSTM3), on the CPU:
  1. at float64 the definition's H3 is oracle.nrv_oracle.bilstm's on the same tensors, and what lies behind it lstm4fit.forward;
  2. forward at a shipped model's tensors, on windows of a fixture read with Xin formed from the oracle's own pieces, gives the
     oracle's probabilities;
  3. the float64 gradient is autograd's float64 gradient to 1e-9 of each tensor's scale, in every case;
  4. central differences on a handful of coordinates per tensor agree;
  5. the condition on tests/lstm3fit_cases.py holds;
  6. cpu_bound is finite (its value is printed);
  7. pack / unpack, the vector's length, fitted_model;
  8. lstm4fit.batch_terms_dx is batch_terms bit for bit in what they share, and its dXb is autograd's;
  9. epoch skips and counts a non-finite batch.
The training command line does not offer this depth yet (Left out), so nothing of it is tested here."""
import math

import numpy as np
import pytest

import lstm3fit_cases as lc
import lstm4fit_cases as l4c
from nanoreviser_amd import headfit as hf
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import lstm3fit as lf
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.weights import load_model

IDS = lambda c: "T%d-m%d-n%d-%s-act%d" % c      # noqa: E731
SMALL = [c for c in lc.GRAD_CASES if c[2] <= 96]
FITTED = list(range(34, 40)) + list(range(44, 60))
FROZEN = list(range(0, 34)) + list(range(40, 44))


# ---- 1, 2. forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(11, 1, 33, "plain", 0), (13, 1, 31, "zeros", 0), (11, 1, 33, "plain", 1), (1, 0, 33, "plain", 0)], ids=IDS)
def test_forward_is_the_oracles_bilstm_and_lstm4fits_forward(case):
    from oracle import nrv_oracle as O
    T, model, n, kind, act = case
    C = lc.n_class(model)
    X, y, th = lc.rows_case(*case)
    sc, sh = lc.bn(model)
    parts = [a.astype(np.float64) for a in lf.unpack(th, T, C)[:6]]
    want = O.bilstm(X.astype(np.float64), parts, O.hard_sigmoid if act == 0 else O.sigmoid)
    h3, xb4, x4, mo, f, p = lf.forward(X, th, sc, sh, T, C, act, np.float64)
    assert h3.shape == (n, T, 256) and np.abs(h3 - want).max() <= 1e-12
    assert np.array_equal(xb4, h3 * sc.astype(np.float64) + sh.astype(np.float64))
    x42, mo2, f2, p2 = l4.forward(xb4, th[lf.N_LSTM3:], T, C, act, np.float64)
    assert np.array_equal(x4, x42) and np.array_equal(mo, mo2) and np.array_equal(f, f2) and np.array_equal(p, p2)
    # float32: one multiply and one add, each rounded
    h32 = lf.lstm(X, th, T, C, act, np.float32)[1]
    b32 = lf.bn(h32, sc, sh, np.float32)
    assert b32.dtype == np.float32 and np.array_equal(b32, (h32 * sc).astype(np.float32) + sh)


def test_forward_at_a_shipped_model_gives_the_oracles_probabilities(species_models, reads):
    from oracle import nrv_oracle as O
    _, rd, _ = reads(reads.keys[0])
    rt = hs.read_tensors(rd)
    sw, fw = hs.sliding_windows(rt.sig_ev, rt.feat_ev, 11)
    sw, fw = np.ascontiguousarray(sw[100:148]), np.ascontiguousarray(fw[100:148])
    q = O.predict_pair(species_models["ecoli"][0].tensors, species_models["ecoli"][1].tensors, sw, fw, np.float64)
    for k, m in enumerate(species_models["ecoli"]):
        w = [np.asarray(t, np.float64) for t in m.tensors]
        s = O.signal_branch(w, sw.astype(np.float64).reshape(-1, 50)).reshape(48, 11, 64)
        r = O._bn(O.bilstm(fw.astype(np.float64), w[12:18], O.hard_sigmoid), *w[18:22])
        r = O._bn(O.bilstm(r, w[22:28], O.hard_sigmoid), *w[28:32])
        xin = np.concatenate([r, s], axis=-1)
        # (the BatchNorm in the oracle's own form, not folded: sc and sh at float64)
        g, be, mu, var = w[40:44]
        sc = g / np.sqrt(var + l4.BN_EPS)
        sh = be - mu * sc
        p = lf.forward(xin, lf.params_from_model(m), sc, sh, 11, m.n_class, 0, np.float64)[5]
        assert np.abs(p - q[k]).max() <= 1e-6, (k, np.abs(p - q[k]).max())      # (the parameters are f32 both ways)
        sc32, sh32 = l4.bn_scale_shift(m)
        assert np.abs(sc32 - sc).max() <= 1e-5 * np.abs(sc).max() and np.abs(sh32 - sh).max() <= 1e-5
        p32 = lf.forward(xin, lf.params_from_model(m), sc32, sh32, 11, m.n_class, 0, np.float64)[5]
        assert np.abs(p32 - q[k]).max() <= 1e-5


# ---- 3 .. 6. gradient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.GRAD_CASES, ids=IDS)
def test_gradient_is_autograds_in_float64(case):
    T, model, n, kind, act = case
    C = lc.n_class(model)
    X, y, th = lc.rows_case(*case)
    sc, sh = lc.bn(model)
    opts = tf.default_opts(model)
    g, st = lf.batch_terms(X, y, th, sc, sh, T, C, opts, act, np.float64)
    gt, ce, cn, ok = lc.torch_terms(X, y, th, sc, sh, T, C, opts, act, np.float64)
    sp = lc.spans(T, C)
    assert len(lc.TENSORS) == 23
    for k in lc.TENSORS:
        scale = np.abs(gt[sp[k]]).max()
        assert np.abs(g[sp[k]] - gt[sp[k]]).max() <= 1e-9 * scale, (k, np.abs(g[sp[k]] - gt[sp[k]]).max(), scale)
        assert scale > 0 or (T == 1 and k in ("U3f", "U3b", "U4f", "U4b")), k
    if T == 1:
        assert not any(g[sp[k]].any() for k in ("U3f", "U3b", "U4f", "U4b"))
    assert st.correct == ok and abs(st.ce_sum - ce) <= 1e-9 * ce and abs(st.center_sum - cn) <= 1e-9 * cn
    # everything behind lstm3 is lstm4fit.batch_terms' gradient on the definition's own Xb4
    xb4 = lf.forward(X, th, sc, sh, T, C, act, np.float64)[1]
    g4, st4 = l4.batch_terms(xb4, y, th[lf.N_LSTM3:], T, C, opts, act, np.float64)
    assert np.array_equal(g[lf.N_LSTM3:], g4) and st4.correct == st.correct


@pytest.mark.parametrize("case", [(11, 1, 31, "plain", 0), (2, 1, 33, "plain", 0), (11, 1, 33, "plain", 1)], ids=IDS)
def test_central_differences_agree(case):
    T, model, n, kind, act = case
    C = lc.n_class(model)
    X, y, th = lc.rows_case(*case)
    sc, sh = lc.bn(model)
    opts = tf.default_opts(model)
    g, _ = lf.batch_terms(X, y, th, sc, sh, T, C, opts, act, np.float64)

    def loss(theta):
        st = lf.evaluate(X, y, theta, np.arange(n), sc, sh, T, C, opts, act, np.float64)[1]
        return (st.ce_sum + float(np.float32(opts.lam)) * st.center_sum) / n
    rng = np.random.default_rng(1)
    th64 = th.astype(np.float64)
    for k, s in lc.spans(T, C).items():
        big = np.argsort(-np.abs(g[s]))[:64]               # coordinates whose derivative is not lost in the difference's rounding
        for j in rng.choice(big, 3, replace=False):
            i, h = s.start + int(j), 1e-6
            a, b = th64.copy(), th64.copy()
            a[i] += h
            b[i] -= h
            num = (loss(a) - loss(b)) / (2 * h)
            assert abs(num - g[i]) <= 1e-5 * max(abs(g[i]), np.abs(g[s]).max()), (k, int(j), num, g[i])


@pytest.mark.parametrize("case", lc.GRAD_CASES + [lc.CHUNK_CASE, (11, 0, 1100, "plain", 0)], ids=IDS)
def test_the_condition_on_the_cases_holds(case):
    c = lc.condition(*case)
    print(f"{case}: nearest kink {c['kink']}, largest f32 - f64 pre-activation difference {c['diff']}, shares {c['shares']}")
    assert c["same"], case
    if case[4] == 0 and case[2] <= 512:                    # (the 1100-row set of the epoch tests is compared byte for byte, not graded)
        assert c["ok"] and all(k >= 8 * d for k, d in zip(c["kink"], c["diff"])), c
        assert len(c["shares"]) == 2 and all(v > 0 for s in c["shares"] for v in s), c         # both clips and the open side, in each layer
    X, y, th = lc.rows_case(*case)
    assert np.all(th != 0) and X.dtype == np.float32 and X.shape == (case[2], case[0], 192)
    if case[3] == "zeros":
        assert not X[0].any() and X[1].any()
    if case[3] == "absent":
        assert not (y == 2).any()


def test_cpu_bound_of_the_device_grade_is_finite():
    K, worst = lc.cpu_bound(SMALL)
    print(f"lstm3 depth, the cases of at most 96 rows: gradient bound sized on the CPU: K = {K:.4g} (worst restatement grade {worst:.4g})")
    assert K == 2 * worst and math.isfinite(K) and K >= 2.0


# ---- 7. plumbing -----------------------------------------------------------------------------------------------------------
def test_pack_unpack_and_fitted_model(species_models, tmp_path):
    for T, C in ((1, 5), (11, 6), (32, 6)):
        th = np.arange(lf.n_params(T, C), dtype=np.float32)
        parts = lf.unpack(th, T, C)
        assert [a.shape for a in parts[:6]] == [(192, 512), (128, 512), (512,)] * 2 and len(parts) == 23
        assert np.array_equal(lf.pack(*parts), th) and lf.n_params(T, C) == 328704 + l4.n_params(T, C) and lf.N_LSTM3 == 328704
        assert all(np.array_equal(a, b) for a, b in zip(parts[6:], l4.unpack(th[lf.N_LSTM3:], T, C)))
        sp = lc.spans(T, C)
        assert all(np.array_equal(th[sp[k]], a.ravel()) for k, a in zip(lc.TENSORS, parts))
    with pytest.raises(ValueError, match="lstm3 depth"):
        lf.unpack(np.zeros(l4.n_params(11, 6)), 11, 6)
    for k, m in enumerate(species_models["ecoli"]):
        th = lf.params_from_model(m)
        parts = lf.unpack(th, m.T, m.n_class)
        assert all(np.array_equal(a, m.tensors[i]) for i, a in zip(FITTED, parts[:22])) and not parts[22].any()
        assert np.array_equal(th[lf.N_LSTM3:], l4.params_from_model(m))
        theta = lc.params(11, m.n_class, 9 + k)
        fitted = lf.fitted_model(m, theta)
        assert len(fitted.tensors) == 60
        assert all(fitted.tensors[i] is m.tensors[i] or fitted.tensors[i].tobytes() == m.tensors[i].tobytes() for i in FROZEN)
        stem = str(tmp_path / f"m{k}")
        lf.write_f32(fitted, stem)
        back = load_model(stem + ".f32")
        assert all(back.tensors[i].tobytes() == m.tensors[i].tobytes() for i in FROZEN)           # 0 .. 33 and the BatchNorm 40 .. 43
        for i, b in zip(FITTED, lf.unpack(theta, 11, m.n_class)[:22]):
            assert np.array_equal(back.tensors[i], b) and not np.array_equal(back.tensors[i], m.tensors[i]), i
        assert np.array_equal(lf.with_lstm4(th, theta[lf.N_LSTM3:])[lf.N_LSTM3:], theta[lf.N_LSTM3:])
        assert np.array_equal(lf.with_lstm4(th, theta[lf.N_LSTM3:])[:lf.N_LSTM3], th[:lf.N_LSTM3])
    assert lf.adam_step is tf.adam_step and lf.FitOpts is tf.FitOpts and lf.write_f32 is tf.write_f32      # reused, not copied
    assert lf.bn_scale_shift is l4.bn_scale_shift
    assert "moving statistics" in lf.__doc__ and "DEVIATION" in lf.__doc__


# ---- 8. the data gradient out of lstm4 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(11, 1, 33, "plain", 0), (1, 0, 33, "plain", 0), (11, 1, 33, "plain", 1)], ids=IDS)
def test_lstm4fit_batch_terms_dx(case):
    import torch
    T, model, n, kind, act = case
    C = l4c.n_class(model)
    X, y, th = l4c.rows_case(*case)
    opts = tf.default_opts(model)
    for dt in (np.float64, np.float32):
        g, st = l4.batch_terms(X, y, th, T, C, opts, act, dt)
        g2, st2, dX = l4.batch_terms_dx(X, y, th, T, C, opts, act, dt)
        assert g.tobytes() == g2.tobytes() and st == st2 and dX.shape == (n, T, 256) and dX.dtype == dt
    # autograd's derivative of the batch's SUM of row losses with respect to Xb
    tht = torch.tensor(th.astype(np.float64))
    x = torch.tensor(X.astype(np.float64), requires_grad=True)
    lstm, thh = l4c._torch_split(tht, T, C)
    W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce = l4c.hc._split(thh, T, C, lambda a, s: a.reshape(s))
    x4 = l4c._torch_lstm(x, lstm, T, act)[0]
    yt = torch.tensor(np.asarray(y, np.int64))
    cw = torch.tensor(opts.cw6(), dtype=torch.float64)[yt]
    mo = torch.relu(torch.relu(torch.relu(x4 @ W1 + b1) @ W2 + b2) @ Wm + bm)
    f = torch.relu(mo.reshape(-1, 6 * T) @ Wf + bf)
    logp = torch.log_softmax(f @ Wo + bo, dim=1)
    L = (cw * -logp[torch.arange(n), yt]).sum() + float(np.float32(opts.lam)) * ((f - Ce[yt]) ** 2).sum()
    L.backward()
    want = x.grad.numpy()
    dX = l4.batch_terms_dx(X, y, th, T, C, opts, act, np.float64)[2]
    assert np.abs(dX - want).max() <= 1e-9 * np.abs(want).max() and np.abs(want).max() > 0


# ---- 9. epoch --------------------------------------------------------------------------------------------------------------
def test_epoch_skips_and_counts_a_nonfinite_batch():
    T, model, C, n = 11, 1, 5, 76
    X, y, th = lc.rows_case(T, model, 33, "plain", 0)
    sc, sh = lc.bn(model)
    X = np.concatenate([X, X[:10] * 0.5, X])[:n]
    y = np.concatenate([y, y[:10], y])[:n]
    opts = tf.default_opts(model, B=32)
    order = np.random.default_rng(1).permutation(n)
    s = tf.FitState(th.astype(np.float64))
    st = lf.epoch(X, y, s, order, sc, sh, T, C, opts, 0, np.float64)
    assert (st.rows, st.steps, st.nonfinite, s.t) == (76, 3, 0, 3)
    r = tf.FitState(th.astype(np.float64))
    for t, (lo, hi) in enumerate(((0, 32), (32, 64), (64, 76)), 1):
        g, _ = lf.batch_terms(X[order[lo:hi]], y[order[lo:hi]], r.theta, sc, sh, T, C, opts, 0, np.float64)
        r.theta, r.m, r.v = tf.adam_step(r.theta, r.m, r.v, g, opts, t, np.float64)
    assert np.array_equal(s.theta, r.theta) and not np.array_equal(s.theta[:lf.N_LSTM3], th[:lf.N_LSTM3])
    Xn = X.copy()
    Xn[40, 3, 7] = np.inf                                  # lands in the second batch of 32
    for dtype in (np.float64, np.float32):
        s = tf.FitState(th.astype(dtype))
        st = lf.epoch(Xn, y, s, np.arange(n), sc, sh, T, C, opts, 0, dtype)
        assert (st.rows, st.steps, st.nonfinite, s.t) == (44, 2, 1, 2) and np.isfinite(s.theta).all()
        r = tf.FitState(th.astype(dtype))
        lf.epoch(Xn, y, r, np.concatenate([np.arange(32), np.arange(64, 76)]), sc, sh, T, C, opts, 0, dtype)
        assert np.array_equal(s.theta, r.theta) and r.t == 2
    p, se = lf.evaluate(X, y, th, np.arange(n), sc, sh, T, C, opts, 0, np.float32)
    assert p.shape == (n, C) and se.rows == n and np.allclose(p.sum(1), 1, atol=1e-6)
