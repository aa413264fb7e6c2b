"""The definition of the signal fit (nanoreviser_amd/signalfit.py, depth NRV_FIT_SIGNAL), on the CPU:
  1. forward at a shipped model's tensors, on windows of a fixture read, gives oracle.nrv_oracle.signal_branch's S and the
     oracle's probabilities to 1e-6 at float64;
  2. the float64 gradient is autograd's float64 gradient to 1e-9 of each tensor's scale, in every case;
  3. central differences on a few coordinates per new tensor agree;
  4. the condition on tests/signalfit_cases.py holds;
  5. cpu_bound is finite (its value is printed);
  6. lstm3fit.batch_terms returns its old bytes, and batch_terms_dx's dXin is autograd's;
  7. pack / unpack, the vector's length, fitted_model: exactly the listed tensors change;
  8. epoch skips and counts a non-finite batch;
  9. NanoReviser_train.py --fit_depth signal: accepted, lstm3 refused with the pinned words, and a run through the stand-in engine
     writes files weights.load_model reads, with the depth in _summary.json."""
import json
import math
import os

import numpy as np
import pytest

import lstm3fit_cases as l3c
import signalfit_cases as sc_
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import lstm3fit as l3
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd import train_cli
from nanoreviser_amd.weights import load_model

IDS = lambda c: "T%d-m%d-n%d-%s-act%d" % c      # noqa: E731
SMALL = [c for c in sc_.GRAD_CASES if c[2] <= 96]
SIG_IDS = [0, 1, 6, 7, 32, 33]
FITTED = SIG_IDS + list(range(34, 40)) + list(range(44, 60))
FROZEN = [i for i in range(60) if i not in FITTED]


# ---- 1. forward ------------------------------------------------------------------------------------------------------------
def test_forward_at_a_shipped_model_gives_the_oracles_s_and_probabilities(species_models, reads):
    from oracle import nrv_oracle as O
    _, rd, _ = reads(reads.keys[0])
    rt = hs.read_tensors(rd)
    sw, fw = hs.sliding_windows(rt.sig_ev, rt.feat_ev, 11)
    sw, fw = np.ascontiguousarray(sw[100:148]), np.ascontiguousarray(fw[100:148])
    q = O.predict_pair(species_models["ecoli"][0].tensors, species_models["ecoli"][1].tensors, sw, fw, np.float64)
    for k, m in enumerate(species_models["ecoli"]):
        w = [np.asarray(t, np.float64) for t in m.tensors]
        want_s = O.signal_branch(w, sw.astype(np.float64).reshape(-1, 50)).reshape(48, 11, 64)
        r = O._bn(O.bilstm(fw.astype(np.float64), w[12:18], O.hard_sigmoid), *w[18:22])
        x2 = O._bn(O.bilstm(r, w[22:28], O.hard_sigmoid), *w[28:32])
        # (the BatchNorms in the oracle's own form, not folded: every scale and shift at float64)
        cb = []
        for base in (2, 8):
            g, be, mu, var = w[base:base + 4]
            s = g / np.sqrt(var + l4.BN_EPS)
            cb += [s, be - mu * s]
        g, be, mu, var = w[40:44]
        sc = g / np.sqrt(var + l4.BN_EPS)
        sh = be - mu * sc
        out = sf.forward(x2, sw.reshape(48, 11, 50), sf.params_from_model(m), cb, sc, sh, 11, m.n_class, 0, np.float64)
        assert out[0].shape == (48, 11, 64) and np.abs(out[0] - want_s).max() <= 1e-6, np.abs(out[0] - want_s).max()
        assert np.abs(out[6] - q[k]).max() <= 1e-6, (k, np.abs(out[6] - q[k]).max())
        cb32 = sf.conv_bn(m)
        assert all(a.dtype == np.float32 and np.abs(a - b).max() <= 1e-5 * max(np.abs(b).max(), 1) for a, b in zip(cb32, cb))
        p32 = sf.forward(x2, sw.reshape(48, 11, 50), sf.params_from_model(m), cb32, *l4.bn_scale_shift(m), 11, m.n_class, 0, np.float64)[6]
        assert np.abs(p32 - q[k]).max() <= 1e-5


# ---- 2 .. 5. gradient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc_.GRAD_CASES, ids=IDS)
def test_gradient_is_autograds_in_float64(case):
    T, model, n, kind, act = case
    C = sc_.n_class(model)
    x2, sig, y, th = sc_.rows_case(*case)
    cb, (sc, sh) = sc_.conv_bn(model), sc_.bn(model)
    opts = tf.default_opts(model)
    g, st = sf.batch_terms(x2, sig, y, th, cb, sc, sh, T, C, opts, act, np.float64)
    gt, ce, cn, ok = sc_.torch_terms(x2, sig, y, th, cb, sc, sh, T, C, opts, act, np.float64)
    sp = sc_.spans(T, C)
    assert len(sc_.TENSORS) == 29 == len(sp)
    for k in sc_.TENSORS:
        scale = np.abs(gt[sp[k]]).max()
        assert np.abs(g[sp[k]] - gt[sp[k]]).max() <= 1e-9 * scale, (k, np.abs(g[sp[k]] - gt[sp[k]]).max(), scale)
        assert scale > 0 or (T == 1 and k in ("U3f", "U3b", "U4f", "U4b")), k
    if T == 1:
        assert not any(g[sp[k]].any() for k in ("U3f", "U3b", "U4f", "U4b"))
    assert st.correct == ok and abs(st.ce_sum - ce) <= 1e-9 * ce and abs(st.center_sum - cn) <= 1e-9 * cn
    # everything behind Xin is lstm3fit.batch_terms' gradient on the definition's own Xin
    S = sf.forward(x2, sig, th, cb, sc, sh, T, C, act, np.float64)[0]
    g3, st3 = l3.batch_terms(sf.xin(x2, S, T), y, th[sf.N_SIGNAL:], sc, sh, T, C, opts, act, np.float64)
    assert np.array_equal(g[sf.N_SIGNAL:], g3) and st3.correct == st.correct


@pytest.mark.parametrize("case", [(11, 1, 31, "plain", 0), (11, 0, 33, "edges", 0), (13, 1, 31, "zeros", 0)], ids=IDS)
def test_central_differences_agree(case):
    T, model, n, kind, act = case
    C = sc_.n_class(model)
    x2, sig, y, th = sc_.rows_case(*case)
    cb, (sc, sh) = sc_.conv_bn(model), sc_.bn(model)
    opts = tf.default_opts(model)
    g, _ = sf.batch_terms(x2, sig, y, th, cb, sc, sh, T, C, opts, act, np.float64)

    def loss(theta):
        st = sf.evaluate(x2, sig, y, theta, np.arange(n), cb, sc, sh, T, C, opts, act, np.float64)[1]
        return (st.ce_sum + float(np.float32(opts.lam)) * st.center_sum) / n
    rng = np.random.default_rng(1)
    th64 = th.astype(np.float64)
    sp = sc_.spans(T, C)
    for k in sc_.SIG_TENSORS:
        s = sp[k]
        big = np.argsort(-np.abs(g[s]))[:8]                # coordinates whose derivative is not lost in the difference's rounding
        for j in rng.choice(big, 3, replace=False):
            i, h = s.start + int(j), 1e-6
            a, b = th64.copy(), th64.copy()
            a[i] += h
            b[i] -= h
            num = (loss(a) - loss(b)) / (2 * h)
            assert abs(num - g[i]) <= 1e-5 * max(abs(g[i]), np.abs(g[s]).max()), (k, int(j), num, g[i])


@pytest.mark.parametrize("case", sc_.GRAD_CASES + [sc_.CHUNK_CASE], ids=IDS)
def test_the_condition_on_the_cases_holds(case):
    c = sc_.condition(*case)
    print(f"{case}: conv: nearest kink {c['conv_kink']}, largest f32 - f64 difference {c['conv_diff']}, open {c['conv_shares']}; "
          f"gates: nearest kink {c['kink']}, difference {c['diff']}, shares {c['shares']}")
    assert c["same"], case
    assert all(0 < v < 1 for v in c["conv_shares"]), c     # both sides of both ReLUs
    if case[2] <= 512:                                     # (the chunk case: see SEEDS.  The 1100-row set of the device's epoch tests is
                                                           # compared byte for byte between device runs, never graded: it is not a case)
        assert c["ok"] and all(k >= 8 * d for k, d in zip(c["conv_kink"], c["conv_diff"])), c
        if case[4] == 0:
            assert all(k >= 8 * d for k, d in zip(c["kink"], c["diff"])) and all(v > 0 for s in c["shares"] for v in s), c
    x2, sig, y, th = sc_.rows_case(*case)
    assert np.all(th != 0) and x2.shape == (case[2], case[0], 128) and sig.shape == (case[2], case[0], 50) and sig.dtype == np.float32
    if case[3] == "zeros":
        assert not sig[0].any() and not x2[0].any() and sig[1].any()
        k = sf.branch(sig[:1], th, sc_.conv_bn(case[1]), case[0], sc_.n_class(case[1]))
        assert np.array_equal(k["z1"][0, 0, 0] > 0, th[24:32] > 0)       # the sides of conv1's ReLUs are its biases' signs
    if case[3] == "edges":
        assert not sig[:, :, 1:49].any() and sig[:, :, 0].all() and sig[:, :, 49].all()
    if case[3] == "absent":
        assert not (y == 2).any()


def test_cpu_bound_of_the_device_grade_is_finite():
    K, worst = sc_.cpu_bound(SMALL[:6])
    print(f"signal depth, six cases: gradient bound sized on the CPU: K = {K:.4g} (worst restatement grade {worst:.4g})")
    assert K == 2 * worst and math.isfinite(K) and K >= 2.0


# ---- 6. lstm3fit keeps its bytes -------------------------------------------------------------------------------------------
def _batch_terms_before(Xin, y, theta, sc, sh, T, C, opts, act, dtype):
    """lstm3fit.batch_terms as it stood before batch_terms_dx was split off it: the same statements without the data gradient."""
    from nanoreviser_amd.lstm3fit import D_X, H, N_LSTM3, _act_d, bn, lstm, unpack
    dt = np.dtype(dtype)
    theta = np.asarray(theta)
    Xin, H3, keep = lstm(Xin, theta, T, C, act, dt)
    n = Xin.shape[0]
    g4, st, dXb4 = l4.batch_terms_dx(bn(H3, sc, sh, dt), y, theta[N_LSTM3:], T, C, opts, act, dt)
    dX3 = dXb4 * np.asarray(sc).astype(dt)
    parts = [a.astype(dt) for a in unpack(theta, T, C)[:6]]
    one = dt.type(1)
    grads = []
    for d in range(2):
        U = parts[3 * d + 1]
        k = keep[d]
        gW, gU, gb = np.zeros((D_X, 4 * H), dt), np.zeros((H, 4 * H), dt), np.zeros(4 * H, dt)
        dz_next = np.zeros((n, 4 * H), dt)
        dcf = np.zeros((n, H), dt)
        for s in range(T - 1, -1, -1):
            t = T - 1 - s if d else s
            i, f, g, o, c = (k[q][:, s] for q in "ifgoc")
            c_prev = k["c"][:, s - 1] if s > 0 else np.zeros((n, H), dt)
            h_prev = H3[:, (t + 1 if d else t - 1), d * H:(d + 1) * H] if s > 0 else np.zeros((n, H), dt)
            dh = dX3[:, t, d * H:(d + 1) * H] + dz_next @ U.T
            tc = np.tanh(c)
            do = dh * tc
            dc = dh * o * (one - tc * tc) + dcf
            dz = np.concatenate([dc * g * _act_d(i, act), dc * c_prev * _act_d(f, act), dc * i * (one - g * g),
                                 do * _act_d(o, act)], axis=1)
            gW += Xin[:, t].T @ dz
            gU += h_prev.T @ dz
            gb += dz.sum(axis=0)
            dcf = dc * f
            dz_next = dz
        grads += [gW, gU, gb]
    g = np.concatenate([a.ravel() for a in grads]) / dt.type(n)
    return np.concatenate([g.astype(dt), g4]), st


@pytest.mark.parametrize("case", [(11, 1, 33, "plain", 0), (1, 0, 33, "plain", 0), (11, 1, 33, "plain", 1)], ids=IDS)
def test_lstm3fit_batch_terms_dx(case):
    import torch
    T, model, n, kind, act = case
    C = l3c.n_class(model)
    X, y, th = l3c.rows_case(*case)
    sc, sh = l3c.bn(model)
    opts = tf.default_opts(model)
    for dt in (np.float64, np.float32):
        g, st = l3.batch_terms(X, y, th, sc, sh, T, C, opts, act, dt)
        g2, st2, dX = l3.batch_terms_dx(X, y, th, sc, sh, T, C, opts, act, dt)
        assert g.tobytes() == g2.tobytes() and st == st2 and dX.shape == (n, T, 192) and dX.dtype == dt
        g0, st0 = _batch_terms_before(X, y, th, sc, sh, T, C, opts, act, dt)
        assert g.tobytes() == g0.tobytes() and st == st0                                       # its old bytes
    # autograd's derivative of the batch's SUM of row losses with respect to Xin
    tht = torch.tensor(th.astype(np.float64))
    x = torch.tensor(X.astype(np.float64), requires_grad=True)
    x4, _, _, thh = l3c._torch_forward(x, tht, torch.tensor(sc.astype(np.float64)), torch.tensor(sh.astype(np.float64)), T, C, act)
    W1, b1, W2, b2, Wm, bm, Wf, bf, Wo, bo, Ce = l3c.hc._split(thh, T, C, lambda a, s: a.reshape(s))
    yt = torch.tensor(np.asarray(y, np.int64))
    cw = torch.tensor(opts.cw6(), dtype=torch.float64)[yt]
    mo = torch.relu(torch.relu(torch.relu(x4 @ W1 + b1) @ W2 + b2) @ Wm + bm)
    f = torch.relu(mo.reshape(-1, 6 * T) @ Wf + bf)
    logp = torch.log_softmax(f @ Wo + bo, dim=1)
    L = (cw * -logp[torch.arange(n), yt]).sum() + float(np.float32(opts.lam)) * ((f - Ce[yt]) ** 2).sum()
    L.backward()
    want = x.grad.numpy()
    dX = l3.batch_terms_dx(X, y, th, sc, sh, T, C, opts, act, np.float64)[2]
    assert np.abs(dX - want).max() <= 1e-9 * np.abs(want).max() and np.abs(want).max() > 0


# ---- 7. plumbing -----------------------------------------------------------------------------------------------------------
def test_pack_unpack_and_fitted_model(species_models, tmp_path):
    for T, C in ((1, 5), (11, 6), (32, 6)):
        th = np.arange(sf.n_params(T, C), dtype=np.float32)
        parts = sf.unpack(th, T, C)
        assert [a.shape for a in parts[:6]] == [(3, 8), (8,), (3, 8, 8), (8,), (400, 64), (64,)] and len(parts) == 29
        assert np.array_equal(sf.pack(*parts), th) and sf.n_params(T, C) == 25896 + l3.n_params(T, C) and sf.N_SIGNAL == 25896
        assert all(np.array_equal(a, b) for a, b in zip(parts[6:], l3.unpack(th[sf.N_SIGNAL:], T, C)))
        sp = sc_.spans(T, C)
        assert all(np.array_equal(th[sp[k]], a.ravel()) for k, a in zip(sc_.TENSORS, parts))
    with pytest.raises(ValueError, match="signal depth"):
        sf.unpack(np.zeros(l3.n_params(11, 6)), 11, 6)
    for k, m in enumerate(species_models["ecoli"]):
        th = sf.params_from_model(m)
        parts = sf.unpack(th, m.T, m.n_class)
        assert all(np.array_equal(a.ravel(), np.asarray(m.tensors[i]).ravel()) for i, a in zip(FITTED, parts[:28])) and not parts[28].any()
        assert np.array_equal(th[sf.N_SIGNAL:], l3.params_from_model(m))
        theta = sc_.params(11, m.n_class, 9 + k)
        fitted = sf.fitted_model(m, theta)
        assert len(fitted.tensors) == 60 and all(np.asarray(a).shape == np.asarray(b).shape for a, b in zip(fitted.tensors, m.tensors))
        assert all(fitted.tensors[i] is m.tensors[i] or fitted.tensors[i].tobytes() == m.tensors[i].tobytes() for i in FROZEN)
        stem = str(tmp_path / f"m{k}")
        sf.write_f32(fitted, stem)
        back = load_model(stem + ".f32")
        assert all(back.tensors[i].tobytes() == m.tensors[i].tobytes() for i in FROZEN)           # exactly the listed tensors change
        for i, b in zip(FITTED, sf.unpack(theta, 11, m.n_class)[:28]):
            assert np.array_equal(back.tensors[i].ravel(), b.ravel()) and not np.array_equal(back.tensors[i], m.tensors[i]), i
        assert np.array_equal(sf.with_lstm3(th, theta[sf.N_SIGNAL:])[sf.N_SIGNAL:], theta[sf.N_SIGNAL:])
        assert np.array_equal(sf.with_lstm3(th, theta[sf.N_SIGNAL:])[:sf.N_SIGNAL], th[:sf.N_SIGNAL])
    assert sf.adam_step is tf.adam_step and sf.FitOpts is tf.FitOpts and sf.write_f32 is tf.write_f32      # reused, not copied
    assert "moving statistics" in sf.__doc__ and "DEVIATIONS" in sf.__doc__ and "Dropout" in sf.__doc__


# ---- 8. epoch --------------------------------------------------------------------------------------------------------------
def test_epoch_skips_and_counts_a_nonfinite_batch():
    T, model, C, n = 11, 1, 5, 76
    x2, sig, y, th = sc_.rows_case(T, model, 33, "plain", 0)
    cb, (sc, sh) = sc_.conv_bn(model), sc_.bn(model)
    x2 = np.concatenate([x2, x2[:10] * 0.5, x2])[:n]
    sig = np.concatenate([sig, sig[:10] * 0.5, sig])[:n]
    y = np.concatenate([y, y[:10], y])[:n]
    opts = tf.default_opts(model, B=32)
    sn = sig.copy()
    sn[40, 3, 7] = np.inf                                  # lands in the second batch of 32
    s = tf.FitState(th.astype(np.float32))
    st = sf.epoch(x2, sn, y, s, np.arange(n), cb, sc, sh, T, C, opts, 0, np.float32)
    assert (st.rows, st.steps, st.nonfinite, s.t) == (44, 2, 1, 2) and np.isfinite(s.theta).all()
    r = tf.FitState(th.astype(np.float32))
    sf.epoch(x2, sn, y, r, np.concatenate([np.arange(32), np.arange(64, 76)]), cb, sc, sh, T, C, opts, 0, np.float32)
    assert np.array_equal(s.theta, r.theta) and r.t == 2 and not np.array_equal(s.theta[:232], th[:232])
    p, se = sf.evaluate(x2, sig, y, th, np.arange(n), cb, sc, sh, T, C, opts, 0, np.float32)
    assert p.shape == (n, C) and se.rows == n and np.allclose(p.sum(1), 1, atol=1e-6)


# ---- 9. command line -------------------------------------------------------------------------------------------------------
def test_fit_depth_signal_argument_checks(tmp_path, capsys):
    d = str(tmp_path)
    base = ["-d", d, "-S", "ecoli", "-M", str(tmp_path / "out"), "--labels_from", d]
    boom = lambda *a: pytest.fail("no engine may be made for a refused command line")        # noqa: E731
    assert train_cli.main(base + ["--fit_depth", "lstm3"], reviser_factory=boom) == 2
    err = capsys.readouterr().err
    assert all(w in err for w in ("--fit_depth", "tail or head", "lstm4", "'lstm3'", "signal")), err
    for init in ("transfer", "fresh", "fresh_head"):
        assert train_cli.check_args(train_cli.get_args(base + ["--fit_depth", "signal", "--fit_init", init])) is None
    assert "--fit_depth signal" in train_cli.__doc__ and "--fit_depth lstm3 is not" in train_cli.__doc__


def test_train_cli_at_signal_depth_writes_a_model_directory(tmp_path, monkeypatch, species_models):
    import __graft_entry__ as g
    from signalfit_engine import SignalEcho
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
        made.append(SignalEcho(m1.T, (m1, m2)))
        return made[-1]
    m1, m2 = species_models["ecoli"]
    T = m1.T
    out = str(tmp_path / "model")
    argv = ["-d", src, "-S", "ecoli", "-M", out, "-e", "1", "-b", "2048", "--labels_from", lab, "--validation_split", "0.1",
            "--seed", "7", "--fit_depth", "signal", "--model_type", "model2"]
    assert train_cli.main(argv, reviser_factory=factory) == 0
    eng = made[0]
    assert eng.closed and eng.depth_calls == [16]
    n = eng.fit_count()
    n_train, n_val = tf.val_split(n, 0.1)
    stem = train_cli.stem(out, "ecoli", 2)
    back = load_model(stem + ".f32")
    assert back.T == T and all(back.tensors[i].tobytes() == m2.tensors[i].tobytes() for i in FROZEN)
    theta, t = eng.fit_params(1)
    assert theta.size == sf.n_params(T, 5) and t == math.ceil(n_train / 2048)
    for i, b in zip(FITTED, sf.unpack(theta, T, 5)[:28]):
        assert np.array_equal(back.tensors[i].ravel(), b.ravel()) and not np.array_equal(back.tensors[i], m2.tensors[i]), i
    assert np.array_equal(np.fromfile(stem + "_centers.f32", "<f4"), theta[-80:])
    s = json.load(open(stem + "_summary.json"))
    assert s["options"]["fit_depth"] == "signal" and s["options"]["init"] == "transfer" and s["rows"] == n and s["val_rows"] == n_val
    # the start: the signal branch, lstm3 and lstm4 are always the model's own; --fit_init acts on the layers behind lstm4
    base = ["-d", src, "--labels_from", lab, "--fit_depth", "signal", "--seed", "7"]
    own = sf.params_from_model(m1)
    front = sf.N_SIGNAL + l3.N_LSTM3 + l4.N_LSTM4
    th, how = train_cli._start(train_cli.get_args(base), 0, m1, T)
    assert how == "transfer" and np.array_equal(th, own)
    th, how = train_cli._start(train_cli.get_args(base + ["--fit_init", "fresh"]), 0, m1, T)
    assert how == "fresh" and np.array_equal(th[:front], own[:front]) and np.array_equal(th[-tf.n_params(T, 6):], tf.fresh_params(T, 6, 7))
    th, how = train_cli._start(train_cli.get_args(base + ["--model2_train_dir", stem + ".f32"]), 1, m2, T)
    assert how == "continued" and np.array_equal(th, theta)
