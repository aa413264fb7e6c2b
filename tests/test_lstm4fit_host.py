"""The definition of the lstm4 fit (nanoreviser_amd/lstm4fit.py, depth NRV_FIT_LSTM4) and the command line around it, on the CPU:
  1. at float64 the definition's X4 is oracle.nrv_oracle.bilstm's on the same tensors, and the forward behind it headfit.forward;
  2. forward at a shipped model's tensors, on windows of a fixture read with Xb formed from the oracle's lstm3, gives the
     oracle's probabilities;
  3. the float64 gradient is autograd's float64 gradient to 1e-9 of each tensor's scale, in every case;
  4. central differences on a handful of coordinates per tensor agree;
  5. the condition on tests/lstm4fit_cases.py holds;
  6. cpu_bound is finite (its value is printed);
  7. pack / unpack, the vector's length, fitted_model;
  8. epoch skips and counts a non-finite batch;
  9. NanoReviser_train.py --fit_depth lstm4: the argument checks;
 10. a whole run on a stand-in engine driven by the definition (tests/lstm4fit_engine.py) writes the files, the depth recorded."""
import json
import math
import os

import numpy as np
import pytest

import lstm4fit_cases as lc
from nanoreviser_amd import headfit as hf
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import lstm4fit as lf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd import train_cli
from nanoreviser_amd.weights import load_model

IDS = lambda c: "T%d-m%d-n%d-%s-act%d" % c      # noqa: E731
CHUNK_CASE = (2, 0, 4130, "plain", 1)           # tests/test_gpu_lstm4fit.py's batch of more than one scratch chunk
SMALL = [c for c in lc.GRAD_CASES if c[2] <= 96]


# ---- 1, 2. forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(11, 1, 33, "plain", 0), (13, 1, 31, "zeros", 0), (11, 1, 33, "plain", 1), (1, 0, 33, "plain", 0)], ids=IDS)
def test_forward_is_the_oracles_bilstm_and_headfits_forward(case):
    from oracle import nrv_oracle as O
    T, model, n, kind, act = case
    C = lc.n_class(model)
    X, y, th = lc.rows_case(*case)
    parts = [a.astype(np.float64) for a in lf.unpack(th, T, C)[:6]]
    want = O.bilstm(X.astype(np.float64), parts, O.hard_sigmoid if act == 0 else O.sigmoid)
    x4, mo, f, p = lf.forward(X, th, T, C, act, np.float64)
    assert x4.shape == (n, T, 128) and np.abs(x4 - want).max() <= 1e-12
    mo2, f2, p2 = hf.forward(x4, th[lf.N_LSTM4:], T, C, np.float64)
    assert np.array_equal(mo, mo2) and np.array_equal(f, f2) and np.array_equal(p, p2)
    if act == 0:                                           # both clipped sides and the open side are met
        z = np.concatenate([k["z"][:, :, np.r_[0:128, 192:256]].ravel() for k in lf.lstm(X, th, T, C, act, np.float64)[2]])
        assert (z <= -2.5).any() and (z >= 2.5).any() and (np.abs(z) < 2.5).any()


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
        x3 = O.bilstm(np.concatenate([r, s], axis=-1), w[34:40], O.hard_sigmoid)
        xb64 = O._bn(x3, *w[40:44])
        p = lf.forward(xb64, lf.params_from_model(m), 11, m.n_class, 0, np.float64)[3]
        assert np.abs(p - q[k]).max() <= 1e-6, (k, np.abs(p - q[k]).max())      # (the parameters are f32 both ways)
        xb = lf.xb_from_lstm3(x3.astype(np.float32), m)                         # the f32 row the engine's set holds
        assert xb.dtype == np.float32 and xb.shape == (48, 11, 256) and np.abs(xb - xb64).max() <= 1e-5
        sc, sh = lf.bn_scale_shift(m)
        assert np.array_equal(xb, (x3.astype(np.float32) * sc).astype(np.float32) + sh)


# ---- 3 .. 6. gradient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.GRAD_CASES, ids=IDS)
def test_gradient_is_autograds_in_float64(case):
    T, model, n, kind, act = case
    C = lc.n_class(model)
    X, y, th = lc.rows_case(*case)
    opts = tf.default_opts(model)
    g, st = lf.batch_terms(X, y, th, T, C, opts, act, np.float64)
    gt, ce, cn, ok = lc.torch_terms(X, y, th, T, C, opts, act, np.float64)
    sp = lc.spans(T, C)
    for k in lc.TENSORS:
        scale = np.abs(gt[sp[k]]).max()
        assert np.abs(g[sp[k]] - gt[sp[k]]).max() <= 1e-9 * scale, (k, np.abs(g[sp[k]] - gt[sp[k]]).max(), scale)
        assert scale > 0 or (T == 1 and k in ("U4f", "U4b")), k
    if T == 1:
        assert not g[sp["U4f"]].any() and not g[sp["U4b"]].any()
    assert st.correct == ok and abs(st.ce_sum - ce) <= 1e-9 * ce and abs(st.center_sum - cn) <= 1e-9 * cn
    # the head's blocks are headfit.batch_terms' gradient on the definition's own X4
    gh, sth = hf.batch_terms(lf.lstm(X, th, T, C, act, np.float64)[1], y, th[lf.N_LSTM4:], T, C, opts, np.float64)
    assert np.array_equal(g[lf.N_LSTM4:], gh) and sth.correct == st.correct


@pytest.mark.parametrize("case", [(11, 1, 31, "plain", 0), (2, 1, 33, "plain", 0), (11, 1, 33, "plain", 1)], ids=IDS)
def test_central_differences_agree(case):
    T, model, n, kind, act = case
    C = lc.n_class(model)
    X, y, th = lc.rows_case(*case)
    opts = tf.default_opts(model)
    g, _ = lf.batch_terms(X, y, th, T, C, opts, act, np.float64)

    def loss(theta):
        st = lf.evaluate(X, y, theta, np.arange(n), T, C, opts, act, np.float64)[1]
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


@pytest.mark.parametrize("case", lc.GRAD_CASES + [CHUNK_CASE, (11, 0, 1100, "plain", 0)], ids=IDS)
def test_the_condition_on_the_cases_holds(case):
    c = lc.condition(*case)
    print(f"{case}: nearest kink {c['kink']:.3g}, largest f32 - f64 pre-activation difference {c['diff']:.3g}, shares {c['shares']}")
    assert c["same"], case
    if case[4] == 0 and case[2] <= 512:                    # (the 1100-row set of the epoch tests is compared byte for byte, not graded)
        assert c["ok"] and c["kink"] >= 8 * c["diff"] and all(v > 0 for v in c["shares"]), c
    X, y, th = lc.rows_case(*case)
    assert np.all(th != 0) and X.dtype == np.float32
    if case[3] == "zeros":
        assert not X[0].any() and X[1].any()


def test_cpu_bound_of_the_device_grade_is_finite():
    K, worst = lc.cpu_bound(SMALL)
    print(f"lstm4 depth, the cases of at most 96 rows: gradient bound sized on the CPU: K = {K:.4g} (worst restatement grade {worst:.4g})")
    assert K == 2 * worst and math.isfinite(K) and K >= 2.0


# ---- 7. plumbing -----------------------------------------------------------------------------------------------------------
def test_pack_unpack_and_fitted_model(species_models, tmp_path):
    for T, C in ((1, 5), (11, 6), (32, 6)):
        th = np.arange(lf.n_params(T, C), dtype=np.float32)
        parts = lf.unpack(th, T, C)
        assert [a.shape for a in parts[:6]] == [(256, 256), (64, 256), (256,)] * 2 and len(parts) == 17
        assert np.array_equal(lf.pack(*parts), th) and lf.n_params(T, C) == 164352 + hf.n_params(T, C) and lf.N_LSTM4 == 164352
        assert all(np.array_equal(a, b) for a, b in zip(parts[6:], hf.unpack(th[lf.N_LSTM4:], T, C)))
        sp = lc.spans(T, C)
        assert all(np.array_equal(th[sp[k]], a.ravel()) for k, a in zip(lc.TENSORS, parts))
    with pytest.raises(ValueError, match="lstm4 depth"):
        lf.unpack(np.zeros(hf.n_params(11, 6)), 11, 6)
    for k, m in enumerate(species_models["ecoli"]):
        th = lf.params_from_model(m)
        parts = lf.unpack(th, m.T, m.n_class)
        assert all(np.array_equal(a, m.tensors[44 + i]) for i, a in enumerate(parts[:16])) and not parts[16].any()
        assert np.array_equal(th[lf.N_LSTM4:], hf.params_from_model(m))
        theta = lc.params(11, m.n_class, 9 + k)
        fitted = lf.fitted_model(m, theta)
        assert len(fitted.tensors) == 60 and all(a is b or np.array_equal(a, b) for a, b in zip(fitted.tensors[:44], m.tensors[:44]))
        stem = str(tmp_path / f"m{k}")
        lf.write_f32(fitted, stem)
        back = load_model(stem + ".f32")
        for i, (a, b) in enumerate(zip(back.tensors[44:], lf.unpack(theta, 11, m.n_class)[:16])):
            assert np.array_equal(a, b) and not np.array_equal(a, m.tensors[44 + i]), i
        assert np.array_equal(lf.with_head(th, theta[lf.N_LSTM4:])[lf.N_LSTM4:], theta[lf.N_LSTM4:])
    assert lf.adam_step is tf.adam_step and lf.FitOpts is tf.FitOpts and lf.write_f32 is tf.write_f32      # reused, not copied


# ---- 8. epoch --------------------------------------------------------------------------------------------------------------
def test_epoch_skips_and_counts_a_nonfinite_batch():
    T, model, C, n = 11, 1, 5, 76
    X, y, th = lc.rows_case(T, model, 33, "plain", 0)
    X = np.concatenate([X, X[:10] * 0.5, X])[:n]
    y = np.concatenate([y, y[:10], y])[:n]
    opts = tf.default_opts(model, B=32)
    order = np.random.default_rng(1).permutation(n)
    s = tf.FitState(th.astype(np.float64))
    st = lf.epoch(X, y, s, order, T, C, opts, 0, np.float64)
    assert (st.rows, st.steps, st.nonfinite, s.t) == (76, 3, 0, 3)
    r = tf.FitState(th.astype(np.float64))
    for t, (lo, hi) in enumerate(((0, 32), (32, 64), (64, 76)), 1):
        g, _ = lf.batch_terms(X[order[lo:hi]], y[order[lo:hi]], r.theta, T, C, opts, 0, np.float64)
        r.theta, r.m, r.v = tf.adam_step(r.theta, r.m, r.v, g, opts, t, np.float64)
    assert np.array_equal(s.theta, r.theta) and not np.array_equal(s.theta[:lf.N_LSTM4], th[:lf.N_LSTM4])
    Xn = X.copy()
    Xn[40, 3, 7] = np.inf                                  # lands in the second batch of 32
    for dtype in (np.float64, np.float32):
        s = tf.FitState(th.astype(dtype))
        st = lf.epoch(Xn, y, s, np.arange(n), T, C, opts, 0, dtype)
        assert (st.rows, st.steps, st.nonfinite, s.t) == (44, 2, 1, 2) and np.isfinite(s.theta).all()
        r = tf.FitState(th.astype(dtype))
        lf.epoch(Xn, y, r, np.concatenate([np.arange(32), np.arange(64, 76)]), T, C, opts, 0, dtype)
        assert np.array_equal(s.theta, r.theta) and r.t == 2
    p, se = lf.evaluate(X, y, th, np.arange(n), T, C, opts, 0, np.float32)
    assert p.shape == (n, C) and se.rows == n and np.allclose(p.sum(1), 1, atol=1e-6)


# ---- 9, 10. command line ---------------------------------------------------------------------------------------------------
def test_fit_depth_lstm4_argument_checks(tmp_path, capsys):
    d = str(tmp_path)
    base = ["-d", d, "-S", "ecoli", "-M", str(tmp_path / "out"), "--labels_from", d]
    boom = lambda *a: pytest.fail("no engine may be made for a refused command line")        # noqa: E731
    for extra, words in ((["--fit_depth", "lstm3"], ("--fit_depth", "tail or head", "lstm4", "'lstm3'")),
                         (["--fit_depth", "lstm4", "--fit_init", "warm"], ("--fit_init", "fresh_head", "'warm'"))):
        assert train_cli.main(base + extra, reviser_factory=boom) == 2
        err = capsys.readouterr().err
        assert all(w in err for w in words), (extra, err)
    for init in ("transfer", "fresh", "fresh_head"):
        assert train_cli.check_args(train_cli.get_args(base + ["--fit_depth", "lstm4", "--fit_init", init])) is None
    assert "--fit_depth lstm4" in train_cli.__doc__


def test_train_cli_at_lstm4_depth_writes_a_model_directory(tmp_path, monkeypatch, species_models):
    import __graft_entry__ as g
    from lstm4fit_engine import Lstm4Echo
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
        made.append(Lstm4Echo(m1.T))
        return made[-1]
    m1, m2 = species_models["ecoli"]
    T = m1.T
    out = str(tmp_path / "model")
    argv = ["-d", src, "-S", "ecoli", "-M", out, "-e", "1", "-b", "2048", "--labels_from", lab, "--validation_split", "0.1",
            "--seed", "7", "--fit_depth", "lstm4", "--model_type", "model2"]
    assert train_cli.main(argv, reviser_factory=factory) == 0
    eng = made[0]
    assert eng.closed and eng.depth_calls == [4]
    n = eng.fit_count()
    n_train, n_val = tf.val_split(n, 0.1)
    stem = train_cli.stem(out, "ecoli", 2)
    back = load_model(stem + ".f32")
    assert back.T == T and all(np.array_equal(a, b) for a, b in zip(back.tensors[:44], m2.tensors[:44]))
    theta, t = eng.fit_params(1)
    assert theta.size == lf.n_params(T, 5) and t == math.ceil(n_train / 2048)
    for i, (a, b) in enumerate(zip(back.tensors[44:], lf.unpack(theta, T, 5)[:16])):
        assert np.array_equal(a, b) and not np.array_equal(a, m2.tensors[44 + i]), i              # the fitted sixteen, every one moved
    assert np.array_equal(np.fromfile(stem + "_centers.f32", "<f4"), theta[-80:])
    s = json.load(open(stem + "_summary.json"))
    assert s["options"]["fit_depth"] == "lstm4" and s["options"]["init"] == "transfer" and s["rows"] == n and s["val_rows"] == n_val
    # the start: lstm4 is always the model's own; --fit_init acts on the layers behind it as at head depth
    base = ["-d", src, "--labels_from", lab, "--fit_depth", "lstm4", "--seed", "7"]
    own = lf.params_from_model(m1)
    th, how = train_cli._start(train_cli.get_args(base), 0, m1, T)
    assert how == "transfer" and np.array_equal(th, own)
    th, how = train_cli._start(train_cli.get_args(base + ["--fit_init", "fresh"]), 0, m1, T)
    assert how == "fresh" and np.array_equal(th[:lf.N_LSTM4 + hf.N_MLP], own[:lf.N_LSTM4 + hf.N_MLP])
    assert np.array_equal(th[lf.N_LSTM4 + hf.N_MLP:], tf.fresh_params(T, 6, 7))
    th, how = train_cli._start(train_cli.get_args(base + ["--fit_init", "fresh_head"]), 1, m2, T)
    assert how == "fresh_head" and np.array_equal(th[:lf.N_LSTM4], lf.params_from_model(m2)[:lf.N_LSTM4])
    assert np.array_equal(th[lf.N_LSTM4:], hf.fresh_params(T, 5, 8))
    th, how = train_cli._start(train_cli.get_args(base + ["--model2_train_dir", stem + ".f32"]), 1, m2, T)
    assert how == "continued" and np.array_equal(th, theta)
