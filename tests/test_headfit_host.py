"""The definition of the head fit (nanoreviser_amd/headfit.py, depth NRV_FIT_HEAD) and the command line around it, on the CPU:
  1. the condition on tests/headfit_cases.py: float64, NumPy float32 and torch float32 take the same side at every ReLU;
  2. the definition's gradient against torch.autograd in float64, to the bound tests/test_tailfit_host.py uses for the tail;
  3. consistency with the tail: the last five blocks are tailfit.batch_terms' gradient on F = the head's own main_out;
  4. the floors: cpu_bound, sized at run time;
  5. an epoch on head rows: the short last batch, a non-finite batch skipped and counted;
  6. plumbing: pack / unpack, params_from_model, fresh_params, fitted_model, the weight file round trip;
  7. NanoReviser_train.py --fit_depth: refusals by text, the unchanged namespace at tail depth, and a whole run at head depth
     on a stand-in engine driven by the definition (tests/headfit_engine.py)."""
import json
import math
import os

import numpy as np
import pytest

import headfit_cases as hc
import tailfit_cases as tc
from nanoreviser_amd import headfit as hf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd import train_cli
from nanoreviser_amd.weights import load_model

IDS = lambda c: "T%d-m%d-n%d-%s" % c      # noqa: E731


# ---- 1. the condition on the cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.GRAD_CASES + [(11, 0, 1100, "plain")], ids=IDS)
def test_every_relu_takes_the_same_side_in_all_three_evaluations(case):
    T, model, n, kind = case
    C = hc.n_class(model)
    X, y, th = hc.rows_case(*case)
    s64, z64 = hc.relu_sides(X, th, T, C, np.float64)
    s32, z32 = hc.relu_sides(X, th, T, C, np.float32)
    st, zt = hc.relu_sides(X, th, T, C, "torch32")
    print(f"{case}: {s64.size} ReLUs, {int(s64.sum())} open; smallest |pre-activation| f64 {z64:.3g}, f32 {z32:.3g}, torch f32 {zt:.3g}")
    assert s64.size == n * (T * (128 + 32 + 6) + 16)
    assert np.array_equal(s64, s32) and np.array_equal(s64, st), (int((s64 != s32).sum()), int((s64 != st).sum()))
    assert 0.2 < s64.mean() < 0.8                          # neither all dead nor all open: every mask matters
    assert np.all(th != 0) and X.dtype == np.float32 and np.abs(X).max() < 1
    if kind == "zeros":
        assert not X[0].any() and X[1].any()


# ---- 2 .. 4. gradient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.GRAD_CASES, ids=IDS)
def test_gradient_is_autograds_in_float64(case):
    """tests/test_tailfit_host.py's bound for the same comparison of the tail, 2 (n + 6T + 48) sqrt(n) eps64 |g|, unchanged."""
    T, model, n, kind = case
    C = hc.n_class(model)
    X, y, th = hc.rows_case(*case)
    opts = tf.default_opts(model)
    g, st = hf.batch_terms(X, y, th, T, C, opts, np.float64)
    gt, ce, cn, ok = hc.torch_terms(X, y, th, T, C, opts, np.float64)
    bound = 2 * (n + 6 * T + 48) * math.sqrt(n) * tc.EPS64 * np.linalg.norm(gt)
    sp = hc.spans(T, C)
    for k in hc.TENSORS:                                   # per tensor, each against its own norm
        bk = 2 * (n + 6 * T + 48) * math.sqrt(n) * tc.EPS64 * np.linalg.norm(gt[sp[k]])
        assert np.linalg.norm(g[sp[k]] - gt[sp[k]]) <= bk, (k, np.linalg.norm(g[sp[k]] - gt[sp[k]]), bk)
        assert np.linalg.norm(gt[sp[k]]) > 0, k
    assert np.linalg.norm(g - gt) <= bound
    assert g.size == hf.n_params(T, C) == 20838 + tf.n_params(T, C)
    assert st.rows == n and st.correct == ok and st.steps == 0 and st.nonfinite == 0
    assert abs(st.ce_sum - ce) <= 64 * n * tc.EPS64 * max(abs(ce), 1) and abs(st.center_sum - cn) <= 64 * n * tc.EPS64 * max(abs(cn), 1)
    if kind == "absent":
        assert not g[sp["Ce"]].reshape(C, 16)[2].any() and g[sp["bo"]][2] != 0


@pytest.mark.parametrize("case", hc.GRAD_CASES, ids=IDS)
def test_last_five_blocks_are_the_tails_gradient(case):
    T, model, n, kind = case
    C = hc.n_class(model)
    X, y, th = hc.rows_case(*case)
    opts = tf.default_opts(model)
    g, st = hf.batch_terms(X, y, th, T, C, opts, np.float64)
    mo, f, p = hf.forward(X, th, T, C, np.float64)
    assert mo.shape == (n, T, 6) and f.shape == (n, 16) and p.shape == (n, C)
    gt, stt = tf.batch_terms(mo.reshape(n, 6 * T), y, th[hf.N_MLP:], T, C, opts, np.float64)
    bound = 2 * (n + 6 * T + 48) * math.sqrt(n) * tc.EPS64 * np.linalg.norm(gt)
    assert np.linalg.norm(g[hf.N_MLP:] - gt) <= bound
    assert (st.rows, st.correct, st.ce_sum, st.center_sum) == (stt.rows, stt.correct, stt.ce_sum, stt.center_sum)


def test_cpu_bound_of_the_device_grade_is_small():
    K, worst = hc.cpu_bound()
    print(f"head depth: gradient bound sized on the CPU: K = {K:.4g} (worst restatement grade {worst:.4g})")
    assert K == 2 * worst and 2.0 <= K <= 64.0, K


# ---- 5. epoch --------------------------------------------------------------------------------------------------------------
def test_epoch_on_head_rows():
    T, model, C, n = 11, 1, 5, 76
    X, y, th = hc.rows_case(T, model, 33)
    X = np.concatenate([X, X[:10] * 0.5, X])[:n]
    y = np.concatenate([y, y[:10], y])[:n]
    opts = tf.default_opts(model, B=32)
    order = np.random.default_rng(1).permutation(n)
    s = tf.FitState(th.astype(np.float64))
    st = hf.epoch(X, y, s, order, T, C, opts, np.float64)
    assert (st.rows, st.steps, st.nonfinite, s.t) == (76, 3, 0, 3)
    r = tf.FitState(th.astype(np.float64))
    for t, (lo, hi) in enumerate(((0, 32), (32, 64), (64, 76)), 1):
        g, _ = hf.batch_terms(X[order[lo:hi]], y[order[lo:hi]], r.theta, T, C, opts, np.float64)
        r.theta, r.m, r.v = tf.adam_step(r.theta, r.m, r.v, g, opts, t, np.float64)
    assert np.array_equal(s.theta, r.theta) and np.array_equal(s.v, r.v)
    Xn = X.copy()
    Xn[40, 3, 7] = np.nan                                  # lands in the second batch of 32
    for dtype in (np.float64, np.float32):
        s = tf.FitState(th.astype(dtype))
        st = hf.epoch(Xn, y, s, np.arange(n), T, C, opts, dtype)
        assert (st.rows, st.steps, st.nonfinite, s.t) == (44, 2, 1, 2) and np.isfinite(s.theta).all()
        r = tf.FitState(th.astype(dtype))
        hf.epoch(Xn, y, r, np.concatenate([np.arange(32), np.arange(64, 76)]), T, C, opts, dtype)
        assert np.array_equal(s.theta, r.theta) and r.t == 2
    p, se = hf.evaluate(X, y, th, np.arange(n), T, C, opts, np.float32)
    assert p.shape == (n, C) and se.rows == n and np.allclose(p.sum(1), 1, atol=1e-6)


# ---- 6. plumbing -----------------------------------------------------------------------------------------------------------
def test_pack_unpack_and_the_models_own_head(species_models):
    for T, C in ((1, 5), (11, 6), (13, 5), (32, 6)):
        th = np.arange(hf.n_params(T, C), dtype=np.float32)
        parts = hf.unpack(th, T, C)
        assert [a.shape for a in parts] == [(128, 128), (128,), (128, 32), (32,), (32, 6), (6,), (6 * T, 16), (16,), (16, C), (C,), (C, 16)]
        assert np.array_equal(hf.pack(*parts), th) and hf.n_params(T, C) == 20838 + tf.n_params(T, C)
        assert all(np.array_equal(a, b) for a, b in zip(parts[6:], tf.unpack(th[hf.N_MLP:], T, C)))
        sp = hc.spans(T, C)
        assert all(np.array_equal(th[sp[k]], a.ravel()) for k, a in zip(hc.TENSORS, parts))
    with pytest.raises(ValueError, match="head depth"):
        hf.unpack(np.zeros(tf.n_params(11, 6)), 11, 6)
    for m in species_models["ecoli"]:
        th = hf.params_from_model(m)
        parts = hf.unpack(th, m.T, m.n_class)
        assert all(np.array_equal(a, m.tensors[50 + i]) for i, a in enumerate(parts[:10])) and not parts[10].any()
        assert np.array_equal(th[hf.N_MLP:], tf.params_from_model(m))
    th = hf.fresh_params(13, 6, 4)
    parts = hf.unpack(th, 13, 6)
    assert all(not parts[i].any() for i in (1, 3, 5, 7, 9, 10)) and all(parts[i].any() for i in (0, 2, 4, 6, 8))
    for i, (a, b) in ((0, (128, 128)), (2, (128, 32)), (4, (32, 6)), (6, (78, 16)), (8, (16, 6))):
        lim = math.sqrt(6 / (a + b))
        assert 0.5 * lim < np.abs(parts[i]).max() <= lim
    assert np.array_equal(th, hf.fresh_params(13, 6, 4)) and not np.array_equal(th, hf.fresh_params(13, 6, 5))
    t2 = hf.with_tail(th, tf.fresh_params(13, 6, 9))
    assert np.array_equal(t2[:hf.N_MLP], th[:hf.N_MLP]) and np.array_equal(t2[hf.N_MLP:], tf.fresh_params(13, 6, 9))
    assert hf.adam_step is tf.adam_step and hf.lr_t is tf.lr_t and hf.val_split is tf.val_split and hf.epoch_order is tf.epoch_order
    assert hf.FitOpts is tf.FitOpts and hf.FitStats is tf.FitStats and hf.write_f32 is tf.write_f32      # reused, not copied


@pytest.mark.parametrize("T", (11, 13))
def test_fitted_model_replaces_50_to_59_and_the_file_round_trips(tmp_path, species_models, T):
    for k, m in enumerate(species_models["ecoli"]):
        theta = hc.params(T, m.n_class, 9 + k)
        fitted = hf.fitted_model(m, theta, T)
        assert len(fitted.tensors) == 60 and all(a is b or np.array_equal(a, b) for a, b in zip(fitted.tensors[:50], m.tensors[:50]))
        stem = str(tmp_path / f"m{k}")
        hf.write_f32(fitted, stem)
        back = load_model(stem + ".h5")
        assert back.T == T and back.n_class == m.n_class
        assert all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(back.tensors[:50], m.tensors[:50]))
        for i, (a, b) in enumerate(zip(back.tensors[50:], hf.unpack(theta, T, m.n_class)[:10])):
            assert np.array_equal(a, b) and not np.array_equal(a, m.with_window(T).tensors[50 + i]), i
        assert json.load(open(stem + ".json"))["n_f32"] == fitted.flat().size
        assert np.array_equal(hf.params_from_model(back)[:-16 * m.n_class], theta[:-16 * m.n_class])


# ---- 7. command line -------------------------------------------------------------------------------------------------------
def test_fit_depth_refusals_and_the_unchanged_namespace(tmp_path, capsys):
    d = str(tmp_path)
    base = ["-d", d, "-S", "ecoli", "-M", str(tmp_path / "out"), "--labels_from", d]
    boom = lambda *a: pytest.fail("no engine may be made for a refused command line")        # noqa: E731
    for extra, words in ((["--fit_depth", "body"], ("--fit_depth", "tail or head", "'body'")),
                         (["--fit_init", "fresh_head"], ("--fit_init fresh_head", "--fit_depth tail")),
                         (["--fit_depth", "head", "--fit_init", "warm"], ("--fit_init", "fresh_head", "'warm'")),
                         (["--fit_depth", "tail", "--fit_init", "warm"], ("--fit_init must be transfer or fresh",))):
        assert train_cli.main(base + extra, reviser_factory=boom) == 2
        err = capsys.readouterr().err
        assert all(w in err for w in words), (extra, err)
    a0, a1 = train_cli.get_args(base), train_cli.get_args(base + ["--fit_depth", "tail"])
    assert vars(a0) == vars(a1) and a0.fit_depth == "tail"
    assert train_cli.check_args(a0) is None and train_cli.check_args(a1) is None and vars(a0) == vars(a1)
    today = {"fast5_base_dir", "species", "output_model", "window_size", "epochs", "batch_size", "validation_split", "model_type",
             "model1_train_dir", "model2_train_dir", "labels_from", "seed", "lr", "center_weight", "class_weight1", "class_weight2",
             "fit_init", "model_dir", "basecall_group", "basecall_subgroup", "reads_per_call", "cw1", "cw2"}
    assert set(vars(a0)) == today | {"fit_depth"}
    for init in ("transfer", "fresh", "fresh_head"):
        assert train_cli.check_args(train_cli.get_args(base + ["--fit_depth", "head", "--fit_init", init])) is None


def test_train_cli_at_head_depth_writes_a_model_directory(tmp_path, monkeypatch, species_models):
    import __graft_entry__ as g
    from headfit_engine import HeadEcho
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
    src = _many(tmp_path, 4)
    names = sorted(os.listdir(src))
    lab = _labels_dir(tmp_path, names, (names[1],), (names[2],))
    made = []

    def factory(a, m1, m2):
        made.append(HeadEcho(m1.T))
        return made[-1]
    m1, m2 = species_models["ecoli"]
    T = m1.T
    out = str(tmp_path / "model")
    argv = ["-d", src, "-S", "ecoli", "-M", out, "-e", "2", "-b", "256", "--labels_from", lab, "--validation_split", "0.1",
            "--reads_per_call", "3", "--seed", "7", "--fit_depth", "head"]
    assert train_cli.main(argv, reviser_factory=factory) == 0
    eng = made[0]
    assert eng.closed and eng.depth_calls == [1] and [c[0] for c in eng.calls] == [3, 1] and eng.calls[0][2] > 0
    n = eng.fit_count()
    n_train, n_val = tf.val_split(n, 0.1)
    for k, m in enumerate((m1, m2)):
        stem = train_cli.stem(out, "ecoli", k + 1)
        back = load_model(stem + ".h5")
        assert back.T == T and all(np.array_equal(a, b) for a, b in zip(back.tensors[:50], m.tensors[:50]))
        theta, t = eng.fit_params(k)
        assert theta.size == hf.n_params(T, m.n_class) and t == 2 * math.ceil(n_train / 256)
        for i, (a, b) in enumerate(zip(back.tensors[50:], hf.unpack(theta, T, m.n_class)[:10])):
            assert np.array_equal(a, b) and not np.array_equal(a, m.tensors[50 + i]), i       # the fitted ten, every one moved
        cen = np.fromfile(stem + "_centers.f32", "<f4")
        assert np.array_equal(cen, theta[-16 * m.n_class:]) and cen.any()
        hist = open(stem + "_history.tsv").read().split("\n")
        assert hist[0] == train_cli.HISTORY_HEAD and hist[-1] == "" and len(hist) == 4
        s = json.load(open(stem + "_summary.json"))
        assert s["options"]["fit_depth"] == "head" and s["options"]["init"] == "transfer" and s["rows"] == n and s["val_rows"] == n_val
    # the start: transfer is the model's own 50 .. 59; fresh keeps 50 .. 55 and draws the tail; fresh_head draws all five layers
    base = ["-d", src, "--labels_from", lab, "--fit_depth", "head", "--seed", "7"]
    own = hf.params_from_model(m1)
    th, how = train_cli._start(train_cli.get_args(base), 0, m1, T)
    assert how == "transfer" and np.array_equal(th, own)
    th, how = train_cli._start(train_cli.get_args(base + ["--fit_init", "fresh"]), 0, m1, T)
    assert how == "fresh" and np.array_equal(th[:hf.N_MLP], own[:hf.N_MLP]) and np.array_equal(th[hf.N_MLP:], tf.fresh_params(T, 6, 7))
    th, how = train_cli._start(train_cli.get_args(base + ["-w", "13"]), 1, m2, 13)
    assert how == "fresh" and th.size == hf.n_params(13, 5) and np.array_equal(th[:hf.N_MLP], hf.params_from_model(m2)[:hf.N_MLP])
    assert np.array_equal(th[hf.N_MLP:], tf.fresh_params(13, 5, 8))
    th, how = train_cli._start(train_cli.get_args(base + ["--fit_init", "fresh_head"]), 1, m2, T)
    assert how == "fresh_head" and np.array_equal(th, hf.fresh_params(T, 5, 8))
    # an earlier head run is where --model1_train_dir continues from, centres included; only model 1 is written then
    out2 = str(tmp_path / "model2")
    prev = train_cli.stem(out, "ecoli", 1)
    argv2 = ["-d", src, "-S", "ecoli", "-M", out2] + argv[6:] + ["--model_type", "model1", "--model1_train_dir", prev + ".f32", "-e", "1"]
    assert train_cli.main(argv2, reviser_factory=factory) == 0
    assert sorted(os.listdir(os.path.join(out2, "ecoli"))) == [f"ecoli_win13_50ep_model1{e}" for e in
                                                               (".f32", ".json", "_centers.f32", "_history.tsv", "_summary.json")]
    s2 = json.load(open(train_cli.stem(out2, "ecoli", 1) + "_summary.json"))
    assert s2["options"]["init"] == "continued" and s2["options"]["fit_depth"] == "head"
    th, how = train_cli._start(train_cli.get_args(argv2), 0, m1, T)
    assert how == "continued" and np.array_equal(th, made[0].fit_params(0)[0])
    # at tail depth the summary is today's: no depth key, and the engine is never asked for a depth
    out3 = str(tmp_path / "model3")
    argv3 = ["-d", src, "-S", "ecoli", "-M", out3, "-e", "1", "--labels_from", lab, "--model_type", "model2"]
    assert train_cli.main(argv3, reviser_factory=factory) == 0
    assert made[-1].depth_calls == [] and made[-1].depth == 0
    assert "fit_depth" not in json.load(open(train_cli.stem(out3, "ecoli", 2) + "_summary.json"))["options"]
