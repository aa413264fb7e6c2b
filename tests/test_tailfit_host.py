"""The definition of the tail fit (nanoreviser_amd/tailfit.py) and the command line around it, on the CPU:
  1. the definition's gradient against torch.autograd in float64 on tests/tailfit_cases.py;
  2. Adam against a plain scalar loop written here; the elementwise f32 form the device is compared with is the same function;
  3. an epoch: the last batch is short and divided by its own size; a non-finite batch is skipped and counted;
  4. the label mapping against hoststage.score_calls' own y1 / y2 on score_cases;
  5. the weight file round trip: 56 identical tensors and the fitted four;
  6. NanoReviser_train.py: argument refusals, and the files of a run on a stand-in engine (tests/tailfit_engine.py)."""
import json
import math
import os

import numpy as np
import pytest

import score_cases
import tailfit_cases as tc
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd import train_cli
from nanoreviser_amd.weights import load_model


# ---- 1. gradient ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.GRAD_CASES, ids=lambda c: "T%d-m%d-n%d-%s" % c)
def test_gradient_is_autograds_in_float64(case):
    """Both sides evaluate the same expression graph in float64 in their own order.  An element of g is a sum of at most
    n + 16 products (n rows; 16 features or C classes) of factors that each carry a chain of at most 6T + 16 + C + 8
    roundings (the two dense layers, the softmax), so by the standard bound for recursive summation each side is off by at
    most (n + 6T + 48) eps64 times the sum of the ABSOLUTE terms of that element.  Rows pull in both directions, so that sum
    exceeds the element itself; taken over the whole vector in the 2-norm the excess is bounded by sqrt(n) (Cauchy-Schwarz
    over the rows).  Two sides: a factor 2.  The bound is 2 (n + 6T + 48) sqrt(n) eps64 |g|; a wrong formula is off by O(|g|)."""
    T, model, n, kind = case
    C = tc.n_class(model)
    F, y, th = tc.rows_case(*case)
    opts = tf.default_opts(model)
    g, st = tf.batch_terms(F, y, th, T, C, opts, np.float64)
    gt, ce, cn, ok = tc.torch_terms(F, y, th, T, C, opts, np.float64)
    bound = 2 * (n + 6 * T + 48) * math.sqrt(n) * tc.EPS64 * np.linalg.norm(gt)
    assert np.linalg.norm(g - gt) <= bound, (np.linalg.norm(g - gt), bound)
    assert g.size == tf.n_params(T, C) and np.linalg.norm(gt) > 0
    assert st.rows == n and st.correct == ok and st.steps == 0 and st.nonfinite == 0
    assert abs(st.ce_sum - ce) <= 64 * n * tc.EPS64 * max(abs(ce), 1) and abs(st.center_sum - cn) <= 64 * n * tc.EPS64 * max(abs(cn), 1)
    if kind == "absent":                                  # a class nobody has: its centre does not move, its logit still does
        sp = tc.spans(T, C)
        assert not g[sp["Ce"]].reshape(C, 16)[2].any() and g[sp["bo"]][2] != 0


def test_cpu_bound_of_the_device_grade_is_small():
    """the bound the device is held to comes from the CPU alone and stays a small multiple of the f32 floor."""
    K, worst = tc.cpu_bound()
    assert K == 2 * worst and 2.0 <= K <= 64.0, K


# ---- 2. Adam ---------------------------------------------------------------------------------------------------------------
def test_adam_is_the_scalar_loop():
    rng = np.random.default_rng(3)
    opts = tf.FitOpts(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7)
    th = rng.normal(0, 1, 40)
    m, v = np.zeros(40), np.zeros(40)
    b1, b2, eps, lr0 = (float(np.float32(x)) for x in (opts.beta1, opts.beta2, opts.eps, opts.lr))
    th_s, m_s, v_s = th.copy(), m.copy(), v.copy()
    for t in range(1, 6):
        g = rng.normal(0, 0.1, 40)
        th, m, v = tf.adam_step(th, m, v, g, opts, t, np.float64)
        lr_t = lr0 * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        for i in range(40):                               # Keras 2.2.4, optimizers.py Adam.get_updates, one scalar at a time
            m_s[i] = b1 * m_s[i] + (1.0 - b1) * g[i]
            v_s[i] = b2 * v_s[i] + (1.0 - b2) * g[i] * g[i]
            th_s[i] = th_s[i] - lr_t * m_s[i] / (math.sqrt(v_s[i]) + eps)
        assert np.allclose(th, th_s, rtol=8 * tc.EPS64, atol=0) and np.allclose(m, m_s, rtol=8 * tc.EPS64, atol=0)
        assert np.allclose(v, v_s, rtol=8 * tc.EPS64, atol=0)
        g32 = g.astype(np.float32)
        a = tf.adam_step(th.astype(np.float32), m.astype(np.float32), v.astype(np.float32), g32, opts, t, np.float32)
        b = tc.adam_f32(th.astype(np.float32), m.astype(np.float32), v.astype(np.float32), g32, opts, t)
        assert all(x.dtype == np.float32 and np.array_equal(x, y) for x, y in zip(a, b))
    assert abs(tf.lr_t(opts, 1) - lr0 * math.sqrt(1 - b2) / (1 - b1)) < 1e-18


# ---- 3. epoch --------------------------------------------------------------------------------------------------------------
def test_last_batch_is_divided_by_its_own_size():
    T, model, C = 11, 0, 6
    F, y, th = tc.rows_case(T, model, 76)
    opts = tf.default_opts(model, B=32)
    order = np.random.default_rng(1).permutation(76)
    s = tf.FitState(th.astype(np.float64))
    st = tf.epoch(F, y, s, order, T, C, opts, np.float64)
    assert (st.rows, st.steps, st.nonfinite, s.t) == (76, 3, 0, 3)
    r = tf.FitState(th.astype(np.float64))
    for t, (lo, hi) in enumerate(((0, 32), (32, 64), (64, 76)), 1):
        idx = order[lo:hi]
        g, _ = tf.batch_terms(F[idx], y[idx], r.theta, T, C, opts, np.float64)
        if hi == 76:                                      # 12 rows: the mean of 12, not 12 / 32 of a mean
            dup = np.concatenate([idx, idx])
            g2, _ = tf.batch_terms(F[dup], y[dup], r.theta, T, C, opts, np.float64)
            assert np.allclose(g, g2, rtol=0, atol=1e-13 * np.abs(g).max())
        r.theta, r.m, r.v = tf.adam_step(r.theta, r.m, r.v, g, opts, t, np.float64)
    assert np.array_equal(s.theta, r.theta) and np.array_equal(s.m, r.m) and np.array_equal(s.v, r.v)


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_nonfinite_batch_is_skipped_and_counted(dtype):
    T, model, C = 11, 1, 5
    F, y, th = tc.rows_case(T, model, 76)
    F = F.copy()
    F[40, 3] = np.nan                                     # lands in the second batch of 32
    opts = tf.default_opts(model, B=32)
    s = tf.FitState(th.astype(dtype))
    st = tf.epoch(F, y, s, np.arange(76), T, C, opts, dtype)
    assert (st.rows, st.steps, st.nonfinite, s.t) == (44, 2, 1, 2) and np.isfinite(s.theta).all()
    assert np.isfinite(st.ce_sum) and np.isfinite(st.center_sum)
    keep = np.concatenate([np.arange(32), np.arange(64, 76)])
    r = tf.FitState(th.astype(dtype))
    tf.epoch(F, y, r, keep, T, C, tf.default_opts(model, B=32), dtype)
    assert np.array_equal(s.theta, r.theta) and r.t == 2  # the skipped batch left nothing behind: t did not advance either


# ---- 4. labels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 2, 11, 13, 32))
def test_label_mapping_is_the_score_blocks(T):
    c, _, _ = score_cases.cached_case(T=T) if hasattr(score_cases, "cached_case") else (score_cases.score_case(T=T), None, None)
    el = np.asarray(c["ev_len"], np.int64)
    w, y1, y2 = tf.labelled_windows(c["labels"], el, T)
    zeros = np.zeros(c["n"], np.int8)
    sc = hs.score_calls(c["bases"], el, zeros, zeros, None, None, c["labels"], c["score_thr"], T)   # c1 = c2 = 0: column = the label
    ev_off = np.cumsum(el) - el
    read_of = np.searchsorted(ev_off + el, w + (T - 1) // 2, side="right")
    assert w.size == int(sc[:, 1].sum()) > 0 and np.all(np.diff(w) > 0)
    for r in range(len(el)):
        mine = read_of == r
        assert int(mine.sum()) == int(sc[r, 1])
        assert np.array_equal(np.bincount(y1[mine], minlength=6), sc[r, 2:38:6].astype(np.int64)), r
        assert np.array_equal(np.bincount(y2[mine], minlength=5), sc[r, 38:63:5].astype(np.int64)), r
    assert y1.max() <= 5 and y2.max() <= 4 and (y1[y1 > 0] == y2[y1 > 0] + 1).all()


# ---- 5. weight files -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (11, 13))
def test_weight_file_round_trip(tmp_path, species_models, T):
    for k, m in enumerate(species_models["ecoli"]):
        theta = tc.params(T, m.n_class, 9 + k)
        fitted = tf.fitted_model(m, theta, T)
        stem = str(tmp_path / f"m{k}")
        tf.write_f32(fitted, stem)
        back = load_model(stem + ".h5")                   # the .h5 name the command line asks for finds the .f32
        assert back.T == T and back.n_class == m.n_class
        assert all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(back.tensors[:56], m.tensors[:56]))
        for a, b in zip(back.tensors[56:], tf.unpack(theta, T, m.n_class)[:4]):
            assert np.array_equal(a, b)
        assert json.load(open(stem + ".json"))["n_f32"] == fitted.flat().size
        assert np.array_equal(tf.params_from_model(back)[:-16 * m.n_class], theta[:-16 * m.n_class])


def test_fresh_tail_is_glorot_with_zero_biases():
    th = tf.fresh_params(13, 6, 4)
    Wf, bf, Wo, bo, Ce = tf.unpack(th, 13, 6)
    assert not bf.any() and not bo.any() and not Ce.any()
    assert 0.5 * math.sqrt(6 / 94) < np.abs(Wf).max() <= math.sqrt(6 / 94) and np.abs(Wo).max() <= math.sqrt(6 / 22)
    assert np.array_equal(th, tf.fresh_params(13, 6, 4)) and not np.array_equal(th, tf.fresh_params(13, 6, 5))
    assert tf.val_split(1100, 0.01) == (1089, 11) and tf.val_split(10, 0.0) == (10, 0)
    assert sorted(tf.epoch_order(50, 3, 2).tolist()) == list(range(50))
    assert not np.array_equal(tf.epoch_order(50, 3, 2), tf.epoch_order(50, 3, 3))


# ---- 6. command line -------------------------------------------------------------------------------------------------------
def test_train_cli_refuses_bad_arguments(tmp_path, capsys):
    d = str(tmp_path)
    base = ["-d", d, "-S", "ecoli", "-M", str(tmp_path / "out")]
    boom = lambda *a: pytest.fail("no engine may be made for a refused command line")        # noqa: E731
    for extra, word in (([], "--labels_from"), (["--labels_from", d + "/none"], "--labels_from"),
                        (["--labels_from", d, "--model_type", "model3"], "--model_type"),
                        (["--labels_from", d, "--fit_init", "warm"], "--fit_init"),
                        (["--labels_from", d, "-w", "33"], "-w"), (["--labels_from", d, "-e", "0"], "-e"),
                        (["--labels_from", d, "-b", "65537"], "-b"), (["--labels_from", d, "--validation_split", "1.0"], "--validation_split"),
                        (["--labels_from", d, "--class_weight1", "1,2,3"], "--class_weight1"),
                        (["--labels_from", d, "--class_weight2", "1,1,1,1,x"], "--class_weight2")):
        assert train_cli.main(base + extra, reviser_factory=boom) == 2
        assert word in capsys.readouterr().err, extra
    assert train_cli.main(["-d", d + "/none", "--labels_from", d], reviser_factory=boom) == 2


def test_train_cli_writes_a_model_directory(tmp_path, monkeypatch, species_models):
    import __graft_entry__ as g
    from nanoreviser_amd import hostlib
    from tailfit_engine import FitEcho
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
        assert m1.T == m2.T == 13 and m1.n_class == 6 and m2.n_class == 5
        made.append(FitEcho(m1.T))
        return made[-1]
    out = str(tmp_path / "model")
    argv = ["-d", src, "-S", "ecoli", "-M", out, "-w", "13", "-e", "3", "-b", "256", "--labels_from", lab, "--validation_split", "0.1",
            "--reads_per_call", "3", "--seed", "7"]
    assert train_cli.main(argv, reviser_factory=factory) == 0
    eng = made[0]
    assert eng.closed and [c[0] for c in eng.calls] == [3, 1] and eng.calls[0][2] > 0      # two device calls, file order
    n = eng.fit_count()
    m1, m2 = species_models["ecoli"]
    for k, m in enumerate((m1, m2)):
        stem = train_cli.stem(out, "ecoli", k + 1)
        back = load_model(stem + ".h5")
        assert back.T == 13 and all(np.array_equal(a, b) for a, b in zip(back.tensors[:56], m.tensors[:56]))
        theta, t = eng.fit_params(k)
        n_train, n_val = tf.val_split(n, 0.1)
        assert t == 3 * math.ceil(n_train / 256) and n_val > 0
        for a, b in zip(back.tensors[56:], tf.unpack(theta, 13, m.n_class)[:4]):
            assert np.array_equal(a, b)
        assert not np.array_equal(back.tensors[56], m.with_window(13).tensors[56])
        cen = np.fromfile(stem + "_centers.f32", "<f4")
        assert np.array_equal(cen, theta[-16 * m.n_class:]) and cen.any()
        hist = open(stem + "_history.tsv").read().split("\n")
        assert hist[0] == train_cli.HISTORY_HEAD and hist[-1] == "" and len(hist) == 5
        rows = [ln.split("\t") for ln in hist[1:4]]
        assert [r[0] for r in rows] == ["1", "2", "3"] and all(len(r) == 8 and r[7] == "0" for r in rows)
        assert all(math.isfinite(float(x)) for r in rows for x in r[1:7])
        assert float(rows[-1][1]) < float(rows[0][1])     # the stand-in's rows can be fitted: the loss falls
        s = json.load(open(stem + "_summary.json"))
        assert s["rows"] == n and s["train_rows"] == n_train and s["val_rows"] == n_val and s["reads"] == 2
        assert sorted(map(tuple, s["skipped_reads"])) == sorted([(names[1], "no_labels"), (names[2], "stale_labels")])
        assert s["options"]["window_size"] == 13 and s["options"]["init"] == "fresh" and s["seconds"] >= 0
    # an earlier run's tail is where --model1_train_dir starts from; only model 1 is written then
    out2 = str(tmp_path / "model2")
    argv2 = argv[:5] + [out2] + argv[6:] + ["--model_type", "model1", "--model1_train_dir", train_cli.stem(out, "ecoli", 1) + ".f32", "-e", "1"]
    assert train_cli.main(argv2, reviser_factory=factory) == 0
    assert sorted(os.listdir(os.path.join(out2, "ecoli"))) == [f"ecoli_win13_50ep_model1{e}" for e in
                                                               (".f32", ".json", "_centers.f32", "_history.tsv", "_summary.json")]
    assert json.load(open(train_cli.stem(out2, "ecoli", 1) + "_summary.json"))["options"]["init"] == "continued"
