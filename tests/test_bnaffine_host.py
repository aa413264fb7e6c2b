"""The definition of the gamma / beta fit (nanoreviser_amd/bnaffine.py), on the CPU:
  1. the analytic gamma / beta gradient agrees with central differences of the definition's own float64 loss, for every BatchNorm
     at each of the three depths, both models, both gate functions, at T = 1 and T = 3 with three rows;
  2. the rest of the gradient IS the depth's own definition on the folded pairs, and the statistics are its;
  3. params_from_model and the fold give signalfit.conv_bn, fullfit.read_bn and lstm3's pairs byte for byte; the block's lengths;
  4. fitted_model changes tensors base, base + 1 of the BatchNorms inside and no other byte;
  5. epoch refolds behind every update and skips a non-finite batch, which changes nothing;
  6. `taps` absent changes nothing in the three depths' definitions;
  7. the command line: the refusals of train_cli, a stand-in run of --fit_bn_affine -e 1, alone and with --bn_reestimate;
  8. cpu_bound is finite (its value is printed) and the recorded bound stands in the cases file."""
import json
import math
import os

import numpy as np
import pytest

import bnaffine_cases as bac
import bnfit_cases as bc
from nanoreviser_amd import bnaffine as ba
from nanoreviser_amd import bnfit, fitdepth, train_cli
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import lstm3fit as l3
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.weights import load_model

BN_AFFINE = [2, 3, 8, 9, 18, 19, 28, 29, 40, 41]


def _depth_terms(depth, x, sig, y, theta, pairs, T, C, opts, act, dt, **kw):
    if depth == "full":
        return ff.batch_terms(x, sig, y, theta, pairs["bn_l1"] + pairs["bn_l2"], pairs["bn_c1"] + pairs["bn_c2"], *pairs["bn_l3"], T, C,
                              opts, act, dt, **kw)
    if depth == "signal":
        return sf.batch_terms_dx(x, sig, y, theta, pairs["bn_c1"] + pairs["bn_c2"], *pairs["bn_l3"], T, C, opts, act, dt, **kw)[:2]
    return l3.batch_terms_dx(x, y, theta, *pairs["bn_l3"], T, C, opts, act, dt, **kw)[:2]


# ---- 1. central differences ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bac.CD_CASES, ids=bac.IDS)
def test_gamma_beta_gradient_against_central_differences(case):
    depth, T, model, n, act, variant = case
    C = bac.n_class(model)
    x, sig, y, vec, stats = bac.rows_case(*case)
    opts = tf.default_opts(model)
    g, _ = ba.batch_terms(depth, x, sig, y, vec, stats, T, C, opts, act, np.float64, np.float64)

    def loss(v):
        st = ba.evaluate(depth, x, sig, y, v, np.arange(n), stats, T, C, opts, act, np.float64, np.float64)[1]
        return (st.ce_sum + float(np.float32(opts.lam)) * st.center_sum) / n
    rng = np.random.default_rng(1)
    v64 = vec.astype(np.float64)
    sp = bac.spans(depth)
    assert list(sp) == list(bac.names(depth)) and len(sp) == 2 * len(bnfit.inside(depth))
    for k, s in sp.items():
        assert np.abs(g[s]).max() > 0, k
        big = np.argsort(-np.abs(g[s]))[:8]                 # coordinates whose derivative is not lost in the difference's rounding
        for j in rng.choice(big, 3, replace=False):
            i, h = s.start + int(j), 1e-6
            a, b = v64.copy(), v64.copy()
            a[i] += h
            b[i] -= h
            num = (loss(a) - loss(b)) / (2 * h)
            assert abs(num - g[i]) <= 1e-5 * max(abs(g[i]), np.abs(g[s]).max()), (k, int(j), num, g[i])


# ---- 2. the rest is the depth's own ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in bac.CASES if c[3] <= 33], ids=bac.IDS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_rest_of_the_gradient_is_the_depths_own_definition(case, dtype):
    depth, T, model, n, act, variant = case
    C = bac.n_class(model)
    x, sig, y, vec, stats = bac.rows_case(*case)
    opts = tf.default_opts(model)
    nb = ba.n_block(depth)
    g, st = ba.batch_terms(depth, x, sig, y, vec, stats, T, C, opts, act, dtype)
    pairs = ba.pairs_of(depth, vec, stats)
    g0, st0 = _depth_terms(depth, x, sig, y, vec[nb:], pairs, T, C, opts, act, np.dtype(dtype))
    assert g.shape == (ba.n_params(depth, T, C),) and g.dtype == np.dtype(dtype)
    assert np.array_equal(g[nb:], g0) and st == st0
    p, se = ba.evaluate(depth, x, sig, y, vec, np.arange(n), stats, T, C, opts, act, dtype)
    assert (se.ce_sum, se.center_sum, se.correct) == (st.ce_sum, st.center_sum, st.correct) and p.shape == (n, C)
    if variant == "gamma0":                                 # a dead scale: its beta still has a gradient, and nothing divides by it
        assert all(pairs[k][0][1] == 0 for k in pairs) and np.isfinite(g).all()
        assert all(g[s][1] != 0 for k, s in bac.spans(depth).items() if k.endswith("beta"))


# ---- 3. the block and the fold ---------------------------------------------------------------------------------------------
def test_params_from_model_and_the_fold_give_the_depths_pairs_byte_for_byte(species_models):
    assert [ba.n_block(d) for d in bac.DEPTHS] == [512, 544, 864] == [fitdepth.BY_NAME[d].bn for d in bac.DEPTHS]
    assert all(d.bn == 0 for d in fitdepth.DEPTHS if d.name not in bac.DEPTHS)
    for sp in species_models.values():
        for m in sp:
            T, C = m.T, m.n_class
            for depth in bac.DEPTHS:
                fit = fitdepth.BY_NAME[depth].fit
                vec = ba.params_from_model(depth, m)
                nb = ba.n_block(depth)
                assert vec.dtype == np.float32 and vec.size == ba.n_params(depth, T, C) == nb + fit.n_params(T, C)
                assert vec[nb:].tobytes() == fit.params_from_model(m).tobytes()
                gb, theta = ba.unpack(depth, vec, T, C)
                assert list(gb) == list(bnfit.inside(depth)) and theta.size == fit.n_params(T, C)
                for k, (g, b) in gb.items():
                    base = bnfit.BATCHNORMS[k][0]
                    assert g.tobytes() == np.asarray(m.tensors[base], np.float32).tobytes()
                    assert b.tobytes() == np.asarray(m.tensors[base + 1], np.float32).tobytes()
                assert ba.pack(depth, gb, theta).tobytes() == vec.tobytes()
                pairs = ba.pairs_of(depth, vec, ba.stats_of(m))
                want = dict(zip(("bn_l3",), (tuple(l4.bn_scale_shift(m)),)))
                if depth != "lstm3":
                    cb = sf.conv_bn(m)
                    want.update(bn_c1=cb[:2], bn_c2=cb[2:])
                if depth == "full":
                    rb = ff.read_bn(m)
                    want.update(bn_l1=rb[:2], bn_l2=rb[2:])
                assert set(pairs) == set(want)
                for k in pairs:
                    assert pairs[k][0].tobytes() == want[k][0].tobytes() and pairs[k][1].tobytes() == want[k][1].tobytes(), (depth, k)
    with pytest.raises(ValueError, match="no BatchNorm lies inside"):
        ba.n_block("lstm4")
    with pytest.raises(ValueError, match="with the BatchNorm block in front"):
        ba.unpack("signal", np.zeros(sf.n_params(11, 6), np.float32), 11, 6)


# ---- 4. fitted_model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", bac.DEPTHS)
def test_fitted_model_changes_gamma_and_beta_of_the_batchnorms_inside_and_nothing_else(species_models, depth):
    m = species_models["ecoli"][1]
    T, C = m.T, m.n_class
    fit = fitdepth.BY_NAME[depth].fit
    vec = ba.params_from_model(depth, m)
    same = ba.fitted_model(depth, m, vec)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(same.tensors, m.tensors))
    rng = np.random.default_rng(4)
    moved = vec.copy()
    nb = ba.n_block(depth)
    moved[:nb] += rng.normal(0, 0.1, nb).astype(np.float32)
    out = ba.fitted_model(depth, m, moved)
    own = fit.fitted_model(m, moved[nb:], T)
    inside = [bnfit.BATCHNORMS[k][0] + i for k in bnfit.inside(depth) for i in range(2)]
    for i in range(60):
        a, b = np.asarray(out.tensors[i]), np.asarray(own.tensors[i])
        assert a.shape == b.shape and a.dtype == np.float32
        assert (a.tobytes() != b.tobytes()) == (i in inside), i
    gb, _ = ba.unpack(depth, moved, T, C)
    for k, (g, b) in gb.items():
        base = bnfit.BATCHNORMS[k][0]
        assert out.tensors[base].tobytes() == g.tobytes() and out.tensors[base + 1].tobytes() == b.tobytes()
        assert all(out.tensors[base + i].tobytes() == np.asarray(m.tensors[base + i]).tobytes() for i in (2, 3))
    assert set(inside) <= set(BN_AFFINE) and out.source.endswith("+bnaffine")
    # with re-estimated statistics as well: bnfit.with_stats on top
    stats = {k: {"mean": np.full(bnfit.BATCHNORMS[k][1], 0.25, np.float32), "var": np.full(bnfit.BATCHNORMS[k][1], 2.0, np.float32)}
             for k in bnfit.inside(depth)}
    both = bnfit.with_stats(out, stats)
    for k in bnfit.inside(depth):
        base = bnfit.BATCHNORMS[k][0]
        assert both.tensors[base].tobytes() == out.tensors[base].tobytes() and float(both.tensors[base + 3].ravel()[0]) == 2.0


# ---- 5. epoch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", bac.DEPTHS)
def test_epoch_refolds_behind_every_update_and_skips_a_non_finite_batch(depth):
    T, model, n, act = 3, 0, 33, 0
    C = 6
    x, sig, y, vec, stats = bac.rows_case(depth, T, model, n, act, "plain")
    opts = tf.FitOpts(B=11, lr=1e-2, lam=tf.LAMBDA, cw=tf.CW1)
    order = np.arange(n)
    state = tf.FitState(vec.copy())
    tot = ba.epoch(depth, x, sig, y, state, order, stats, T, C, opts, act, np.float32)
    assert tot.steps == 3 and tot.nonfinite == 0 and state.t == 3 and tot.rows == n
    # by hand: the gradient of each batch at the vector the update before it left - so on the pairs refolded from it
    th, m_, v_ = vec.copy(), np.zeros_like(vec), np.zeros_like(vec)
    nb = ba.n_block(depth)
    for k in range(3):
        idx = order[11 * k:11 * k + 11]
        g, _ = ba.batch_terms(depth, x[idx], None if sig is None else sig[idx], y[idx], th, stats, T, C, opts, act, np.float32)
        before = ba.pairs_of(depth, th, stats)
        th, m_, v_ = tf.adam_step(th, m_, v_, g, opts, k + 1, np.dtype(np.float32))
        after = ba.pairs_of(depth, th, stats)
        assert all(before[q][0].tobytes() != after[q][0].tobytes() and before[q][1].tobytes() != after[q][1].tobytes() for q in before)
    assert np.asarray(state.theta).tobytes() == th.tobytes() and not np.array_equal(th[:nb], vec[:nb])
    # a batch holding inf: counted, and neither the vector nor Adam's state moves
    xb = np.array(sig if depth != "lstm3" else x)
    xb[12] = np.inf
    state2 = tf.FitState(vec.copy())
    args = (x, xb) if depth != "lstm3" else (xb, None)
    tot2 = ba.epoch(depth, *args, y, state2, order, stats, T, C, opts, act, np.float32)
    assert tot2.nonfinite == 1 and tot2.steps == 2 and state2.t == 2 and tot2.rows == 22
    state3 = tf.FitState(vec.copy())
    ba.epoch(depth, x, sig, y, state3, np.r_[order[:11], order[22:]], stats, T, C, opts, act, np.float32)
    assert np.asarray(state2.theta).tobytes() == np.asarray(state3.theta).tobytes()


# ---- 6. taps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", bac.DEPTHS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_taps_absent_changes_nothing_and_present_names_the_five_pairs(depth, dtype):
    T, model, n, act = 3, 1, 33, 0
    C = 5
    x, sig, y, vec, stats = bac.rows_case(depth, T, model, n, act, "plain")
    opts = tf.default_opts(model)
    pairs = ba.pairs_of(depth, vec, stats)
    theta = vec[ba.n_block(depth):]
    taps = {}
    a = _depth_terms(depth, x, sig, y, theta, pairs, T, C, opts, act, np.dtype(dtype))
    b = _depth_terms(depth, x, sig, y, theta, pairs, T, C, opts, act, np.dtype(dtype), taps=taps)
    c = _depth_terms(depth, x, sig, y, theta, pairs, T, C, opts, act, np.dtype(dtype), taps=None)
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1] == b[1] == c[1]
    assert list(sorted(taps)) == sorted(bnfit.inside(depth))
    shapes = {"bn_l3": (n, T, 256), "bn_l2": (n, T, 128), "bn_l1": (n, T, 32), "bn_c2": (n, T, 50, 8), "bn_c1": (n, T, 50, 8)}
    for k, (dy, xa) in taps.items():
        assert dy.shape == xa.shape == shapes[k] and dy.dtype == xa.dtype == np.dtype(dtype), k


# ---- 7. the command line ---------------------------------------------------------------------------------------------------
def test_train_cli_refusals(tmp_path, capsys):
    base = ["-d", str(tmp_path), "--labels_from", str(tmp_path)]

    def boom(*a):
        raise AssertionError("a refused command line made an engine")
    for depth in ("tail", "head", "lstm4"):
        err = train_cli.check_args(train_cli.get_args(base + ["--fit_depth", depth, "--fit_bn_affine"]))
        assert err == f"--fit_bn_affine: no BatchNorm lies inside the fitted section at --fit_depth {depth} (signal and full have them)"
        assert train_cli.main(base + ["--fit_depth", depth, "--fit_bn_affine"], reviser_factory=boom) == 2
        assert "--fit_bn_affine" in capsys.readouterr().err
    assert "--fit_depth must be" in train_cli.check_args(train_cli.get_args(base + ["--fit_depth", "lstm3", "--fit_bn_affine"]))
    assert train_cli.main(base + ["--fit_bn_affine"], reviser_factory=boom) == 2          # the default depth is tail
    capsys.readouterr()
    for depth in ("signal", "full"):
        assert train_cli.check_args(train_cli.get_args(base + ["--fit_depth", depth, "--fit_bn_affine"])) is None
        assert train_cli.check_args(train_cli.get_args(base + ["--fit_depth", depth, "--fit_bn_affine", "--bn_reestimate", "-e", "0"])) is None
        assert train_cli.check_args(train_cli.get_args(base + ["--fit_depth", depth, "--fit_bn_affine", "-e", "0"])) == "-e must be at least 1"
    a = train_cli.get_args(base)
    assert not train_cli.fit_bn_affine(a) and not hasattr(a, "fit_bn_affine")
    assert train_cli.fit_bn_affine(train_cli.get_args(base + ["--fit_bn_affine"])) and "--fit_bn_affine" in train_cli.__doc__


def test_train_cli_fit_bn_affine_on_the_stand_in(tmp_path, monkeypatch, species_models):
    import __graft_entry__ as g
    from bnaffine_engine import AffineEcho
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
    src = _many(tmp_path, 1)
    lab = _labels_dir(tmp_path, sorted(os.listdir(src)), (), ())
    made = []

    def factory(a, m1, m2):
        made.append(AffineEcho(m1.T, (m1, m2)))
        return made[-1]
    m1, m2 = species_models["ecoli"]
    T = m1.T

    def run(name, *extra):
        out = str(tmp_path / name)
        argv = ["-d", src, "-S", "ecoli", "-M", out, "-b", "512", "--labels_from", lab, "--validation_split", "0.8", "--seed", "7",
                "--fit_depth", "full", "--model_type", "model2", "-e", "1"] + list(extra)
        assert train_cli.main(argv, reviser_factory=factory) == 0
        stem = train_cli.stem(out, "ecoli", 2)
        return made[-1], stem, json.load(open(stem + "_summary.json"))

    # without the option: no call, no entry, and gamma / beta are the loaded bytes
    eng, stem, s = run("plain")
    assert eng.affine_calls == [] and "bn_affine" not in s and "fit_bn_affine" not in s["options"] and eng.closed
    plain = load_model(stem + ".f32")
    assert all(plain.tensors[i].tobytes() == np.asarray(m2.tensors[i]).tobytes() for i in BN_AFFINE)
    n = eng.fit_count()
    n_train, _ = tf.val_split(n, 0.8)
    # with it: switched on behind fit_set_depth on the empty set; the vector starts from the model's own gamma / beta
    eng, stem, s = run("affine", "--fit_bn_affine")
    assert eng.affine_calls == [(True, 0)] and eng.depth_calls[-1] == 32 and eng.bn_calls == []
    theta, t = eng.fit_params(1)
    assert t == math.ceil(n_train / 512) and theta.size == ba.n_params("full", T, 5)
    twin = AffineEcho(T, (m1, m2))
    twin.fit_set_depth("full")
    twin.fit_set_bn_affine(True)
    twin.feat, twin.sig, twin.y = eng.feat, eng.sig, eng.y
    twin.fit_begin(1, ba.params_from_model("full", m2), tf.FitOpts(B=512, lr=1e-3, lam=tf.LAMBDA, cw=tf.CW2))
    twin.fit_epoch(1, tf.epoch_order(n_train, 7, 0))
    assert twin.fit_params(1)[0].tobytes() == theta.tobytes()
    back = load_model(stem + ".f32")
    assert back.flat().tobytes() == ba.fitted_model("full", m2, theta, T).flat().tobytes()
    assert all(back.tensors[i].tobytes() != np.asarray(m2.tensors[i]).tobytes() for i in BN_AFFINE)
    assert all(back.tensors[i].tobytes() == np.asarray(m2.tensors[i]).tobytes() for i in (4, 5, 10, 11, 20, 21, 30, 31, 42, 43))
    assert np.fromfile(stem + "_centers.f32", "<f4").tobytes() == theta[-16 * 5:].tobytes()
    e = s["bn_affine"]
    start = ba.params_from_model("full", m2)
    assert s["options"]["fit_bn_affine"] is True and list(e) == ["bn_c1", "bn_c2", "bn_l1", "bn_l2", "bn_l3"]
    for k, (sg, sb) in ba.spans("full").items():
        assert e[k] == {"max_dgamma": float(np.abs(theta[sg].astype(np.float64) - start[sg]).max()),
                        "max_dbeta": float(np.abs(theta[sb].astype(np.float64) - start[sb]).max())}
        assert 0 < e[k]["max_dgamma"] < 0.01 and 0 < e[k]["max_dbeta"] < 0.01      # one Adam step of lr 1e-3 per batch
    # with --bn_reestimate: the statistics first, on the starting gamma / beta, then the fit on them; the model carries both
    eng, stem, s = run("both", "--fit_bn_affine", "--bn_reestimate")
    assert [(k, r.tolist(), t_) for k, r, t_ in eng.bn_calls] == [(1, list(range(n_train)), 0)] and eng.affine_calls == [(True, 0)]
    theta2, _ = eng.fit_params(1)
    stats = eng.fit_bn_stats(1)
    both = load_model(stem + ".f32")
    assert both.flat().tobytes() == bnfit.with_stats(ba.fitted_model("full", m2, theta2, T), stats).flat().tobytes()
    assert theta2.tobytes() != theta.tobytes() and "bn_reestimate" in s and "bn_affine" in s


# ---- 8. the bound ----------------------------------------------------------------------------------------------------------
def test_cpu_bound_is_finite_and_recorded():
    small = [c for c in bac.CASES if c[3] <= 33]
    K, worst = bac.cpu_bound(small)
    print(f"bnaffine: K = {K:.4g} over the cases of at most 33 rows (worst restatement grade {worst:.4g}); recorded over all {bac.K_RECORDED}")
    assert np.isfinite(K) and K >= 2.0
    assert bac.K_RECORDED is not None and np.isfinite(bac.K_RECORDED) and bac.K_RECORDED >= 2.0
    for c in small:
        r = bac.reference(*c)
        assert all(np.isfinite(v) for v in r["dev_np"].values()) and all(np.isfinite(v) for v in r["dev_torch"].values())
        assert all(r["scale"][k] > 0 for k in bac.names(c[0])), c
