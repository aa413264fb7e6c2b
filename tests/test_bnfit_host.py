"""Re-estimating the BatchNorm statistics from the fit set: nanoreviser_amd/bnfit.py, the definition, and the command line's
--bn_reestimate on a stand-in engine (tests/bnfit_engine.py).  CPU only.
  1. stages() and inside() per depth;
  2. reestimate on a float64 set against np.mean / np.var of the same activations, stage by stage; a second call, the same bytes;
  3. with_stats changes exactly the moving_* tensors, and folded() is conv_bn / read_bn / bn_scale_shift of the model it wrote;
  4. the exact case of the device test 1: the definition's sums are math.fsum's;
  5. the cases, the bound and the seeds of tests/bnfit_cases.py;
  6. the command line: refusals, _summary.json with and without the option, the files of a run without it, -e 0 --bn_reestimate."""
import json
import math
import os

import numpy as np
import pytest

import bnfit_cases as bc
from nanoreviser_amd import bnfit, train_cli
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import lstm3fit as l3
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.weights import load_model

BN_MOVING = [4, 5, 10, 11, 20, 21, 30, 31, 42, 43]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def test_stages_and_inside_per_depth():
    assert bnfit.stages("lstm3") == (("bn_l3",),)
    assert bnfit.stages("signal") == (("bn_c1",), ("bn_c2",), ("bn_l3",))
    assert bnfit.stages("full") == (("bn_c1", "bn_l1"), ("bn_c2", "bn_l2"), ("bn_l3",))
    assert bnfit.inside("lstm3") == ("bn_l3",) and bnfit.inside("signal") == ("bn_c1", "bn_c2", "bn_l3")
    assert bnfit.inside("full") == ("bn_c1", "bn_c2", "bn_l1", "bn_l2", "bn_l3")
    assert [bnfit.BATCHNORMS[k] for k in bnfit.inside("full")] == [(2, 8), (8, 8), (18, 32), (28, 128), (40, 256)]
    for depth in ("tail", "head", "lstm4", "body"):
        with pytest.raises(ValueError, match="no BatchNorm lies inside the fitted section"):
            bnfit.stages(depth)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", bc.DEPTHS)
def test_reestimate_is_numpy_mean_and_var_stage_by_stage(depth):
    """An f64 set (the case's rows widened): the statistics against a direct np.mean / np.var of the same activations, each stage
    formed with the stages before folded in - within f64 rounding of the pivoted sums, and equal once rounded to f32 but for a last
    place."""
    T, model, n, act = 11, 1, 33, 0
    x, sig, y, th = bc.rows_case(depth, T, model, n, act)
    m, bn = bc.loaded(model)
    C = bc.n_class(model)
    rows = np.random.default_rng(2).permutation(n)[:29]
    x64, sig64 = np.asarray(x, np.float64), None if sig is None else np.asarray(sig, np.float64)
    got = bnfit.reestimate(depth, x64, sig64, th, bn, rows, T, C, act, np.float64)
    assert tuple(got) == bnfit.inside(depth)
    pairs = {k: bnfit.fold(*bn[k]) for k in bnfit.inside(depth)}
    for names in bnfit.stages(depth):
        a = bnfit.activations(depth, names, x64[rows], None if sig is None else sig64[rows], th, pairs, T, C, act, np.float64)
        for k in names:
            ch = bnfit.BATCHNORMS[k][1]
            per = 50 if k in ("bn_c1", "bn_c2") else 1
            assert a[k].shape == (29 * T * per, ch) and got[k]["n"] == 29 * T * per
            mean, var = a[k].mean(axis=0), a[k].var(axis=0)
            assert got[k]["mean"].dtype == got[k]["var"].dtype == np.float32
            assert np.allclose(got[k]["mean"], mean, rtol=2e-7, atol=1e-12) and np.allclose(got[k]["var"], var, rtol=3e-7, atol=1e-9), k       # (a constant channel away from its pivot: S2 / N - m m cancels to ~1e-12, not 0; eps is 1e-3)
            p = bn[k][2].astype(np.float64)
            assert np.allclose(got[k]["s1"], (a[k] - p).sum(axis=0), rtol=1e-12, atol=1e-9)
            pairs[k] = bnfit.fold(bn[k][0], bn[k][1], got[k]["mean"], got[k]["var"])
    again = bnfit.reestimate(depth, x64, sig64, th, bn, rows, T, C, act, np.float64)
    assert all(again[k][f].tobytes() == got[k][f].tobytes() for k in got for f in ("mean", "var", "s1", "s2"))
    # a repeated index counts twice; an empty list is refused
    twice = bnfit.reestimate(depth, x64, sig64, th, bn, np.concatenate([rows, rows]), T, C, act, np.float64)
    assert all(twice[k]["n"] == 2 * got[k]["n"] for k in got)
    with pytest.raises(ValueError):
        bnfit.reestimate(depth, x64, sig64, th, bn, [], T, C, act, np.float64)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_with_stats_changes_the_moving_tensors_only_and_folded_is_the_written_models(tmp_path):
    T, model, n, act = 11, 0, 33, 0
    x, sig, y, th = bc.rows_case("full", T, model, n, act)
    m, bn = bc.loaded(model)
    stats = bc.reference("full", T, model, n, act)["ref"]
    w = bnfit.with_stats(m, stats)
    for i in range(60):
        same = w.tensors[i].tobytes() == np.asarray(m.tensors[i]).tobytes()
        assert same == (i not in BN_MOVING), i
        assert w.tensors[i].shape == np.asarray(m.tensors[i]).shape and w.tensors[i].dtype == np.float32
    assert w.T == m.T and w.n_class == m.n_class
    part = bnfit.with_stats(m, {"bn_l3": stats["bn_l3"]})
    assert [i for i in range(60) if part.tensors[i].tobytes() != np.asarray(m.tensors[i]).tobytes()] == [42, 43]
    tf.write_f32(w, str(tmp_path / "w"))
    back = load_model(str(tmp_path / "w.f32"))
    fo = bnfit.folded(bn, stats)
    s1, h1, s2, h2 = sf.conv_bn(back)
    r1, g1, r2, g2 = ff.read_bn(back)
    sc, sh = l4.bn_scale_shift(back)
    want = {"bn_c1": (s1, h1), "bn_c2": (s2, h2), "bn_l1": (r1, g1), "bn_l2": (r2, g2), "bn_l3": (sc, sh)}
    assert set(fo) == set(want)
    for k in want:
        assert fo[k][0].tobytes() == want[k][0].tobytes() and fo[k][1].tobytes() == want[k][1].tobytes(), k
        assert np.isfinite(fo[k][0]).all() and np.isfinite(fo[k][1]).all()
    d = bnfit.drift(bn, stats)
    assert set(d) == set(want) and all(v["n"] == stats[k]["n"] for k, v in d.items())


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", [(11, 33), bc.CHUNK])
def test_the_exact_case_has_exact_sums(T, n):
    md, x2, sig, y, th = bc.dyadic_case(T, n)
    bn = bnfit.bn_of(md)
    got = bnfit.reestimate("signal", x2, sig, th, bn, np.arange(n), T, 6, 0, np.float32)["bn_c1"]
    a1 = np.maximum(sig.astype(np.float64), 0).reshape(-1)
    assert got["n"] == a1.size
    for c in range(8):
        p = float(bn["bn_c1"][2][c])
        d = a1 - p
        assert got["s1"][c] == math.fsum(d) and got["s2"][c] == math.fsum(d * d)
        assert float(got["s1"][c] * 8).is_integer() and float(got["s2"][c] * 64).is_integer()
    assert len({got["s1"][c] for c in range(8)}) > 1        # the pivots differ by channel


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_listed_ones():
    assert len(bc.CASES) == len(set(bc.CASES)) == 24
    shapes = {(c[1], c[3]) for c in bc.CASES}
    assert shapes == {(11, 1), (11, 33), (11, 160), (32, 33), (2, 4130)} and bc.CHUNK[1] == 4096 + 34
    for d in bc.DEPTHS:
        assert {(c[2], c[4]) for c in bc.CASES if c[0] == d and c[1:4:2] == (11, 33)} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_cpu_bound_of_the_device_grade_is_finite():
    small = [c for c in bc.CASES if c[1] == 11 and c[3] <= 33 and c[2] == 0]
    K, worst = bc.cpu_bound(small)
    print(f"bnfit: K = {K:.3g} over {len(small)} cases (worst restatement grade {worst:.3g}); recorded over all cases {bc.K_RECORDED}")
    assert math.isfinite(K) and K >= 2.0
    for c in small:                                         # what the device's grade is formed from exists for every BatchNorm
        r = bc.reference(*c)
        assert set(r["ref"]) == set(bnfit.inside(c[0])) == set(r["dev_np"]) == set(r["dev_torch"])
        assert all(math.isfinite(v) for how in ("dev_np", "dev_torch") for pair in r[how].values() for v in pair)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_bn_reestimate_argument_checks(tmp_path, capsys):
    d = str(tmp_path)
    base = ["-d", d, "-S", "ecoli", "-M", str(tmp_path / "out"), "--labels_from", d]
    boom = lambda *a: pytest.fail("no engine may be made for a refused command line")        # noqa: E731
    for depth in ("tail", "head", "lstm4"):
        assert train_cli.main(base + ["--fit_depth", depth, "--bn_reestimate"], reviser_factory=boom) == 2
        err = capsys.readouterr().err
        assert "--bn_reestimate" in err and "no BatchNorm lies inside the fitted section" in err and depth in err, err
    assert train_cli.main(base + ["--bn_reestimate"], reviser_factory=boom) == 2              # the default depth is tail
    capsys.readouterr()
    for depth in ("signal", "full"):
        for e in ("0", "1"):
            assert train_cli.check_args(train_cli.get_args(base + ["--fit_depth", depth, "--bn_reestimate", "-e", e])) is None
        assert train_cli.check_args(train_cli.get_args(base + ["--fit_depth", depth, "-e", "0"])) == "-e must be at least 1"
    assert "-e must be at least 1" in train_cli.check_args(train_cli.get_args(base + ["--fit_depth", "full", "--bn_reestimate", "-e", "-1"]))
    assert not train_cli.bn_reestimate(train_cli.get_args(base)) and train_cli.bn_reestimate(train_cli.get_args(base + ["--bn_reestimate"]))
    assert "--bn_reestimate" in train_cli.__doc__


def _fit_before(a_argv, eng, k, theta0, n_train, n_val):
    """fit_model as it was before --bn_reestimate existed, call for call -> the history lines."""
    a = train_cli.get_args(a_argv)
    assert train_cli.check_args(a) is None
    opts = tf.FitOpts(B=a.batch_size, lr=a.lr, lam=a.center_weight, cw=a.cw1 if k == 0 else a.cw2)
    eng.fit_begin(k, theta0, opts)
    val = np.arange(n_train, n_train + n_val, dtype=np.uint32)
    lines = []
    for ep in range(a.epochs):
        st = eng.fit_epoch(k, tf.epoch_order(n_train, a.seed, ep))
        loss, ce, cn = st.loss(opts.lam)
        sv = eng.fit_eval(k, val, want_p=False)[1]
        lines.append(f"{ep + 1}\t{loss:.6f}\t{ce:.6f}\t{cn:.6f}\t{st.acc():.6f}\t{sv.loss(opts.lam)[0]:.6f}\t{sv.acc():.6f}\t{st.nonfinite}")
    return lines


def test_train_cli_bn_reestimate_on_the_stand_in(tmp_path, monkeypatch, species_models):
    import __graft_entry__ as g
    from bnfit_engine import BnEcho
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
        made.append(BnEcho(m1.T, (m1, m2)))
        return made[-1]
    m1, m2 = species_models["ecoli"]
    T = m1.T

    def run(name, *extra):
        out = str(tmp_path / name)
        argv = ["-d", src, "-S", "ecoli", "-M", out, "-b", "512", "--labels_from", lab, "--validation_split", "0.8", "--seed", "7",
                "--fit_depth", "full", "--model_type", "model2"] + list(extra)
        assert train_cli.main(argv, reviser_factory=factory) == 0
        stem = train_cli.stem(out, "ecoli", 2)
        return argv, made[-1], stem, json.load(open(stem + "_summary.json"))

    # without the option: no entry in the summary, no call, and the files are what the command line wrote before the option existed
    argv, eng, stem, s = run("plain", "-e", "1")
    assert "bn_reestimate" not in s and eng.bn_calls == [] and eng.closed
    n = eng.fit_count()
    n_train, n_val = tf.val_split(n, 0.8)
    twin = BnEcho(T, (m1, m2))
    twin.feat, twin.sig, twin.y = eng.feat, eng.sig, eng.y
    lines = _fit_before(argv, twin, 1, ff.params_from_model(m2), n_train, n_val)
    assert open(stem + "_history.tsv", "rb").read() == (train_cli.HISTORY_HEAD + "\n" + "\n".join(lines) + "\n").encode()
    plain = load_model(stem + ".f32")
    assert plain.flat().tobytes() == ff.fitted_model(m2, twin.fit_params(1)[0], T).flat().tobytes()
    assert all(plain.tensors[i].tobytes() == m2.tensors[i].tobytes() for i in BN_MOVING)
    # with it: one call on the TRAINING rows behind fit_begin and before the first epoch; the written model carries the statistics
    argv, eng, stem, s = run("bn", "-e", "1", "--bn_reestimate")
    assert [(k, r.tolist(), t) for k, r, t in eng.bn_calls] == [(1, list(range(n_train)), 0)]
    stats = eng.fit_bn_stats(1)
    back = load_model(stem + ".f32")
    theta, t = eng.fit_params(1)
    assert t == math.ceil(n_train / 512)
    assert back.flat().tobytes() == bnfit.with_stats(ff.fitted_model(m2, theta, T), stats).flat().tobytes()
    assert all(back.tensors[i].tobytes() != m2.tensors[i].tobytes() for i in BN_MOVING)
    assert not np.array_equal(theta, twin.fit_params(1)[0])                                   # the epoch ran on the new statistics
    e = s["bn_reestimate"]
    assert list(e) == ["bn_c1", "bn_c2", "bn_l1", "bn_l2", "bn_l3"] and e == bnfit.drift(bnfit.bn_of(m2), stats)
    assert e["bn_c1"]["n"] == n_train * T * 50 and e["bn_l3"]["n"] == n_train * T
    assert all(set(v) == {"n", "max_dmean_sigma", "var_ratio_min", "var_ratio_max"} for v in e.values())
    assert s["options"]["fit_depth"] == "full" and s["train_rows"] == n_train
    # -e 0 with it: AdaBN without a fit - the loaded model with re-estimated statistics alone
    argv, eng, stem, s = run("adabn", "-e", "0", "--bn_reestimate")
    theta0 = ff.params_from_model(m2)
    assert eng.fit_params(1)[1] == 0 and eng.fit_params(1)[0].tobytes() == theta0.tobytes()
    back0 = load_model(stem + ".f32")
    assert all((back0.tensors[i].tobytes() == m2.tensors[i].tobytes()) == (i not in BN_MOVING) for i in range(60))
    assert all(back0.tensors[i].tobytes() == back.tensors[i].tobytes() for i in BN_MOVING)     # the same start, the same statistics
    assert open(stem + "_history.tsv").read().split("\n")[0] == train_cli.HISTORY_HEAD and "bn_reestimate" in s and s["options"]["epochs"] == 0
