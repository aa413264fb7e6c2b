"""The dropout behind the identity block, host side (CPU): nanoreviser_amd/dropout.py and the `drop` argument of signalfit.py /
fullfit.py; tests/dropout_cases.py holds the cases and the torch restatement.
  1. philox4x32_10 gives the three known answers;
  2. threshold and scale: rate 1e-12 keeps everything and divides by 1.0f; rate 0.2 has thr 858993459 and keepf float32(0.8);
  3. the drop fraction of the definition lies within 4 sigma of 0.2 (measured: 0.19996 .. 0.20126, at most 1.21 sigma), and the masks
     of two draws, of two models and of rows r and r + 1 differ; the mask is a function of the set row alone;
  4. a keep-everything mask with keepf 1 leaves batch_terms' bytes (that drop = None, the default, does is carried by the
     depths' own unchanged host tests, which never pass it);
  5. with a mask held fixed, directional differences of the float64 loss agree with the analytic gradient per tensor block, to
     the tolerance tests/test_fullfit_host.py uses, and autograd at float64 agrees to 1e-9;
  6. a shifted mask, or a missing division, is orders of magnitude outside the bound the device is held to;
  7. epoch: batch k drops at draw + k on its set rows and the stream advances by the number of batches;
  8. the command line refuses --dropout at --fit_depth tail, head and lstm4 and a rate outside [0, 1), by name;
  9. the command line on a stand-in engine: --dropout switches it on behind fit_set_depth with --dropout_seed (default --seed),
     the epochs are the definition's under the stream, _summary.json records rate, seed and the draw counters, and without the
     option nothing is called and nothing is recorded.
"""
import json
import math
import os

import numpy as np
import pytest

import bnfit_cases as bc
import dropout_cases as dc
from nanoreviser_amd import dropout as dr
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd import train_cli

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


# ---- 1, 2. the generator, the threshold, the scale -------------------------------------------------------------------------
def test_philox_known_answers():
    for counter, key, want in KNOWN:
        got = dr.philox4x32_10(counter, key)
        assert got.dtype == np.uint32 and " ".join("%08x" % v for v in got) == want
    both = dr.philox4x32_10([k[0] for k in KNOWN], [k[1] for k in KNOWN])         # and broadcast over leading axes
    assert [" ".join("%08x" % v for v in row) for row in both] == [k[2] for k in KNOWN]


def test_threshold_and_scale():
    assert dr.threshold(1e-12) == 0 and dr.keep_scale(1e-12) == np.float32(1.0)
    assert dr.keep_mask(7, 3, 1, [0, 5, 5, 4000000000], 3, 1e-12).all()
    assert dr.threshold(0.2) == 858993459 and dr.keep_scale(0.2) == np.float32(0.8) and dr.keep_scale(0.2).dtype == np.float32
    assert dr.threshold(0.0) == 0
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="outside"):
            dr.threshold(bad)
    with pytest.raises(ValueError, match="16 bits"):
        dr.keep_mask(1, 0, 0, [0], 656)
    assert dr.keep_mask(1, 0, 0, [0], 655).shape == (1, 655, 400)


# ---- 3. the mask -----------------------------------------------------------------------------------------------------------
def test_drop_fraction_and_independence():
    rows, T = 5 + 37 * np.arange(33), 11
    sigma = np.sqrt(0.16 / (33 * T * 400))
    masks = {}
    for draw in (0, 7, (1 << 32) + 3):
        for model in (0, 1):
            m = masks[draw, model] = dr.keep_mask(0x1234, draw, model, rows, T, 0.2)
            assert m.shape == (33, T, 400) and m.dtype == np.uint8 and m.size == 145200 and set(np.unique(m)) == {0, 1}
            frac = 1.0 - m.mean()
            print(f"draw {draw} model {model}: dropped {frac:.5f}, {(frac - 0.2) / sigma:+.2f} sigma")
            assert abs(frac - 0.2) <= 4 * sigma
    keys = list(masks)
    assert all(not np.array_equal(masks[a], masks[b]) for i, a in enumerate(keys) for b in keys[i + 1:])
    assert not np.array_equal(dr.keep_mask(0x1234, 0, 0, rows, T), dr.keep_mask(0x1234, 0, 0, rows + 1, T))
    assert not np.array_equal(dr.keep_mask(0x1234, 0, 0, rows, T), dr.keep_mask(0x1234 + (1 << 32), 0, 0, rows, T))      # the seed's high word
    assert not np.array_equal(dr.keep_mask(0x1234, 3, 0, rows, T), dr.keep_mask(0x1234, 3 + (1 << 32), 0, rows, T))      # the draw's
    # a function of the set row alone: any order, any repetition
    pick = np.array([32, 0, 0, 17])
    assert np.array_equal(dr.keep_mask(0x1234, 7, 1, rows[pick], T), masks[7, 1][pick])
    # the words of a quad serve its four elements in order
    w = dr.words(0x1234, 7, 1, rows[:1], T)
    c = [int(rows[0]), (1 << 16) | (4 * 100 + 9), 7, 0]
    assert np.array_equal(w[0, 4, 36:40], dr.philox4x32_10(c, [0x1234, 0]))


# ---- 4. drop = None --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", dc.DEPTHS)
def test_without_a_mask_the_bytes_are_the_parents(depth):
    """That a call without `drop` gives the bytes it gave before the argument existed is carried by the depths' own host tests
    (tests/test_signalfit_host.py, tests/test_fullfit_host.py), which run unchanged and never pass it: `drop` defaults to None.
    What this test adds is the dropout's own path at the point where it must be the identity: a mask of ones with keepf 1
    divides every element of F and dF by 1.0, and the bytes are still those of the call without it."""
    T, model, n = 3, 1, 5
    x, sig, y, th = bc.rows_case(depth, T, model, n, 0)
    fit, fz = (ff if depth == "full" else sf), dc.frozen(depth, model)
    opts = tf.default_opts(model)
    import inspect
    assert inspect.signature(fit.batch_terms).parameters["drop"].default is None
    assert inspect.signature(fit.epoch).parameters["drop"].default is None
    for dt in (np.float64, np.float32):
        g0, s0 = fit.batch_terms(x, sig, y, th, *fz, T, 6 - model, opts, 0, dt)
        ones = (np.ones((n, T, 400), np.uint8), np.float32(1.0))
        g2, s2 = fit.batch_terms(x, sig, y, th, *fz, T, 6 - model, opts, 0, dt, drop=ones)
        assert g0.dtype == dt and g0.tobytes() == g2.tobytes() and s0 == s2
    # and the written-out sum of the parent's formulas for sig_dense: F was not touched
    k = sf.branch(sig, th[ff.N_READ:] if depth == "full" else th, fz[-3], T, 6 - model, np.float64)
    assert np.array_equal(k["F"], sf.branch(sig, th[ff.N_READ:] if depth == "full" else th, fz[-3], T, 6 - model, np.float64, None)["F"])


# ---- 5. the gradient under a fixed mask ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.CD_CASES, ids=dc.IDS)
def test_directional_differences_under_a_fixed_mask(case):
    depth, T, model, n = case
    x, sig, y, th, rows, drop, _ = dc.batch_case(*case)
    assert 0 < drop[0].mean() < 1
    g, st = dc.definition(depth, x, sig, y, th, T, model, drop, np.float64)
    opts = tf.default_opts(model)

    def loss(theta):
        s = dc.definition(depth, x, sig, y, theta, T, model, drop, np.float64)[1]
        return (s.ce_sum + float(np.float32(opts.lam)) * s.center_sum) / n
    rng = np.random.default_rng(1)
    th64 = th.astype(np.float64)
    sp = dc.spans(depth, T, 6 - model)
    blocks = (("W1f", "U2b", "b2f") if depth == "full" else ()) + ("cw1", "cb1", "cw2", "cb2", "Ws", "bs", "W3f", "b3b")
    for k in blocks:
        s = sp[k]
        v = np.zeros_like(th64)
        v[s] = rng.normal(0, 1, s.stop - s.start)
        v /= np.linalg.norm(v)
        h = 1e-6
        num = (loss(th64 + h * v) - loss(th64 - h * v)) / (2 * h)
        want = float(g @ v)
        assert abs(num - want) <= 1e-5 * max(abs(want), np.linalg.norm(g[s])) + 1e-10, (k, num, want)
    # autograd at float64 on the restatement with the same mask
    gt, ce, cn, ok = dc.torch_terms(depth, x, sig, y, th, T, model, drop, np.float64)
    for k, s in sp.items():
        scale = np.abs(gt[s]).max()
        assert np.abs(g[s] - gt[s]).max() <= 1e-9 * scale, (k, np.abs(g[s] - gt[s]).max(), scale)
    assert st.correct == ok and abs(st.ce_sum - ce) <= 1e-9 * ce and abs(st.center_sum - cn) <= 1e-9 * cn
    # the mask matters: the gradient without it is another one
    g0 = dc.definition(depth, x, sig, y, th, T, model, None, np.float64)[0]
    assert np.abs(g0[sp["Ws"]] - g[sp["Ws"]]).max() > 1e-3 * np.abs(g[sp["Ws"]]).max()


# ---- 6. what the bound catches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("signal", 3, 1, 33), ("full", 11, 0, 33)], ids=dc.IDS)
def test_a_shifted_mask_or_a_missing_division_is_far_outside(case):
    depth, T, model, n = case
    K, worst = dc.cpu_bound([case])
    x, sig, y, th, rows, drop, _ = dc.batch_case(*case)
    ref = dc.graded(case)
    mask, keepf = drop
    shifted = (dr.keep_mask(dc.SEED, dc.DRAW, model, np.arange(n), T, dc.RATE), keepf)          # the batch position for the set row
    for name, bad in (("position for row", shifted), ("no division", (mask, np.float32(1.0))), ("another draw", (dr.keep_mask(dc.SEED, dc.DRAW + 1, model, rows, T, dc.RATE), keepf))):
        g, st = dc.definition(depth, x, sig, y, th, T, model, bad, np.float64)
        gr = dc.grades(g, st.ce_sum, st.center_sum, ref)
        print(case, name, "K", round(K, 2), "Ws", f"{gr['Ws']:.3g}", "cw2", f"{gr['cw2']:.3g}", "worst", f"{max(gr.values()):.3g}")
        assert gr["Ws"] > 1000 * K and gr["cw2"] > 1000 * K, (name, gr)
    # the dropped forward is zero exactly where the mask is
    F = sf.branch(sig, th[ff.N_READ:] if depth == "full" else th, dc.frozen(depth, model)[-3], T, 6 - model, np.float64, drop)["F"]
    assert (F[mask == 0] == 0).all() and (F[mask != 0] != 0).any()


# ---- 7. epoch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", dc.DEPTHS)
def test_epoch_draws_per_batch_and_advances(depth):
    T, model, n, B = 3, 0, 7, 3
    x, sig, y, th = bc.rows_case(depth, T, model, n, 0)
    fit, fz = (ff if depth == "full" else sf), dc.frozen(depth, model)
    opts = tf.default_opts(model, B=B)
    order = np.array([6, 2, 0, 5, 1, 3, 4])
    s1 = tf.FitState(th.astype(np.float64), np.zeros(th.size), np.zeros(th.size), 0)
    stream = dr.Stream(0.2, 99, model, draw=4)
    fit.epoch(x, sig, y, s1, order, *fz, T, 6 - model, opts, 0, np.float64, drop=stream)
    assert stream.draw == 4 + 3 and s1.t == 3
    # by hand: batch k at draw 4 + k on its own set rows
    s2 = tf.FitState(th.astype(np.float64), np.zeros(th.size), np.zeros(th.size), 0)
    for k in range(3):
        idx = order[k * B:(k + 1) * B]
        g, _ = fit.batch_terms(x[idx], sig[idx], y[idx], s2.theta, *fz, T, 6 - model, opts, 0, np.float64,
                               drop=dr.terms(99, 4 + k, model, idx, T, 0.2))
        s2.t += 1
        s2.theta, s2.m, s2.v = tf.adam_step(s2.theta, s2.m, s2.v, g, opts, s2.t, np.dtype(np.float64))
    assert s1.theta.tobytes() == s2.theta.tobytes()
    # split in two calls: the same parameters and the same draw
    s3 = tf.FitState(th.astype(np.float64), np.zeros(th.size), np.zeros(th.size), 0)
    st3 = dr.Stream(0.2, 99, model, draw=4)
    fit.epoch(x, sig, y, s3, order[:B], *fz, T, 6 - model, opts, 0, np.float64, drop=st3)
    fit.epoch(x, sig, y, s3, order[B:], *fz, T, 6 - model, opts, 0, np.float64, drop=st3)
    assert s3.theta.tobytes() == s1.theta.tobytes() and st3.draw == stream.draw
    # evaluate never drops: it has no such argument
    import inspect
    assert "drop" not in inspect.signature(fit.evaluate).parameters
    from nanoreviser_amd import bnfit
    assert all("drop" not in inspect.signature(f).parameters for f in vars(bnfit).values() if inspect.isfunction(f))


# ---- 8. the command line ---------------------------------------------------------------------------------------------------
def test_command_line_refusals(tmp_path, capsys):
    base = ["-d", str(tmp_path), "--labels_from", str(tmp_path), "-M", str(tmp_path / "out")]
    for depth in ("tail", "head", "lstm4"):
        assert train_cli.main(base + ["--fit_depth", depth, "--dropout", "0.2"]) == 2
        err = capsys.readouterr().err
        assert f"--dropout: the signal branch is frozen at --fit_depth {depth}, there is nothing to drop (signal and full fit it)" in err
    for rate in ("1.0", "-0.1", "nan", "1.5"):
        for depth in ("signal", "full", "tail"):
            assert train_cli.main(base + ["--fit_depth", depth, "--dropout", rate]) == 2
            assert "--dropout must be in [0, 1)" in capsys.readouterr().err
    a = train_cli.get_args(base + ["--fit_depth", "signal", "--dropout", "0.2"])
    assert train_cli.check_args(a) is None and train_cli.dropout_rate(a) == a.dropout == 0.2 and not hasattr(a, "dropout_seed")
    a = train_cli.get_args(base + ["--fit_depth", "tail"])
    assert train_cli.check_args(a) is None and train_cli.dropout_rate(a) == 0.0     # off by default, at every depth
    assert not hasattr(a, "dropout")                                                # (in the namespace only when given)
    import io
    from contextlib import redirect_stdout
    buf = io.StringIO()
    with pytest.raises(SystemExit), redirect_stdout(buf):
        train_cli.get_args(["--help"])
    assert "0.2 is the reference's rate" in " ".join(buf.getvalue().split())


# ---- 9. the command line on a stand-in -------------------------------------------------------------------------------------
def _drop_echo():
    from fullfit_engine import FullEcho

    class DropEcho(FullEcho):
        """tests/fullfit_engine.py's stand-in with the nrv_fit_set_dropout surface: the epochs are fullfit.epoch at float32 under a
        dropout.Stream at the model's draw; evaluation is the parent's and never drops."""

        def __init__(self, T, models=None):
            super().__init__(T, models)
            self.rate, self.seed, self.draws, self.drop_calls = 0.0, 0, [0, 0], []

        def fit_reset(self):
            keep = (self.rate, self.seed, self.draws, self.drop_calls)
            super().fit_reset()
            self.rate, self.seed, self.draws, self.drop_calls = keep

        def fit_set_depth(self, depth):
            super().fit_set_depth(depth)
            self.rate, self.draws = 0.0, [0, 0]

        def fit_set_dropout(self, rate, seed=0):
            assert 0.0 <= rate < 1.0
            self.rate, self.seed, self.draws = float(rate), int(seed), [0, 0]
            self.drop_calls.append((self.rate, self.seed, self.fit_count(), self.depth))

        def fit_dropout(self):
            return self.rate, self.seed, tuple(self.draws)

        def fit_begin(self, model, params=None, opts=None):
            super().fit_begin(model, params, opts)
            self.draws[model] = 0

        def fit_epoch(self, model, order):
            if not self.rate:
                return super().fit_epoch(model, order)
            stream = dr.Stream(self.rate, self.seed, model, self.draws[model])
            st = ff.epoch(self.feat, self.sig, self.y[model], self.state[model], order, *self._frozen(model), self.T, 6 - model,
                          self.opts[model], 0, np.float32, drop=stream)
            self.draws[model] = stream.draw
            return st
    return DropEcho


def test_command_line_on_a_stand_in(species_models, tmp_path, monkeypatch):
    import __graft_entry__ as g
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
    DropEcho = _drop_echo()
    made = []

    def factory(a, m1, m2):
        made.append(DropEcho(m1.T, (m1, m2)))
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

    eng, stem, s = run("drop", "--dropout", "0.2")
    n_train, _ = tf.val_split(eng.fit_count(), 0.8)
    nb = math.ceil(n_train / 512)
    assert eng.drop_calls == [(0.2, 7, 0, 32)]             # behind fit_set_depth, on the empty set, seeded by --seed
    assert s["options"]["dropout"] == 0.2 and s["options"]["dropout_seed"] == 7
    assert s["dropout"] == {"rate": 0.2, "seed": 7, "draw": [0, nb]}
    theta = eng.fit_params(1)[0]
    twin = DropEcho(T, (m1, m2))
    twin.fit_set_depth("full")
    twin.fit_set_dropout(0.2, 7)
    twin.feat, twin.sig, twin.y = eng.feat, eng.sig, eng.y
    twin.fit_begin(1, ff.params_from_model(m2), tf.FitOpts(B=512, lr=1e-3, lam=tf.LAMBDA, cw=tf.CW2))
    twin.fit_epoch(1, tf.epoch_order(n_train, 7, 0))
    assert twin.fit_params(1)[0].tobytes() == theta.tobytes() and twin.fit_dropout()[2] == (0, nb)
    a = train_cli.get_args(["--dropout", "0.2", "--dropout_seed", "11", "--seed", "7"])
    assert a.dropout_seed == 11 and a.seed == 7
    # without the option: nothing is called, nothing is recorded, and the epoch is the stand-in's own
    plain, _, s0 = run("plain")
    assert plain.drop_calls == [] and plain.fit_dropout() == (0.0, 0, (0, 0))
    assert "dropout" not in s0 and "dropout" not in s0["options"] and "dropout_seed" not in s0["options"]
    assert plain.fit_params(1)[0].tobytes() != theta.tobytes()
