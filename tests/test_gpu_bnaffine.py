"""Fitting gamma and beta of the BatchNorms inside the fitted section on the device (MI355X only, -m gpu): csrc/nrv_bnaffine.h through
nrv_fit_set_bn_affine and the nrv_fit_* entry points.  nanoreviser_amd/bnaffine.py is the definition; tests/bnaffine_cases.py holds
the cases, the two f32 restatements and the floors.  Every tolerance is sized from CPU restatements against the float64 definition.
  1. doors: refusals by whole string at tail / head / lstm4 and in flight; parameter counts at the three depths; nrv_fit_set_depth
     switches it off; nrv_fit_begin is forgotten;
  2. switch on, params NULL (also under NRV_POISON): the front of nrv_fit_params is the model's gamma / beta; nrv_fit_eval's p and
     statistics and nrv_fit_grad behind the block are the switch-off call's BYTES on the same rows; the same call twice gives the
     same bytes;
  3. the gamma / beta gradient, per tensor, within cpu_bound() AND K_RECORDED of the float64 definition: T = 1 with one row, T = 3
     with a short last tile, T = 11 with two tiles for both models and gate functions, a gamma channel of 0, every beta 0, and one
     batch of 4130 rows (a full scratch chunk and a short tile);
  4. one update = tailfit_cases.adam_f32 on nrv_fit_grad's vector, byte for byte; afterwards nrv_fit_eval equals, byte for byte,
     nrv_fit_eval of a fit begun afresh with the stepped vector, and differs from the value before the step: the refold;
  5. a row holding inf: counted in nonfinite, parameters and eval bytes kept;
  6. nrv_fit_bn_reestimate after one update: within tests/test_gpu_bnfit.py's bound of bnfit.reestimate fed the CURRENT gamma /
     beta, the vector's bytes untouched, and later refolds use the new statistics;
  7. it learns: from the shipped model with gamma x 1.3 and beta + 0.2 on every BatchNorm inside, the loss falls, and
     bnaffine.fitted_model in a NEW handle gives nrv_fit_eval's bytes with the switch off;
  8. after the switch has been used, switch-off nrv_fit_grad at signal and full depth gives a fresh handle's bytes;
  9. the command line: NanoReviser_train.py --fit_depth signal --fit_bn_affine -e 1 writes a directory NanoReviser.py --model_dir runs.

Worst device grade seen on an MI355X: see DESIGN section 15."""
import numpy as np
import pytest

import bnaffine_cases as bac
import bnfit_cases as bc
import tailfit_cases as tc
from nanoreviser_amd import bnaffine as ba
from nanoreviser_amd import bnfit, fitdepth
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import tailfit as tf
from test_gpu_bnfit import ACT_NAME, _load, _reviser
from test_gpu_fullfit import ENV, PATTERNS
from test_gpu_headfit import _all_rows, _args, _pack

pytestmark = pytest.mark.gpu

REFUSED_NO_BN = ("nrv_fit_set_bn_affine: no BatchNorm lies inside the fitted section (depths NRV_FIT_LSTM3, NRV_FIT_SIGNAL and NRV_FIT_FULL "
                 "have one)")
REFUSED_IN_FLIGHT = "nrv_fit_set_bn_affine: a raw-read call is in flight (collect it with nrv_reads_raw_end first)"


@pytest.fixture(scope="module")
def handles(species_models):
    """One handle per (window length, recurrent_act) of the shipped ecoli models, made on first use and shared."""
    from nanoreviser_amd.engine import Reviser
    made = {}

    def get(T, act=0):
        if (T, act) not in made:
            m1, m2 = species_models["ecoli"]
            made[T, act] = Reviser(m1.with_window(T), m2.with_window(T), recurrent_activation=ACT_NAME[act])
        return made[T, act]
    yield get
    for rv in made.values():
        rv.close()


@pytest.fixture(scope="module")
def short_reads(reads):
    out = []
    for k in reads.keys:
        _, rd, _ = reads(k)
        out.append(hs.read_tensors_raw(rd))
    return sorted(out, key=lambda r: len(r.starts))[:2]


@pytest.fixture(scope="module")
def grade_bound():
    K, worst = bac.cpu_bound()
    print(f"bnaffine: bound sized on the CPU: K = {K:.3g} (worst restatement grade {worst:.3g}); recorded {bac.K_RECORDED}")
    return K


def _on(rv, depth, model, x, sig, y, on=True):
    """The case's rows at `depth` with the switch set (nrv_fit_set_depth has switched it off)."""
    _load(rv, depth, model, x, sig, y)
    assert not rv.fit_bn_affine()
    if on:
        rv.fit_set_bn_affine(True)
    assert rv.fit_bn_affine() == on


# ---- 1. doors --------------------------------------------------------------------------------------------------------------
def test_doors_refusals_counts_and_forgetting(species_models, short_reads, monkeypatch):
    rv = _reviser(monkeypatch, *species_models["ecoli"], precision="f32")
    lib, h = rv._lib, rv._h
    try:
        assert lib.nrv_fit_bn_affine(h) == 0
        for depth in ("tail", "head", "lstm4"):
            rv.fit_set_depth(depth)
            assert lib.nrv_fit_set_bn_affine(h, 1) == -1 and lib.nrv_last_error(h).decode() == REFUSED_NO_BN
            assert lib.nrv_fit_set_bn_affine(h, 0) == 0 and lib.nrv_fit_bn_affine(h) == 0       # off is what it is
            assert rv.fit_n_params(0) == fitdepth.BY_NAME[depth].fit.n_params(11, 6)
        for depth, nb in (("lstm3", 512), ("signal", 544), ("full", 864)):
            rv.fit_set_depth(depth)
            fit = fitdepth.BY_NAME[depth].fit
            for k, C in ((0, 6), (1, 5)):
                assert rv.fit_n_params(k) == fit.n_params(11, C)
            rv.fit_set_bn_affine(True)
            assert lib.nrv_fit_bn_affine(h) == 1 and rv.fit_depth() == fitdepth.CODES[depth]
            for k, C in ((0, 6), (1, 5)):
                assert rv.fit_n_params(k) == nb + fit.n_params(11, C) == ba.n_params(depth, 11, C)
            with pytest.raises(ValueError, match="expected"):                                      # the other length is not taken
                rv.fit_begin(0, np.zeros(fit.n_params(11, 6), np.float32))
            rv.fit_set_depth(depth)                          # the same depth again: switched off
            assert lib.nrv_fit_bn_affine(h) == 0 and rv.fit_n_params(0) == fit.n_params(11, 6)
        # with rows in the set, and nrv_fit_begin of both models forgotten either way
        x, sig, y, vec, stats = bac.rows_case("signal", 11, 0, 33, 0, "plain")
        _load(rv, "signal", 0, x, sig, y)
        for k in (0, 1):
            rv.fit_begin(k)
        for on in (True, True, False):
            rv.fit_set_bn_affine(on)
            assert rv.fit_count() == 33 and rv.fit_bn_affine() == on
            for k in (0, 1):
                assert lib.nrv_fit_params(h, k, None, None) == -1
                assert lib.nrv_last_error(h).decode() == "nrv_fit_params: no fit in progress for this model (call nrv_fit_begin first)"
                rv.fit_begin(k)
                assert rv.fit_params(k)[0].size == rv.fit_n_params(k) == (544 if on else 0) + fitdepth.BY_NAME["signal"].fit.n_params(11, 6 - k)
        rv.fit_set_bn_affine(True)
        rv.fit_begin(0, vec)
        g, st = rv.fit_grad(0, np.arange(33))
        t = rv.begin_packed_raw(_pack(rv, short_reads[:1]))  # between a _begin and its _end
        for on in (0, 1):
            assert lib.nrv_fit_set_bn_affine(h, on) == -1 and lib.nrv_last_error(h).decode() == REFUSED_IN_FLIGHT
        rv.end_packed_raw(t)
        assert rv.fit_bn_affine()                            # every refusal left the handle usable and the fit alone
        g2, st2 = rv.fit_grad(0, np.arange(33))
        assert g2.tobytes() == g.tobytes() and st2 == st
    finally:
        rv.close()


# ---- 2. switch on, params NULL ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", bac.DEPTHS)
@pytest.mark.parametrize("poison", [None] + sorted(PATTERNS))
def test_switch_on_from_the_handles_own_is_the_switch_off_bytes(species_models, monkeypatch, depth, poison):
    T, model, n, act = 11, 1, 33, 0
    x, sig, y, _, _ = bac.rows_case(depth, T, model, n, act, "plain")
    m1, m2 = species_models["ecoli"]
    rv = _reviser(monkeypatch, m1, m2, poison=poison)
    try:
        rows = np.arange(n)
        nb = ba.n_block(depth)
        _on(rv, depth, model, x, sig, y, on=False)
        rv.fit_begin(model)
        th_off = rv.fit_params(model)[0]
        g_off, s_off = rv.fit_grad(model, rows)
        p_off, e_off = rv.fit_eval(model, rows)
        rv.fit_set_bn_affine(True)
        rv.fit_begin(model)
        vec = rv.fit_params(model)[0]
        assert vec.tobytes() == ba.params_from_model(depth, m2).tobytes() and vec[nb:].tobytes() == th_off.tobytes()
        g_on, s_on = rv.fit_grad(model, rows)
        p_on, e_on = rv.fit_eval(model, rows)
        assert p_on.tobytes() == p_off.tobytes() and e_on == e_off                  # the device fold is nrv_create's, bit for bit
        assert g_on[nb:].tobytes() == g_off.tobytes() and s_on == s_off
        assert np.isfinite(g_on[:nb]).all() and all(g_on[s].any() for s in bac.spans(depth).values())
        g2, s2 = rv.fit_grad(model, rows)
        p2, e2 = rv.fit_eval(model, rows)
        assert g2.tobytes() == g_on.tobytes() and s2 == s_on and p2.tobytes() == p_on.tobytes() and e2 == e_on
    finally:
        rv.close()


# ---- 3. the gradient -------------------------------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("case", bac.CASES + bac.CHUNK_CASES, ids=bac.IDS)
def test_gamma_beta_gradient_against_the_definition(handles, grade_bound, case):
    depth, T, model, n, act, variant = case
    x, sig, y, vec, stats = bac.rows_case(*case)
    rv = handles(T, act)
    _on(rv, depth, model, x, sig, y)
    rv.fit_begin(model, vec)
    g, st = rv.fit_grad(model, np.arange(n))
    r = bac.reference(*case)
    assert g.size == vec.size and np.isfinite(g).all() and (st.rows, st.nonfinite, st.correct) == (n, 0, r["st64"].correct)
    gr = bac.device_grades(g, r, depth)
    for k, v in gr.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(case, {k: round(v, 3) for k, v in gr.items()}, "bounds", round(grade_bound, 3), bac.K_RECORDED,
          "worst so far", {k: round(v, 3) for k, v in WORST.items()})
    assert max(gr.values()) <= grade_bound, gr
    assert max(gr.values()) <= bac.K_RECORDED, gr
    # the rest of the vector's gradient is what the switch-off call gives on the same pairs: the block changes no other launch's sums
    nb = ba.n_block(depth)
    rv.fit_set_bn_affine(False)
    rv.fit_begin(model, vec[nb:])
    if variant == "plain":                                  # (the variants' pairs are not the handle's)
        g_off, st_off = rv.fit_grad(model, np.arange(n))
        assert g[nb:].tobytes() == g_off.tobytes() and st == st_off


# ---- 4. one update and the refold ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(d, 11, 1, 33, 0, "plain") for d in bac.DEPTHS] + [("full", 1, 0, 1, 0, "plain")], ids=bac.IDS)
def test_one_step_is_numpy_f32_adam_and_the_pairs_are_refolded(handles, case):
    depth, T, model, n, act, variant = case
    x, sig, y, vec, stats = bac.rows_case(*case)
    rv = handles(T, act)
    _on(rv, depth, model, x, sig, y)
    opts = tf.default_opts(model)
    rows = np.arange(n)
    rv.fit_begin(model, vec, opts)
    p_before, e_before = rv.fit_eval(model, rows)
    g, _ = rv.fit_grad(model, rows)
    st = rv.fit_epoch(model, rows)
    got, t = rv.fit_params(model)
    want = tc.adam_f32(vec, np.zeros_like(vec), np.zeros_like(vec), g, opts, 1)[0]
    assert (t, st.steps, st.rows, st.nonfinite) == (1, 1, n, 0)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8].tolist()
    assert all(not np.array_equal(got[s], vec[s]) for s in bac.spans(depth).values())              # every gamma and beta moved
    p_after, e_after = rv.fit_eval(model, rows)
    rv.fit_begin(model, got, opts)                           # afresh from the stepped vector: folded by nrv_fit_begin
    p_fresh, e_fresh = rv.fit_eval(model, rows)
    assert p_after.tobytes() == p_fresh.tobytes() and e_after == e_fresh
    assert p_after.tobytes() != p_before.tobytes()
    # and the pairs behind the step are the definition's fold of the stepped gamma / beta: its f32 evaluation agrees
    p32 = ba.evaluate(depth, x, sig, y, got, rows, stats, T, 6 - model, opts, act, np.float64)[0]
    assert np.abs(p_after - p32).max() <= 64 * tc.EPS32


# ---- 5. a non-finite batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", bac.DEPTHS)
def test_nonfinite_batch_is_counted_and_changes_nothing(handles, depth):
    T, model, n, act = 11, 0, 33, 0
    x, sig, y, vec, stats = bac.rows_case(depth, T, model, n, act, "plain")
    x, sig = np.array(x), None if sig is None else np.array(sig)
    (x if depth == "lstm3" else sig)[20, 3, 2] = np.inf
    rv = handles(T, act)
    _on(rv, depth, model, x, sig, y)
    opts = tf.default_opts(model, B=16)
    rv.fit_begin(model, vec, opts)
    clean = np.arange(16)
    p0, e0 = rv.fit_eval(model, clean)
    st = rv.fit_epoch(model, np.arange(16, 32))              # the batch with the row alone
    got, t = rv.fit_params(model)
    assert (t, st.steps, st.nonfinite, st.rows) == (0, 0, 1, 0) and got.tobytes() == vec.tobytes()
    p1, e1 = rv.fit_eval(model, clean)
    assert p1.tobytes() == p0.tobytes() and e1 == e0         # the refold behind a skipped update left the pairs' bytes
    g, sg = rv.fit_grad(model, np.arange(16, 32))
    assert sg.nonfinite == 1 and not np.isfinite(g).all()
    st = rv.fit_epoch(model, np.arange(n))                   # batches of 16, 16 (skipped), 1
    got, t = rv.fit_params(model)
    assert (t, st.steps, st.nonfinite, st.rows) == (2, 2, 1, 17) and np.isfinite(got).all()
    rv.fit_begin(model, vec, opts)
    rv.fit_epoch(model, np.r_[np.arange(16), 32])
    assert rv.fit_params(model)[0].tobytes() == got.tobytes()


# ---- 6. re-estimation with the switch on -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bnfit_bound():
    return bc.cpu_bound()[0]


@pytest.mark.parametrize("depth", bac.DEPTHS)
def test_reestimate_folds_with_the_current_gamma_and_beta(handles, bnfit_bound, depth):
    T, model, n, act = 11, 0, 33, 0
    case = (depth, T, model, n, act)
    x, sig, y, vec, stats = bac.rows_case(*case, "plain")
    rv = handles(T, act)
    _on(rv, depth, model, x, sig, y)
    opts = tf.default_opts(model, lr=0.01)                   # a step large enough for the stages behind to see the new gamma / beta
    rows = np.arange(n)
    rv.fit_begin(model, vec, opts)
    rv.fit_epoch(model, rows)
    cur, t = rv.fit_params(model)
    got = rv.fit_bn_reestimate(model, rows)
    again, t2 = rv.fit_params(model)
    assert again.tobytes() == cur.tobytes() and t2 == t == 1                      # gamma, beta and t untouched
    nb = ba.n_block(depth)
    gb, theta = ba.unpack(depth, cur, T, 6)
    _, loaded = bc.loaded(model)
    bn_cur = {k: (gb[k] if k in gb else v[:2]) + v[2:] for k, v in loaded.items()}   # the CURRENT gamma / beta, the loaded pivot
    C = 6
    ref = bnfit.reestimate(depth, x, sig, theta, bn_cur, rows, T, C, act, np.float64)
    r_np = bnfit.reestimate(depth, x, sig, theta, bn_cur, rows, T, C, act, np.float32)
    r_t = bnfit.reestimate(depth, x, sig, theta, bn_cur, rows, T, C, act, np.float32, acts=bc.torch_activations)
    scale = {k: (float(np.max(np.abs(r["mean"].astype(np.float64)) / np.sqrt(r["var"].astype(np.float64) + 1e-3))), 1.0) for k, r in ref.items()}
    r = {"ref": ref, "dev_np": bc.deviations(r_np, ref), "dev_torch": bc.deviations(r_t, ref), "scale": scale}
    g = bc.grades(got, r)
    print(depth, {f"{k}.{w}": round(v, 3) for (k, w), v in g.items()}, "bounds", round(bnfit_bound, 3), bc.K_RECORDED)
    assert max(g.values()) <= bnfit_bound, g                 # tests/test_gpu_bnfit.py's two bounds
    assert max(g.values()) <= bc.K_RECORDED, g
    if depth != "lstm3":                                     # with the LOADED gamma / beta the stages behind the first differ
        old = bnfit.reestimate(depth, x, sig, theta, loaded, rows, T, C, act, np.float64)
        assert max(bc.grades({k: old[k] for k in got}, r).values()) > bc.K_RECORDED
    # later refolds use the new statistics: nrv_fit_eval is the definition's on them, and stays so behind another update
    new_stats = dict(stats)
    new_stats.update({k: (v["mean"], v["var"]) for k, v in got.items()})
    p, _ = rv.fit_eval(model, rows)
    assert np.abs(p - ba.evaluate(depth, x, sig, y, cur, rows, new_stats, T, C, opts, act, np.float64)[0]).max() <= 64 * tc.EPS32
    assert np.abs(p - ba.evaluate(depth, x, sig, y, cur, rows, stats, T, C, opts, act, np.float64)[0]).max() > 64 * tc.EPS32
    rv.fit_epoch(model, rows)
    nxt = rv.fit_params(model)[0]
    p2, _ = rv.fit_eval(model, rows)
    assert np.abs(p2 - ba.evaluate(depth, x, sig, y, nxt, rows, new_stats, T, C, opts, act, np.float64)[0]).max() <= 64 * tc.EPS32


# ---- 7. it learns ----------------------------------------------------------------------------------------------------------
LEARN_E = 4


@pytest.mark.parametrize("depth", ["signal", "full"])
def test_it_learns_and_the_written_model_gives_the_fits_bytes(species_models, short_reads, monkeypatch, tmp_path, depth):
    """The shipped ecoli model with gamma x 1.3 and beta + 0.2 on every BatchNorm inside, every window of the two shortest fixture
    reads labelled with the answers the UNPERTURBED model gives in f32 mode, LEARN_E epochs at the defaults."""
    from nanoreviser_amd.engine import Reviser
    from nanoreviser_amd.weights import load_model
    m1, m2 = species_models["ecoli"]
    el = [len(r.starts) for r in short_reads]
    labels = np.full(sum(el), 5, np.uint8)
    w = tf.labelled_windows(labels, el, 11)[0]
    teacher = Reviser(m1, m2, precision="f32")
    _, _, a1, a2 = teacher.predict_reads_raw(*_args(short_reads))
    teacher.close()
    y1, y2 = a1[w].astype(np.uint8), a2[w].astype(np.uint8)
    rv = _reviser(monkeypatch, m1, m2)
    rv.fit_set_depth(depth)
    rv.fit_set_bn_affine(True)
    n = rv.fit_add_packed(_pack(rv, short_reads), labels)
    assert n == w.size and n > 300
    got = rv.fit_get_rows_full() if depth == "full" else rv.fit_get_rows_signal()
    (rv.fit_set_rows_full if depth == "full" else rv.fit_set_rows_signal)(*got[:-2], y1, y2)
    k, m = 0, m1
    nb = ba.n_block(depth)
    start = ba.params_from_model(depth, m)
    for sg, sb in ba.spans(depth).values():
        start[sg] *= np.float32(1.3)
        start[sb] += np.float32(0.2)
    rv.fit_begin(k, start, tf.default_opts(k))
    rows = _all_rows(rv)
    before = rv.fit_eval(k, rows, want_p=False)[1].loss()[0]
    hist = [rv.fit_epoch(k, tf.epoch_order(n, 3, ep)) for ep in range(LEARN_E)]
    p_fit, e_fit = rv.fit_eval(k, rows)
    after = e_fit.loss()[0]
    loss = [h.loss()[0] for h in hist]
    print(f"{depth}: loss before {before:.4f}, epochs {loss[0]:.4f} -> {loss[-1]:.4f}, after {after:.4f}")
    assert all(h.nonfinite == 0 for h in hist) and loss[-1] < loss[0] and after < before
    theta, t = rv.fit_params(k)
    assert all(not np.array_equal(theta[s], start[s]) for pair in ba.spans(depth).values() for s in pair)
    fm = ba.fitted_model(depth, m, theta)
    tf.write_f32(fm, str(tmp_path / "m"))
    rv.close()
    back = load_model(str(tmp_path / "m.f32"))
    rv2 = _reviser(monkeypatch, back, m2)
    try:
        rv2.fit_set_depth(depth)
        (rv2.fit_set_rows_full if depth == "full" else rv2.fit_set_rows_signal)(*got[:-2], y1, y2)
        rv2.fit_begin(k, theta[nb:], tf.default_opts(k))     # switch off: gamma / beta are the file's, folded by nrv_create
        p2, e2 = rv2.fit_eval(k, rows)
        assert p2.tobytes() == p_fit.tobytes() and e2 == e_fit
    finally:
        rv2.close()


# ---- 8. the switch leaves nothing behind -----------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", ["signal", "full"])
def test_switch_off_gives_a_fresh_handles_bytes_after_the_switch_was_used(species_models, handles, monkeypatch, depth):
    T, model, n, act = 11, 1, 33, 0
    x, sig, y, vec, stats = bac.rows_case(depth, T, model, n, act, "plain")
    nb = ba.n_block(depth)
    used = handles(T, act)
    _on(used, depth, model, x, sig, y)
    used.fit_begin(model, vec, tf.default_opts(model))
    used.fit_epoch(model, np.arange(n))
    used.fit_bn_reestimate(model, np.arange(n))
    used.fit_set_bn_affine(False)
    used.fit_begin(model, vec[nb:])
    g_used, st_used = used.fit_grad(model, np.arange(n))
    fresh = _reviser(monkeypatch, *species_models["ecoli"])
    try:
        _load(fresh, depth, model, x, sig, y)
        fresh.fit_begin(model, vec[nb:])
        g_fresh, st_fresh = fresh.fit_grad(model, np.arange(n))
    finally:
        fresh.close()
    assert g_used.tobytes() == g_fresh.tobytes() and st_used == st_fresh


# ---- 9. command line -------------------------------------------------------------------------------------------------------
def test_command_line_fits_gamma_and_beta_and_model_dir_runs_the_result(tmp_path, monkeypatch, species_models):
    """tests/test_gpu_fullfit.py's command-line run with --fit_depth signal --fit_bn_affine: --labels, NanoReviser_train.py -e 1, then
    NanoReviser.py --model_dir on the written directory in every precision mode."""
    import glob
    import json
    import os
    import shutil
    from conftest import GOLD
    from nanoreviser_amd import cli, train_cli
    from nanoreviser_amd.engine import Reviser
    from nanoreviser_amd.weights import load_model
    from test_gpu_infix import mutate, random_seq
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_SUMMARY",
              "NRV_TRIM_Q", "NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES", "NRV_INFIX", "NRV_LABELS", "NRV_LABELS_BUDGET", "NRV_SCORE",
              "NRV_LABELS_FROM", "NRV_CLI_GROUPS") + ENV:
        monkeypatch.delenv(k, raising=False)
    d = tmp_path / "in"
    d.mkdir()
    src = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")))
    for i in range(2):
        shutil.copy(src[i % len(src)], d / f"s{i:02d}.fast5")
    fa, ldir, out = str(tmp_path / "regions.fa"), str(tmp_path / "labels"), str(tmp_path / "plain") + "/"
    common = ["-d", str(d), "-S", "ecoli", "--gpus", "1", "--thread", "2"]
    assert cli.main(common + ["-o", out]) == 0
    rng = np.random.default_rng(8)
    with open(fa, "w") as fp:                              # the regions: a seeded 5 % mutation of what the plain run wrote, between flanks
        for i in range(2):
            t = (random_seq(rng, 64 + i) + mutate(rng, open(out + f"s{i:02d}_out.fasta", "rb").read().split(b"\n")[1], 0.05) + random_seq(rng, 80)).decode()
            fp.write(f">s{i:02d}\n" + "".join(t[k:k + 70] + "\n" for k in range(0, len(t), 70)))
    assert cli.main(common + ["-o", str(tmp_path / "A") + "/", "--device_merge", "--truth", fa, "--infix", str(tmp_path / "A.inf"), "--labels", ldir]) == 0
    mdir = str(tmp_path / "model")
    made = []

    class Kept(Reviser):                                   # the command line's own engine, kept open behind its close()
        def close(self):
            pass

    def factory(a, m1, m2):
        made.append(Kept(m1, m2, device=0))
        return made[-1]
    assert train_cli.main(["-d", str(d), "-S", "ecoli", "-M", mdir, "-e", "1", "--fit_depth", "signal", "--fit_bn_affine", "--labels_from", ldir],
                          reviser_factory=factory) == 0
    rv = made[0]
    inside = [2, 3, 8, 9, 40, 41]
    try:
        assert rv.fit_depth() == 16 and rv.fit_bn_affine() and rv.fit_count() > 1000
        for k, m in enumerate(species_models["ecoli"]):
            stem = train_cli.stem(mdir, "ecoli", k + 1)
            back = load_model(stem + ".f32")
            theta, t = rv.fit_params(k)
            assert theta.size == ba.n_params("signal", 11, m.n_class) and t > 0
            assert back.flat().tobytes() == ba.fitted_model("signal", m, theta, 11).flat().tobytes() and np.isfinite(back.flat()).all()
            assert all(not np.array_equal(back.tensors[i], m.tensors[i]) for i in inside)
            assert all(back.tensors[i].tobytes() == m.tensors[i].tobytes() for i in (4, 5, 10, 11, 42, 43) + tuple(range(12, 32)))
            s = json.load(open(stem + "_summary.json"))
            assert s["options"]["fit_depth"] == "signal" and s["options"]["fit_bn_affine"] is True
            assert list(s["bn_affine"]) == ["bn_c1", "bn_c2", "bn_l3"]
            assert all(v["max_dgamma"] > 0 and v["max_dbeta"] > 0 for v in s["bn_affine"].values())
    finally:
        Reviser.close(rv)
    for mode in ("f32", "f16x2", "bf16x3"):
        o = str(tmp_path / f"B_{mode}") + "/"
        monkeypatch.setenv("NRV_PRECISION", mode)
        assert cli.main(common + ["-o", o, "--model_dir", mdir]) == 0
        assert all(os.path.getsize(o + f"s{i:02d}_out.fasta") > 100 for i in range(2))
