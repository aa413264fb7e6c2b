"""Re-estimating the BatchNorm statistics on the device (MI355X only, -m gpu): csrc/nrv_bnfit.h through nrv_fit_bn_reestimate /
_count / _get.  nanoreviser_amd/bnfit.py is the definition; tests/bnfit_cases.py holds the cases, the restatements and the floors.
  1. exact bytes, conv stage 1: a case whose sums are exact in f64 in any order - S1, S2, mean and var are the definition's BYTES
     for 1, 33 and 160 rows and for two scratch chunks (4096 + 34 rows);
  2. every stage against the definition at float64: depths lstm3, signal and full, both models, both gate functions, within
     cpu_bound() AND K_RECORDED of the f32 floor;
  3. two calls give the same bytes, and so does a fresh handle;
  4. the fit uses them: nrv_fit_grad and nrv_fit_eval agree with the depth's definition at the NEW (s, h) within the depth's own
     device_grades bound, and no longer with the definition at the old ones; a new nrv_fit_begin is back at the handle's own;
  5. round trip: the model written by with_stats in a new handle gives nrv_fit_eval's bytes, its f32 nrv_predict* agrees under the
     tie rule, its f16x2 mode is within 1e-4 of its f32 mode;
  6. refusals by name with the handle left usable; one row at T = 1; a dead channel;
  7. NRV_POISON changes nothing.

Worst device grade seen on an MI355X: see DESIGN section 14."""
import numpy as np
import pytest

import bnfit_cases as bc
import fullfit_cases as fc
import lstm3fit_cases as l3c
import signalfit_cases as sc_
import tailfit_cases as tc
from nanoreviser_amd import bnfit
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import lstm3fit as l3
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.engine import NrvError
from test_gpu_fullfit import ENV, PATTERNS
from test_gpu_headfit import _pack

pytestmark = pytest.mark.gpu

FIELDS = ("mean", "var", "s1", "s2")
ACT_NAME = {0: "hard_sigmoid", 1: "sigmoid"}


def _reviser(monkeypatch, m1, m2, poison=None, **kw):
    from nanoreviser_amd.engine import Reviser
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if poison is not None:
        monkeypatch.setenv("NRV_POISON", f"{PATTERNS[poison]:08x}")
    rv = Reviser(m1, m2, **kw)
    monkeypatch.delenv("NRV_POISON", raising=False)
    return rv


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


def _load(rv, depth, model, x, sig, y):
    """The case's rows through the depth's unit door (both models read the same rows)."""
    rv.fit_reset()
    rv.fit_set_depth(depth)
    other = np.minimum(y, 4)
    y1, y2 = (y, other) if model == 0 else (other, y)
    if depth == "full":
        rv.fit_set_rows_full(sig, x, y1, y2)
    elif depth == "signal":
        rv.fit_set_rows_signal(x, x, sig, y1, y2)
    else:
        rv.fit_set_rows_lstm3(x, x, y1, y2)
    assert rv.fit_count() == len(y)


def _same(a, b):
    return set(a) == set(b) and all(a[k]["n"] == b[k]["n"] and all(a[k][f].tobytes() == b[k][f].tobytes() for f in FIELDS) for k in a)


@pytest.fixture(scope="module")
def grade_bound():
    K, worst = bc.cpu_bound()
    print(f"bnfit: bound sized on the CPU: K = {K:.3g} (worst restatement grade {worst:.3g}); recorded {bc.K_RECORDED}")
    return K


# ---- 1. exact bytes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", [(11, 1), (11, 33), (11, 160), bc.CHUNK], ids=lambda v: str(v))
def test_exact_sums_give_the_definitions_bytes(species_models, monkeypatch, T, n):
    md, x2, sig, y, th = bc.dyadic_case(T, n)
    rv = _reviser(monkeypatch, md.with_window(T), species_models["ecoli"][1].with_window(T))
    try:
        _load(rv, "signal", 0, x2, sig, y)
        assert rv._lib.nrv_fit_bn_count(rv._h) == 3
        rv.fit_begin(0, th)
        before = rv.fit_bn_stats(0)
        bn = bnfit.bn_of(md)
        assert list(before) == ["bn_c1", "bn_c2", "bn_l3"] and [v["tensor_base"] for v in before.values()] == [2, 8, 40]
        for k, v in before.items():                         # before any re-estimation: the loaded statistics, n = 0
            assert v["n"] == 0 and v["mean"].tobytes() == bn[k][2].tobytes() and v["var"].tobytes() == bn[k][3].tobytes()
            assert not v["s1"].any() and not v["s2"].any()
        got = rv.fit_bn_reestimate(0, np.arange(n))["bn_c1"]
        want = bnfit.reestimate("signal", x2, sig, th, bn, np.arange(n), T, 6, 0, np.float32)["bn_c1"]
        assert got["n"] == want["n"] == n * T * 50
        for f in FIELDS:
            assert got[f].tobytes() == want[f].tobytes(), (f, got[f], want[f])
    finally:
        rv.close()


# ---- 2. every stage against the definition ---------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("case", bc.CASES, ids=bc.IDS)
def test_every_stage_against_the_definition(handles, grade_bound, case):
    depth, T, model, n, act = case
    x, sig, y, th = bc.rows_case(*case)
    rv = handles(T, act)
    _load(rv, depth, model, x, sig, y)
    rv.fit_begin(model, th)
    got = rv.fit_bn_reestimate(model, np.arange(n))
    r = bc.reference(*case)
    assert list(got) == list(bnfit.inside(depth)) and all(got[k]["n"] == r["ref"][k]["n"] for k in got)
    assert all(np.isfinite(got[k][f]).all() for k in got for f in FIELDS) and all((got[k]["var"] >= 0).all() for k in got)
    g = bc.grades(got, r)
    for (k, what), v in g.items():
        WORST[k, what] = max(WORST.get((k, what), 0.0), v)
    print(case, {f"{k}.{w}": round(v, 3) for (k, w), v in g.items()}, "bounds", round(grade_bound, 3), bc.K_RECORDED,
          "worst so far", {f"{k}.{w}": round(v, 3) for (k, w), v in WORST.items()})
    assert max(g.values()) <= grade_bound, g
    assert max(g.values()) <= bc.K_RECORDED, g
    assert rv.fit_params(model)[0].tobytes() == th.tobytes() and rv.fit_params(model)[1] == 0      # parameters and t untouched


# ---- 3. idempotent and deterministic ---------------------------------------------------------------------------------------
def test_two_calls_and_a_fresh_handle_give_the_same_bytes(species_models, handles, monkeypatch):
    case = ("full", 11, 0, 33, 0)
    x, sig, y, th = bc.rows_case(*case)
    rows = np.random.default_rng(5).permutation(33)
    rv = handles(11)
    _load(rv, "full", 0, x, sig, y)
    rv.fit_begin(0, th)
    a = rv.fit_bn_reestimate(0, rows)
    b = rv.fit_bn_reestimate(0, rows)                       # from its own result: nothing a stage reads has changed
    assert _same(a, b) and _same(b, rv.fit_bn_stats(0))
    m1, m2 = species_models["ecoli"]
    fresh = _reviser(monkeypatch, m1, m2)
    try:
        _load(fresh, "full", 0, x, sig, y)
        fresh.fit_begin(0, th)
        assert _same(a, fresh.fit_bn_reestimate(0, rows))
    finally:
        fresh.close()


# ---- 4. the fit uses them --------------------------------------------------------------------------------------------------
def _fit_reference(depth, x, sig, y, th, pairs, T, model, act):
    """The depth's grad_reference with the BatchNorm pairs as an argument -> (the dict device_grades reads, p64, the depth's
    case module)."""
    C = bc.n_class(model)
    opts = tf.default_opts(model)
    sc, sh = pairs["bn_l3"]
    if depth == "full":
        mod, fz = fc, (pairs["bn_l1"] + pairs["bn_l2"], pairs["bn_c1"] + pairs["bn_c2"], sc, sh)
        terms = lambda dt: ff.batch_terms(x, sig, y, th, *fz, T, C, opts, act, dt)                  # noqa: E731
        tt = fc.torch_terms(x, sig, y, th, *fz, T, C, opts, act, np.float32)
        p64 = ff.forward(x, sig, th, *fz, T, C, act, np.float64)[7]
    elif depth == "signal":
        mod, fz = sc_, (pairs["bn_c1"] + pairs["bn_c2"], sc, sh)
        terms = lambda dt: sf.batch_terms(x, sig, y, th, *fz, T, C, opts, act, dt)                  # noqa: E731
        tt = sc_.torch_terms(x, sig, y, th, *fz, T, C, opts, act, np.float32)
        p64 = sf.forward(x, sig, th, *fz, T, C, act, np.float64)[6]
    else:
        mod = l3c
        terms = lambda dt: l3.batch_terms(x, y, th, sc, sh, T, C, opts, act, dt)                    # noqa: E731
        tt = l3c.torch_terms(x, y, th, sc, sh, T, C, opts, act, np.float32)
        p64 = l3.forward(x, th, sc, sh, T, C, act, np.float64)[5]
    g64, st64 = terms(np.float64)
    g32, st32 = terms(np.float32)
    sp = mod.spans(T, C)
    ref = {"g64": g64, "st64": st64, "dev_np": mod.deviations(g32, g64, T, C), "dev_torch": mod.deviations(tt[0], g64, T, C),
           "scale": {k: float(np.abs(g64[s]).max()) for k, s in sp.items()},
           "sums64": (st64.ce_sum, st64.center_sum), "sums_np": (st32.ce_sum, st32.center_sum), "sums_torch": (tt[1], tt[2])}
    return ref, p64, mod


def _ref_bound(ref, mod):
    """The depth's cpu_bound over this one reference: twice the worst grade either restatement gets against the other's floor."""
    worst = 1.0
    for k in mod.TENSORS:
        for a, b in ((ref["dev_np"][k], ref["dev_torch"][k]), (ref["dev_torch"][k], ref["dev_np"][k])):
            g = tc.grade_of(a, b, ref["scale"][k])
            if np.isfinite(g):
                worst = max(worst, g)
    for i in range(2):
        a, b = abs(ref["sums_np"][i] - ref["sums64"][i]), abs(ref["sums_torch"][i] - ref["sums64"][i])
        worst = max(worst, tc.grade_of(a, b, abs(ref["sums64"][i])), tc.grade_of(b, a, abs(ref["sums64"][i])))
    return 2.0 * worst


@pytest.mark.parametrize("depth", bc.DEPTHS)
def test_the_fit_runs_on_the_new_statistics(handles, depth):
    T, model, n, act = 11, 1, 33, 0
    x, sig, y, th = bc.rows_case(depth, T, model, n, act)
    m, bn = bc.loaded(model)
    C = bc.n_class(model)
    rv = handles(T, act)
    _load(rv, depth, model, x, sig, y)
    rows = np.arange(n)
    rv.fit_begin(model, th)
    g_old, st_old = rv.fit_grad(model, rows)
    p_old, _ = rv.fit_eval(model, rows)
    # before any re-estimation the block holds the handle's own pairs: the loaded statistics fold to them
    old_pairs = {k: bnfit.fold(*bn[k]) for k in bnfit.inside(depth)}
    assert _same_pairs(bnfit.folded(bn, rv.fit_bn_stats(model)), old_pairs)
    stats = rv.fit_bn_reestimate(model, rows)
    d = bnfit.drift(bn, stats)
    assert all(v["max_dmean_sigma"] > 0.1 for v in d.values()), d                                 # the statistics moved
    g_new, st_new = rv.fit_grad(model, rows)
    p_new, se = rv.fit_eval(model, rows)
    new_ref, p64_new, mod = _fit_reference(depth, x, sig, y, th, bnfit.folded(bn, stats), T, model, act)
    old_ref, p64_old, _ = _fit_reference(depth, x, sig, y, th, old_pairs, T, model, act)
    recorded = getattr(mod, "K_RECORDED", float("inf"))        # (the full depth's case file has one)
    K = min(_ref_bound(new_ref, mod), recorded)
    gr_new = mod.device_grades(g_new, st_new.ce_sum, st_new.center_sum, new_ref, T, C)
    gr_old = mod.device_grades(g_old, st_old.ce_sum, st_old.center_sum, old_ref, T, C)
    cross = mod.device_grades(g_new, st_new.ce_sum, st_new.center_sum, old_ref, T, C)
    print(depth, "new statistics: worst grade", round(max(gr_new.values()), 3), "bound", round(K, 3), "| before, against the old:",
          round(max(gr_old.values()), 3), "| new against the OLD statistics' definition:", f"{max(cross.values()):.3g}")
    assert max(gr_new.values()) <= K, gr_new
    assert max(gr_old.values()) <= min(_ref_bound(old_ref, mod), recorded), gr_old
    assert max(cross.values()) > max(_ref_bound(new_ref, mod), _ref_bound(old_ref, mod), fc.K_RECORDED), cross                                    # no longer the old statistics' result
    assert np.abs(p_new - p64_new).max() <= 64 * tc.EPS32 and np.abs(p_old - p64_old).max() <= 64 * tc.EPS32
    assert np.abs(p_new - p64_old).max() > 64 * tc.EPS32
    assert (se.rows, se.correct, se.ce_sum, se.center_sum) == (n, st_new.correct, st_new.ce_sum, st_new.center_sum)
    assert (st_new.rows, st_new.correct) == (n, new_ref["st64"].correct)
    # a new nrv_fit_begin copies the handle's pairs again: the bytes from before the re-estimation
    rv.fit_begin(model, th)
    assert all(v["n"] == 0 for v in rv.fit_bn_stats(model).values())
    g_back, st_back = rv.fit_grad(model, rows)
    assert g_back.tobytes() == g_old.tobytes() and st_back == st_old and rv.fit_eval(model, rows)[0].tobytes() == p_old.tobytes()


def _same_pairs(a, b):
    return set(a) == set(b) and all(a[k][i].tobytes() == b[k][i].tobytes() for k in a for i in range(2))


# ---- 5. round trip ---------------------------------------------------------------------------------------------------------
def test_the_written_model_gives_the_fits_bytes_in_a_new_handle(species_models, handles, monkeypatch, tmp_path):
    from nanoreviser_amd.weights import load_model
    T, model, n, act = 11, 0, 160, 0
    feat, sig, y, th = bc.rows_case("full", T, model, n, act)
    m1, m2 = species_models["ecoli"]
    rv = handles(T, act)
    _load(rv, "full", model, feat, sig, y)
    rows = np.arange(n)
    rv.fit_begin(model, th)
    stats = rv.fit_bn_reestimate(model, rows)
    p_fit, st_fit = rv.fit_eval(model, rows)
    tf.write_f32(bnfit.with_stats(ff.fitted_model(m1, th, T), stats), str(tmp_path / "m"))
    back = load_model(str(tmp_path / "m.f32"))
    preds = {}
    for mode in ("f32", "f16x2"):
        rv2 = _reviser(monkeypatch, back, m2, precision=mode)
        try:
            if mode == "f32":
                _load(rv2, "full", model, feat, sig, y)
                rv2.fit_begin(model)                        # the handle's own tensors: the fit's, with zero centres (no file holds them)
                assert rv2.fit_params(model)[0][:-96].tobytes() == th[:-96].tobytes()
                rv2.fit_begin(model, th)                    # the same parameters; the new statistics were folded by nrv_create
                assert all(v["n"] == 0 and v["mean"].tobytes() == stats[k]["mean"].tobytes() and v["var"].tobytes() == stats[k]["var"].tobytes()
                           for k, v in rv2.fit_bn_stats(model).items())
                p2, st2 = rv2.fit_eval(model, rows)
                assert p2.tobytes() == p_fit.tobytes() and st2 == st_fit
            preds[mode] = rv2.predict_pair(sig, feat)[0]
        finally:
            rv2.close()
    d = np.abs(p_fit - preds["f32"]).max(-1)
    print(f"written model: nrv_predict (f32) against nrv_fit_eval, max |dp| = {float(d.max()):.3g}; f16x2 against f32, max |dp| = "
          f"{float(np.abs(preds['f16x2'] - preds['f32']).max()):.3g}")
    assert d.max() <= 1e-4
    srt = np.sort(p_fit.astype(np.float64), -1)
    margin = srt[:, -1] - srt[:, -2]
    for i in np.nonzero(p_fit.argmax(-1) != preds["f32"].argmax(-1))[0]:
        assert margin[i] <= 2 * max(d[i], 1e-6), (int(i), float(margin[i]), float(d[i]))
    assert np.isfinite(preds["f16x2"]).all() and np.abs(preds["f16x2"] - preds["f32"]).max() <= 1e-4


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def short_read(reads):
    out = []
    for k in reads.keys:
        _, rd, _ = reads(k)
        out.append(hs.read_tensors_raw(rd))
    return sorted(out, key=lambda r: len(r.starts))[:1]


def test_refusals_by_name_and_the_handle_stays_usable(species_models, short_read, monkeypatch):
    rv = _reviser(monkeypatch, *species_models["ecoli"], precision="f32")
    lib, h = rv._lib, rv._h
    try:
        def refused(rc, name, word):
            err = lib.nrv_last_error(h).decode()
            assert rc == -1 and err.startswith(name + ": ") and word in err, (name, rc, err)

        one = np.zeros(1, np.uint32)
        ptr = one.ctypes.data_as(rv_u32p())
        for depth in ("tail", "head", "lstm4"):
            rv.fit_set_depth(depth)
            assert lib.nrv_fit_bn_count(h) == 0
            refused(lib.nrv_fit_bn_reestimate(h, 0, ptr, 1), "nrv_fit_bn_reestimate", "no BatchNorm lies inside the fitted section")
            refused(lib.nrv_fit_bn_get(h, 0, 0, None, None, None, None, None), "nrv_fit_bn_get", "no BatchNorm lies inside the fitted section")
        x, sig, y, th = bc.rows_case("signal", 11, 0, 33, 0)
        _load(rv, "signal", 0, x, sig, y)
        assert lib.nrv_fit_bn_count(h) == 3
        refused(lib.nrv_fit_bn_reestimate(h, 0, ptr, 1), "nrv_fit_bn_reestimate", "nrv_fit_begin")
        refused(lib.nrv_fit_bn_get(h, 0, 0, None, None, None, None, None), "nrv_fit_bn_get", "nrv_fit_begin")
        rv.fit_begin(0, th)
        refused(lib.nrv_fit_bn_reestimate(h, 1, ptr, 1), "nrv_fit_bn_reestimate", "nrv_fit_begin")          # the other model has none
        refused(lib.nrv_fit_bn_reestimate(h, 2, ptr, 1), "nrv_fit_bn_reestimate", "model must be 0 or 1")
        for bad in (0, -1):
            refused(lib.nrv_fit_bn_reestimate(h, 0, ptr, bad), "nrv_fit_bn_reestimate", "n_rows")
        refused(lib.nrv_fit_bn_reestimate(h, 0, None, 3), "nrv_fit_bn_reestimate", "null row indices")
        with pytest.raises(NrvError, match="nrv_fit_bn_reestimate: a row index outside the training set"):
            rv.fit_bn_reestimate(0, [0, 33])
        for bad in (-1, 3):
            refused(lib.nrv_fit_bn_get(h, 0, bad, None, None, None, None, None), "nrv_fit_bn_get", "which outside")
        want = rv.fit_bn_reestimate(0, np.arange(33))
        g, st = rv.fit_grad(0, np.arange(33))
        t = rv.begin_packed_raw(_pack(rv, short_read))      # between a _begin and its _end
        refused(lib.nrv_fit_bn_reestimate(h, 0, ptr, 1), "nrv_fit_bn_reestimate", "in flight")
        refused(lib.nrv_fit_bn_get(h, 0, 0, None, None, None, None, None), "nrv_fit_bn_get", "in flight")
        rv.end_packed_raw(t)
        assert _same(rv.fit_bn_stats(0), want)              # every refusal left the handle usable and the statistics alone
        g2, st2 = rv.fit_grad(0, np.arange(33))
        assert g2.tobytes() == g.tobytes() and st2 == st
        assert _same(rv.fit_bn_reestimate(0, np.arange(33)), want)
    finally:
        rv.close()


def rv_u32p():
    import ctypes
    return ctypes.POINTER(ctypes.c_uint32)


def test_one_row_at_T_1_and_a_dead_channel(species_models, monkeypatch):
    # a set of one row at T = 1, lstm3 depth: N = 1, the mean is the row's own output and the variance exactly 0
    m1, m2 = species_models["ecoli"]
    X, y, th = l3c.rows_case(1, 0, 1, "plain", 0)
    rv = _reviser(monkeypatch, m1.with_window(1), m2.with_window(1))
    try:
        _load(rv, "lstm3", 0, X, None, y)
        rv.fit_begin(0, th)
        got = rv.fit_bn_reestimate(0, [0])["bn_l3"]
        want = bnfit.reestimate("lstm3", X, None, th, bc.loaded(0)[1], [0], 1, 6, 0, np.float64)["bn_l3"]
        assert got["n"] == 1 and got["var"].tobytes() == bytes(4 * 256) and np.abs(got["mean"] - want["mean"]).max() <= 4 * tc.EPS32
        assert np.isfinite(rv.fit_eval(0, [0])[0]).all()
    finally:
        rv.close()
    # b1 = -100 on channel 3 of the exact case: a1 is 0 there, the variance exactly 0, the folded scale finite
    md, x2, sig, y, th = bc.dyadic_case(11, 33)
    th = th.copy()
    th[sc_.spans(11, 6)["cb1"]][3] = -100.0
    rv = _reviser(monkeypatch, md, m2)
    try:
        _load(rv, "signal", 0, x2, sig, y)
        rv.fit_begin(0, th)
        got = rv.fit_bn_reestimate(0, np.arange(33))
        c1 = got["bn_c1"]
        assert c1["var"][3] == 0.0 and c1["mean"][3] == 0.0 and (np.delete(c1["var"], 3) > 0).all()
        s, hh = bnfit.folded(bnfit.bn_of(md), got)["bn_c1"]
        assert np.isfinite(s).all() and np.isfinite(hh).all()
        want = bnfit.reestimate("signal", x2, sig, th, bnfit.bn_of(md), np.arange(33), 11, 6, 0, np.float32)["bn_c1"]
        assert all(c1[f].tobytes() == want[f].tobytes() for f in FIELDS)
        g, st = rv.fit_grad(0, np.arange(33))
        assert np.isfinite(g).all() and st.nonfinite == 0
    finally:
        rv.close()


# ---- 7. NRV_POISON ---------------------------------------------------------------------------------------------------------
def test_poison_changes_nothing(species_models, handles, monkeypatch):
    cases = [("full", 11, 0, 33, 0), ("signal", bc.CHUNK[0], 0, bc.CHUNK[1], 1)]
    for case in cases:
        depth, T, model, n, act = case
        x, sig, y, th = bc.rows_case(*case)
        rv = handles(T, act)
        _load(rv, depth, model, x, sig, y)
        rv.fit_begin(model, th)
        want = rv.fit_bn_reestimate(model, np.arange(n))
        p_want = rv.fit_eval(model, np.arange(min(n, 64)))[0]
        m1, m2 = species_models["ecoli"]
        for poison in sorted(PATTERNS):
            pv = _reviser(monkeypatch, m1.with_window(T), m2.with_window(T), poison=poison, recurrent_activation=ACT_NAME[act])
            try:
                _load(pv, depth, model, x, sig, y)
                pv.fit_begin(model, th)
                assert _same(pv.fit_bn_reestimate(model, np.arange(n)), want), (case, poison)
                assert pv.fit_eval(model, np.arange(min(n, 64)))[0].tobytes() == p_want.tobytes(), (case, poison)
            finally:
                pv.close()
