"""The dropout behind the identity block on the device (MI355X only, -m gpu): csrc/nrv_dropout.h and the DROP instantiations of
csrc/nrv_signalfit.h through nrv_fit_set_dropout and the nrv_fit_* entry points.  nanoreviser_amd/dropout.py is the definition;
tests/dropout_cases.py holds the cases, the torch restatement and the floors.  Every set goes in through the unit doors.
  1. nrv_fit_dropout_mask is dropout.keep_mask bit for bit: non-contiguous and repeated rows, a draw above 2^32, a seed with a
     non-zero high word, T 1 / 3 / 11 with 1 / 33 / 64 rows, 4130 rows at T 2, both models;
  2. nrv_fit_grad at rate 0.2 and a non-zero draw, on the set's rows in DESCENDING order, per tensor (gWs among them: F was kept
     dropped) and the two sums within cpu_bound() AND K_RECORDED of the float64 definition under keep_mask's mask, at signal and
     full depth; the 4130-row batch is the depths' own chunk case, sigmoid gates included (dropout_cases.act_of says why), and its
     second scratch chunk proves the mask follows the set row; the draw stays where it was;
  3. with nrv_fit_set_bn_affine as well: every gamma / beta sum (bn_c2's sees the masked dF) within cpu_bound_affine() AND
     K_RECORDED_AFFINE, and the rest of the vector's gradient is the bytes of the call without the block;
  4. at rate 1e-12 (thr 0, keepf 1) nrv_fit_grad, an nrv_fit_epoch of three batches and the parameters behind it are the
     switch-off bytes, at both depths, bn-affine off and on: the variants are the parent's arithmetic;
  5. nrv_fit_eval and nrv_fit_bn_reestimate give the switch-off bytes while the switch is on;
  6. the counter: epoch(order) = epoch(order[:B]) then epoch(order[B:]) in parameters and draw; the same calls twice, and under
     NRV_POISON, give the same bytes; a second epoch at the moved draw differs from a second epoch at the first one's draw;
     a skipped non-finite batch advances the draw but not t; nrv_fit_begin resets it;
  7. refusals by whole string, the handle staying usable; nrv_fit_set_depth switches it off; nrv_fit_begin is not forgotten.
     (T > 655 cannot be reached: nrv_create takes T <= 32.)

Seen on an MI355X (DESIGN section 16 has every case): worst gradient grade 6.22 floors (full depth, T 11, one row, lstm2's b2b)
against K_RECORDED 35.57, signal depth at most 2.62, gWs at most 2.39, the 4130-row case 2.52 / 3.66; worst gamma / beta sum
1.94 against K_RECORDED_AFFINE 26.09."""
import numpy as np
import pytest

import bnaffine_cases as bac
import bnfit_cases as bc
import dropout_cases as dc
from nanoreviser_amd import bnaffine as ba
from nanoreviser_amd import dropout as dr
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import tailfit as tf
from test_gpu_bnfit import ACT_NAME, _load, _reviser, _same
from test_gpu_fullfit import PATTERNS
from test_gpu_headfit import _pack

pytestmark = pytest.mark.gpu

WHO = "nrv_fit_set_dropout: "
REFUSED_RATE = WHO + "rate must lie in [0, 1)"
REFUSED_DEPTH = WHO + "the signal branch is frozen at this depth, there is nothing to drop (depths NRV_FIT_SIGNAL and NRV_FIT_FULL fit it)"
REFUSED_IN_FLIGHT = WHO + "a raw-read call is in flight (collect it with nrv_reads_raw_end first)"
REFUSED_OFF = "nrv_fit_dropout_mask: the dropout is off (call nrv_fit_set_dropout with a rate above 0 first)"


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
def grade_bound():
    K, worst = dc.cpu_bound()
    print(f"dropout: bound sized on the CPU: K = {K:.3g} (worst restatement grade {worst:.3g}); recorded {dc.K_RECORDED}")
    return K


@pytest.fixture(scope="module")
def affine_bound():
    K, worst = dc.cpu_bound_affine()
    print(f"dropout + bn-affine: bound sized on the CPU: K = {K:.3g} (worst restatement grade {worst:.3g}); recorded {dc.K_RECORDED_AFFINE}")
    return K


def _set(rv, depth, model, x, sig, y, rate=dc.RATE, affine=False):
    """The rows through the depth's unit door (nrv_fit_set_depth has switched everything off), then the switches."""
    _load(rv, depth, model, x, sig, y)
    assert rv.fit_dropout() == (0.0, rv.fit_dropout()[1], (0, 0)) and not rv.fit_bn_affine()
    if affine:
        rv.fit_set_bn_affine(True)
    if rate:
        rv.fit_set_dropout(rate, dc.SEED)
        assert rv.fit_dropout() == (rate, dc.SEED, (0, 0))


# ---- 1. the mask's bytes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", [(1, 1), (1, 64), (3, 33), (11, 1), (11, 33), (11, 64), (2, 4130)])
def test_mask_bytes_are_the_definitions(handles, T, n):
    rv = handles(T)
    rng = np.random.default_rng(T * 100 + n)
    rows = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    rows[::3] = rows[0]                                     # repeated
    rows[1::7] = rng.integers(0, 50, rows[1::7].size)       # small next to huge
    rv.fit_reset()
    for depth, model in (("signal", 0), ("full", 1)):
        rv.fit_set_depth(depth)
        rv.fit_set_dropout(dc.RATE, dc.SEED)
        for draw in (dc.DRAW, 0):
            got = rv.fit_dropout_mask(model, rows, draw)
            want = dr.keep_mask(dc.SEED, draw, model, rows, T, dc.RATE)
            assert got.shape == want.shape == (n, T, 400) and got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8].tolist()
        assert rv.fit_dropout()[2] == (0, 0)                # the door's draw is an argument: the counters stay
    rv.fit_set_dropout(0.5, 1)                              # another rate and seed
    assert rv.fit_dropout_mask(0, rows[:5], 9).tobytes() == dr.keep_mask(1, 9, 0, rows[:5], T, 0.5).tobytes()


# ---- 2. the gradient -------------------------------------------------------------------------------------------------------
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("dropout: worst device grade per tensor over the cases run:", {k: round(v, 2) for k, v in sorted(WORST.items(), key=lambda kv: -kv[1])})


@pytest.mark.parametrize("case", dc.CASES + dc.CHUNK_CASES, ids=dc.IDS)
def test_gradient_against_the_definition_under_the_mask(handles, grade_bound, case):
    depth, T, model, n = case
    act = dc.act_of(n)                                      # sigmoid gates for the 4130-row batch, as in the depths' own chunk case
    x, sig, y, th = bc.rows_case(depth, T, model, n, act)
    rv = handles(T, act)
    _set(rv, depth, model, x, sig, y)
    rv.fit_begin(model, th)
    rv.fit_set_dropout_draw(model, dc.DRAW)
    g, st = rv.fit_grad(model, dc.order_of(n))
    assert rv.fit_dropout()[2][model] == dc.DRAW            # nrv_fit_grad leaves the draw
    r = dc.graded(case)
    assert g.size == th.size and np.isfinite(g).all() and (st.rows, st.nonfinite, st.correct) == (n, 0, r["st64"].correct)
    gr = dc.grades(g, st.ce_sum, st.center_sum, r)
    assert "Ws" in gr and "cw2" in gr and "ce_sum" in gr
    for k, v in gr.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(case, "worst", max(gr, key=gr.get), round(max(gr.values()), 3), "Ws", round(gr["Ws"], 3), "cw2", round(gr["cw2"], 3), "bounds",
          round(grade_bound, 3), dc.K_RECORDED, "worst so far", round(max(WORST.values()), 3))
    assert max(gr.values()) <= grade_bound, gr
    assert max(gr.values()) <= dc.K_RECORDED, gr
    g2, st2 = rv.fit_grad(model, dc.order_of(n))            # the same call, the same bytes
    assert g2.tobytes() == g.tobytes() and st2 == st
    rv.fit_set_dropout_draw(model, dc.DRAW + 1)             # another draw, another gradient
    assert rv.fit_grad(model, dc.order_of(n))[0].tobytes() != g.tobytes()


# ---- 3. with the gamma / beta block ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.AFFINE_CASES, ids=dc.IDS)
def test_gamma_beta_sums_see_the_masked_df(handles, affine_bound, case):
    depth, T, model, n = case
    x, sig, y, vec, stats = bac.rows_case(depth, T, model, n, dc.ACT, "plain")
    rv = handles(T)
    _set(rv, depth, model, x, sig, y, affine=True)
    rv.fit_begin(model, vec)
    rv.fit_set_dropout_draw(model, dc.DRAW)
    g, st = rv.fit_grad(model, dc.order_of(n))
    r = dc.graded(case, affine=True)
    gr = dc.grades(g, None, None, r)
    assert set(gr) == set(bac.names(depth)) and "bn_c2.gamma" in gr and st.correct == r["st64"].correct
    print(case, {k: round(v, 3) for k, v in gr.items()}, "bounds", round(affine_bound, 3), dc.K_RECORDED_AFFINE)
    assert max(gr.values()) <= affine_bound, gr
    assert max(gr.values()) <= dc.K_RECORDED_AFFINE, gr
    # the block changes no other launch's sums: behind it, the bytes of the call without it at the same draw
    nb = ba.n_block(depth)
    rv.fit_set_bn_affine(False)
    assert rv.fit_dropout()[0] == dc.RATE                   # (the switch survives the other one)
    rv.fit_begin(model, vec[nb:])
    rv.fit_set_dropout_draw(model, dc.DRAW)
    g_off, st_off = rv.fit_grad(model, dc.order_of(n))
    assert g[nb:].tobytes() == g_off.tobytes() and st == st_off


# ---- 4. the variants are the parent's arithmetic ---------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "bn_affine"])
@pytest.mark.parametrize("depth", dc.DEPTHS)
def test_rate_that_keeps_everything_gives_the_switch_off_bytes(handles, depth, affine):
    T, model, n = 11, 1, 33
    x, sig, y, vec, stats = bac.rows_case(depth, T, model, n, dc.ACT, "plain")
    vec = vec if affine else vec[ba.n_block(depth):]
    rv = handles(T)
    opts = tf.default_opts(model, B=16)
    order = np.random.default_rng(3).permutation(n)
    out = []
    for rate in (0.0, 1e-12):
        _set(rv, depth, model, x, sig, y, rate=rate, affine=affine)
        rv.fit_begin(model, vec, opts)
        if rate:
            rv.fit_set_dropout_draw(model, 5)
        g, sg = rv.fit_grad(model, order)
        se = rv.fit_epoch(model, order)
        p, t = rv.fit_params(model)
        assert t == 3 and rv.fit_dropout()[2][model] == (8 if rate else 0)
        out.append((g.tobytes(), sg, se, p.tobytes()))
    assert out[0] == out[1]
    assert out[0][3] != vec.tobytes()


# ---- 5. evaluation does not drop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", dc.DEPTHS)
def test_eval_and_reestimation_do_not_drop(handles, depth):
    T, model, n = 11, 0, 33
    x, sig, y, th = bc.rows_case(depth, T, model, n, dc.ACT)
    rv = handles(T)
    rows = np.arange(n)
    out = []
    for rate in (0.0, dc.RATE):
        _set(rv, depth, model, x, sig, y, rate=rate)
        rv.fit_begin(model, th)
        if rate:
            rv.fit_set_dropout_draw(model, dc.DRAW)
        p, e = rv.fit_eval(model, rows)
        stats = rv.fit_bn_reestimate(model, rows)
        p2, e2 = rv.fit_eval(model, rows)
        out.append((p.tobytes(), e, stats, p2.tobytes(), e2, rv.fit_grad(model, rows)[0].tobytes()))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and _same(out[0][2], out[1][2])
    assert out[0][3] == out[1][3] and out[0][4] == out[1][4]
    assert out[0][5] != out[1][5]                           # while the gradient does drop


# ---- 6. the counter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", dc.DEPTHS)
def test_the_draw_counter(species_models, handles, monkeypatch, depth):
    T, model, n, B = 3, 1, 33, 8
    x, sig, y, th = bc.rows_case(depth, T, model, n, dc.ACT)
    opts = tf.default_opts(model, B=B)
    order = np.random.default_rng(11).permutation(n)       # five batches, the last of one row

    def run(rv, calls):
        """begin at draw 3, then per call (rows, draw to set first | None) -> (parameters, t, draw)."""
        _set(rv, depth, model, x, sig, y)
        rv.fit_begin(model, th, opts)
        assert rv.fit_dropout()[2] == (0, 0)
        rv.fit_set_dropout_draw(model, 3)
        for rows, draw in calls:
            if draw is not None:
                rv.fit_set_dropout_draw(model, draw)
            st = rv.fit_epoch(model, rows)
            assert st.nonfinite == 0 and st.rows == len(rows)
        p, t = rv.fit_params(model)
        return p.tobytes(), t, rv.fit_dropout()[2]

    rv = handles(T)
    whole = run(rv, [(order, None)])
    assert whole[1:] == (5, (0, 8) if model else (8, 0))
    assert run(rv, [(order[:B], None), (order[B:], None)]) == whole                  # batch k of a call drops at draw + k
    assert run(rv, [(order, None)]) == whole                                         # the same calls, the same bytes
    for poison in sorted(PATTERNS):
        m1, m2 = species_models["ecoli"]
        rp = _reviser(monkeypatch, m1.with_window(T), m2.with_window(T), poison=poison)
        try:
            assert run(rp, [(order, None)]) == whole
        finally:
            rp.close()
    moved = run(rv, [(order, None), (order, None)])                                  # the second epoch at draw 8
    again = run(rv, [(order, None), (order, 3)])                                     # the second epoch at draw 3 once more
    assert moved[1] == again[1] == 10 and moved[0] != again[0] and moved[2][model] == 13 and again[2][model] == 8
    rv.fit_begin(model, th, opts)                                                    # nrv_fit_begin resets the model's draw
    assert rv.fit_dropout()[2] == (0, 0)


@pytest.mark.parametrize("depth", dc.DEPTHS)
def test_a_skipped_batch_advances_the_draw_but_not_t(handles, depth):
    T, model, n = 11, 0, 33
    x, sig, y, th = bc.rows_case(depth, T, model, n, dc.ACT)
    sig = np.array(sig)
    sig[20, 3, 2] = np.inf
    rv = handles(T)
    _set(rv, depth, model, x, sig, y)
    opts = tf.default_opts(model, B=16)
    rv.fit_begin(model, th, opts)
    st = rv.fit_epoch(model, np.arange(16, 32))             # the batch with the row alone
    got, t = rv.fit_params(model)
    assert (t, st.steps, st.nonfinite, st.rows) == (0, 0, 1, 0) and got.tobytes() == th.tobytes()
    assert rv.fit_dropout()[2][model] == 1
    st = rv.fit_epoch(model, np.arange(n))                  # batches of 16, 16 (skipped), 1 at draws 1, 2, 3
    got, t = rv.fit_params(model)
    assert (t, st.steps, st.nonfinite, st.rows) == (2, 2, 1, 17) and np.isfinite(got).all() and rv.fit_dropout()[2][model] == 4
    rv.fit_begin(model, th, opts)                           # the two updates alone, at their draws
    rv.fit_set_dropout_draw(model, 1)
    rv.fit_epoch(model, np.arange(16))
    rv.fit_set_dropout_draw(model, 3)
    rv.fit_epoch(model, np.array([32]))
    assert rv.fit_params(model)[0].tobytes() == got.tobytes()


# ---- 7. doors --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def short_reads(reads):
    out = []
    for k in reads.keys:
        _, rd, _ = reads(k)
        out.append(hs.read_tensors_raw(rd))
    return sorted(out, key=lambda r: len(r.starts))[:1]


def test_doors_refusals_and_what_is_kept(species_models, short_reads, monkeypatch):
    import ctypes as C
    rv = _reviser(monkeypatch, *species_models["ecoli"], precision="f32")
    lib, h = rv._lib, rv._h
    err = lambda: lib.nrv_last_error(h).decode()      # noqa: E731
    try:
        assert rv.fit_dropout() == (0.0, 0, (0, 0))
        assert lib.nrv_fit_dropout(h, None, None, None) == 0                          # any output may be NULL
        for depth in ("tail", "head", "lstm4", "lstm3"):
            rv.fit_set_depth(depth)
            assert lib.nrv_fit_set_dropout(h, 0.2, 1) == -1 and err() == REFUSED_DEPTH
            assert lib.nrv_fit_set_dropout(h, 0.0, 1) == 0 and rv.fit_dropout()[0] == 0.0               # off is what it is
            assert lib.nrv_fit_dropout_mask(h, 0, None, 1, 0, None) == -1 and err() == REFUSED_OFF
        x, sig, y, th = bc.rows_case("signal", 11, 0, 33, 0)
        _load(rv, "signal", 0, x, sig, y)
        for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
            assert lib.nrv_fit_set_dropout(h, bad, 1) == -1 and err() == REFUSED_RATE
        rows = np.arange(33, dtype=np.uint32)
        assert lib.nrv_fit_dropout_mask(h, 0, rows.ctypes.data_as(C.POINTER(C.c_uint32)), 33, 0, None) == -1 and err() == REFUSED_OFF
        rv.fit_begin(0, th)
        g_off, _ = rv.fit_grad(0, rows)
        rv.fit_set_dropout(0.2, dc.SEED)                   # does not forget nrv_fit_begin; the vector keeps its length
        assert rv.fit_params(0)[0].tobytes() == th.tobytes() and rv.fit_count() == 33
        g, st = rv.fit_grad(0, rows)
        assert g.tobytes() != g_off.tobytes()
        assert lib.nrv_fit_set_dropout_draw(h, 0, -1) == -1 and err() == "nrv_fit_set_dropout_draw: draw must not be negative"
        assert lib.nrv_fit_set_dropout_draw(h, 2, 0) == -1 and err() == "nrv_fit_set_dropout_draw: model must be 0 or 1"
        assert lib.nrv_fit_dropout_mask(h, 2, rows.ctypes.data_as(C.POINTER(C.c_uint32)), 33, 0, None) == -1
        assert err() == "nrv_fit_dropout_mask: model must be 0 or 1"
        assert lib.nrv_fit_dropout_mask(h, 0, rows.ctypes.data_as(C.POINTER(C.c_uint32)), 33, 0, None) == -1
        assert err() == "nrv_fit_dropout_mask: null rows / mask"
        rv.fit_set_dropout_draw(1, 6)
        rv.fit_set_dropout(0.2, dc.SEED + 1)               # resets both draws
        assert rv.fit_dropout() == (0.2, dc.SEED + 1, (0, 0))
        rv.fit_set_dropout(0.2, dc.SEED)
        t = rv.begin_packed_raw(_pack(rv, short_reads))    # between a _begin and its _end
        for rate in (0.0, 0.3):
            assert lib.nrv_fit_set_dropout(h, rate, 1) == -1 and err() == REFUSED_IN_FLIGHT
        assert lib.nrv_fit_set_dropout_draw(h, 0, 1) == -1 and "a raw-read call is in flight" in err()
        rv.end_packed_raw(t)
        assert rv.fit_dropout() == (0.2, dc.SEED, (0, 0))  # every refusal left the handle usable and the fit alone
        g2, st2 = rv.fit_grad(0, rows)
        assert g2.tobytes() == g.tobytes() and st2 == st
        rv.fit_set_dropout(0.0, dc.SEED)                   # off again: the parent's bytes
        assert rv.fit_grad(0, rows)[0].tobytes() == g_off.tobytes()
        rv.fit_set_dropout(0.2, dc.SEED)
        rv.fit_reset()
        rv.fit_set_depth("signal")                         # nrv_fit_set_depth, the same depth again included, switches it off
        assert rv.fit_dropout()[0] == 0.0
    finally:
        rv.close()
