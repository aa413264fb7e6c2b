"""Fitting the whole model on the device (MI355X only, -m gpu): csrc/nrv_fullfit.h through the nrv_fit_* entry points at depth
NRV_FIT_FULL.  nanoreviser_amd/fullfit.py is the definition; tests/fullfit_cases.py holds the cases, the two f32 restatements
and the floors.  Every tolerance is sized from CPU restatements against the float64 definition.
  1. doors and refusals: the _full doors round-trip bytes; every door refused by name at the five other depths and in flight;
     depth 32 accepted, 18 .. 31 and 33 refused; NRV_FIT_MAX_FULL_ROWS; a parameter count of another depth;
  2. gradient: every case through the unit doors and nrv_fit_grad, per tensor (41) and sum within cpu_bound() AND K_RECORDED; counts
     exact; T = 1 gives gU1 .. gU4 bytes of zero; `zeros`, `edges` and a batch of two scratch chunks (4130 rows) the same way;
  3. real windows: the set gathered from the short fixture reads is the same bytes from f32 and f16x2 mode; sig is what the same
     handle gathers at signal depth and feat the windows of the call's feat_ev, byte for byte; X2b recomputed by fullfit.forward at
     float64 within the f32 floor of the x2 the signal depth gathered; nrv_fit_eval at the handle's own tensors within the bound
     of the fp64 oracle and equal to the f32 mode's nrv_predict* under the tie rule;
  4. one update = tailfit_cases.adam_f32 on nrv_fit_grad's vector, byte for byte; a three-batch epoch twice and under poison;
  5. a row holding inf in feat: its batch is counted in nonfinite and the parameters keep their bytes;
  6. it learns from the shipped start with lstm1 / lstm2 perturbed, and the written model runs in a new handle in every mode;
  7. the signal depth's nrv_fit_grad gives a fresh handle's bytes after this depth has been used in the process;
  8. the command line: NanoReviser_train.py --fit_depth full -e 1 writes a directory NanoReviser.py --model_dir runs.

Worst device grade seen on an MI355X: see DESIGN section 13."""
import math

import numpy as np
import pytest

import fullfit_cases as fc
import signalfit_cases as sc_
import tailfit_cases as tc
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import headfit as hf
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import lstm3fit as l3
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.engine import FIT_FULL, NrvError
from test_gpu_headfit import _all_rows, _args, _labels_for, _pack
from test_gpu_lstm4fit import _row_bound

pytestmark = pytest.mark.gpu

PATTERNS = {"qnan": 0x7FC00000, "m1500": 0xC4BB8000}
ENV = ("NRV_PRECISION", "NRV_COALESCE", "NRV_LANES", "NRV_POISON", "NRV_FIT_MAX_ROWS", "NRV_FIT_MAX_HEAD_ROWS", "NRV_FIT_MAX_LSTM4_ROWS",
       "NRV_FIT_MAX_LSTM3_ROWS", "NRV_FIT_MAX_SIGNAL_ROWS", "NRV_FIT_MAX_FULL_ROWS")
IDS = lambda c: "T%d-m%d-n%d-%s-act%d" % c      # noqa: E731
CHUNK_CASE = fc.CHUNK_CASE                      # 8260 (row, t) pairs: one scratch chunk of 4096 rows and a second of 34, the last tile short
BN_IDS = [2, 3, 4, 5, 8, 9, 10, 11, 18, 19, 20, 21, 28, 29, 30, 31, 40, 41, 42, 43]
FITTED = list(range(12, 18)) + list(range(22, 28)) + [0, 1, 6, 7, 32, 33] + list(range(34, 40)) + list(range(44, 60))
U_TENSORS = fc.U_TENSORS


def _engine(monkeypatch, m1, m2, poison=None, **kw):
    from nanoreviser_amd.engine import Reviser
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if poison is not None:
        monkeypatch.setenv("NRV_POISON", f"{PATTERNS[poison]:08x}")
    rv = Reviser(m1, m2, **kw)
    monkeypatch.delenv("NRV_POISON", raising=False)
    rv.fit_set_depth("full")
    assert rv.fit_depth() == FIT_FULL == 32
    assert rv.fit_n_params(0) == ff.n_params(rv.T, 6) and rv.fit_n_params(1) == ff.n_params(rv.T, 5)
    return rv


@pytest.fixture(scope="module")
def short_reads(reads):
    out = []
    for k in reads.keys:
        _, rd, _ = reads(k)
        out.append(hs.read_tensors_raw(rd))
    return sorted(out, key=lambda r: len(r.starts))[:2]


@pytest.fixture(scope="module")
def handles(species_models):
    """One full-depth handle per (window length, recurrent_act), made on first use and shared.  Their frozen BatchNorms are the
    shipped ecoli ones, as fullfit_cases.read_bn, .conv_bn and .bn are."""
    from nanoreviser_amd.engine import Reviser
    made = {}

    def get(T, act=0):
        if (T, act) not in made:
            m1, m2 = species_models["ecoli"]
            made[T, act] = Reviser(m1.with_window(T), m2.with_window(T), recurrent_activation="sigmoid" if act else "hard_sigmoid")
            made[T, act].fit_set_depth("full")
        return made[T, act]
    yield get
    for rv in made.values():
        rv.close()


def _frozen(model):
    return (fc.read_bn(model), fc.conv_bn(model)) + tuple(fc.bn(model))


def _set_case(rv, case):
    T, model, n, kind, act = case
    feat, sig, y, th = fc.rows_case(*case)
    other = np.minimum(y, 4)
    rv.fit_set_rows_full(sig, feat, y if model == 0 else other, other if model == 0 else y)
    assert rv.fit_count() == n
    return feat, sig, y, th


@pytest.fixture(scope="module")
def grade_bound():
    K, worst = fc.cpu_bound()
    print(f"full depth: gradient bound sized on the CPU: K = {K:.3g} (worst restatement grade {worst:.3g}); recorded {fc.K_RECORDED}")
    return K


# ---- 1. doors and refusals -------------------------------------------------------------------------------------------------
def test_doors_and_refusals_by_name(species_models, short_reads, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    rv = Reviser(*species_models["ecoli"], precision="f32")
    lib, h = rv._lib, rv._h

    def refused(rc, name, word=""):
        err = lib.nrv_last_error(h).decode()
        assert rc == -1 and err.startswith(name + ": ") and word in err, (name, rc, err)

    rng = np.random.default_rng(3)
    n = 77
    x1, x2 = (rng.normal(0, 1, (n, 11, 128)).astype(np.float32) for _ in range(2))
    sg = rng.normal(0, 1, (n, 11, 50)).astype(np.float32)
    ft = rng.normal(0, 1, (n, 11, 6)).astype(np.float32)
    xin = rng.normal(0, 1, (n, 11, 192)).astype(np.float32)
    xb = rng.normal(0, 1, (n, 11, 256)).astype(np.float32)
    F = rng.uniform(0, 1, (n, 66)).astype(np.float32)
    y1, y2 = rng.integers(0, 6, n).astype(np.uint8), rng.integers(0, 5, n).astype(np.uint8)
    none4, none5 = (None,) * 4, (None,) * 5
    # the five other depths: the _full doors are refused under their own names
    for depth, word in (("tail", "tail depth"), ("head", "head depth"), ("lstm4", "lstm4 depth"), ("lstm3", "lstm3 depth"),
                        ("signal", "signal depth")):
        rv.fit_set_depth(depth)
        with pytest.raises(NrvError, match="nrv_fit_set_rows_full: the set is at " + word):
            rv.fit_set_rows_full(sg, ft, y1, y2)
        refused(lib.nrv_fit_get_rows_full(h, 0, 0, *none4), "nrv_fit_get_rows_full", word)
    rv.fit_set_depth("tail")
    for bad in (2, 3, 5, 6, 7, 9, -1, 10, 15, 17) + tuple(range(18, 32)) + (33, 64):
        refused(lib.nrv_fit_set_depth(h, bad), "nrv_fit_set_depth", "NRV_FIT_TAIL or NRV_FIT_HEAD")
        assert all(w in lib.nrv_last_error(h).decode() for w in ("NRV_FIT_LSTM4", "NRV_FIT_LSTM3", "NRV_FIT_SIGNAL", "NRV_FIT_FULL"))
    # full depth: 32 is accepted on the empty set; the five other depths' doors are refused
    assert lib.nrv_fit_set_depth(h, 32) == 0 and rv.fit_depth() == 32 and rv.fit_count() == 0
    with pytest.raises(NrvError, match="nrv_fit_set_rows: the set is at full depth"):
        rv.fit_set_rows(F, F, y1, y2)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_head: the set is at full depth"):
        rv.fit_set_rows_head(x1, x1, y1, y2)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_lstm4: the set is at full depth"):
        rv.fit_set_rows_lstm4(xb, xb, y1, y2)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_lstm3: the set is at full depth"):
        rv.fit_set_rows_lstm3(xin, xin, y1, y2)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_signal: the set is at full depth"):
        rv.fit_set_rows_signal(x1, x2, sg, y1, y2)
    for name in ("nrv_fit_get_rows", "nrv_fit_get_rows_head", "nrv_fit_get_rows_lstm4", "nrv_fit_get_rows_lstm3"):
        refused(getattr(lib, name)(h, 0, 0, *none4), name, "full depth")
    refused(lib.nrv_fit_get_rows_signal(h, 0, 0, *none5), "nrv_fit_get_rows_signal", "full depth")
    refused(lib.nrv_fit_set_rows_full(h, None, None, None, None, 4), "nrv_fit_set_rows_full", "null rows")
    with pytest.raises(NrvError, match="nrv_fit_set_rows_full: a label outside"):
        rv.fit_set_rows_full(sg, ft, np.full(n, 6, np.uint8), y2)
    refused(lib.nrv_fit_params(h, 0, None, None), "nrv_fit_params", "nrv_fit_begin")          # the depth change forgot any begin
    # the doors round-trip bytes, sub-ranges too
    rv.fit_set_rows_full(sg, ft, y1, y2)
    assert rv.fit_count() == n
    got = rv.fit_get_rows_full()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, (sg, ft, y1, y2)))
    for first, count in ((0, 1), (31, 33), (76, 1), (77, 0)):
        sub = rv.fit_get_rows_full(first, count)
        assert all(a.tobytes() == b[first:first + count].tobytes() for a, b in zip(sub, (sg, ft, y1, y2))), (first, count)
    with pytest.raises(NrvError, match="nrv_fit_get_rows_full: rows outside the training set"):
        rv.fit_get_rows_full(70, 8)
    with pytest.raises(ValueError):
        rv.fit_set_rows_full(xin, ft, y1, y2)
    for d in (0, 1, 4, 8, 16):
        refused(lib.nrv_fit_set_depth(h, d), "nrv_fit_set_depth", "not empty")
    # a parameter count of another depth is refused
    for other in (tf.n_params(11, 6), hf.n_params(11, 6), l4.n_params(11, 6), l3.n_params(11, 6), sf.n_params(11, 6)):
        with pytest.raises(ValueError, match=f"expected {ff.n_params(11, 6)} parameters, got {other}"):
            rv.fit_begin(0, np.zeros(other, np.float32))
    rv.fit_begin(0)
    rows = np.arange(33, dtype=np.uint32)
    want_g, want_st = rv.fit_grad(0, rows)
    assert want_g.size == ff.n_params(11, 6) == 52608 + 25896 + 328704 + 164352 + 20838 + tf.n_params(11, 6)
    # in flight: the depth cannot change and the doors are refused under their own names
    t = rv.begin_packed_raw(_pack(rv, short_reads[:1]))
    refused(lib.nrv_fit_set_depth(h, 0), "nrv_fit_set_depth", "in flight")
    refused(lib.nrv_fit_set_rows_full(h, None, None, None, None, 0), "nrv_fit_set_rows_full", "in flight")
    refused(lib.nrv_fit_get_rows_full(h, 0, 0, *none4), "nrv_fit_get_rows_full", "in flight")
    assert lib.nrv_fit_depth(h) == 32
    rv.end_packed_raw(t)
    g3, st3 = rv.fit_grad(0, rows)
    assert g3.tobytes() == want_g.tobytes() and st3 == want_st and rv.fit_count() == n          # the handle stayed usable
    rv.close()
    # a handle under NRV_FIT_MAX_FULL_ROWS = 1000 refuses an adding call whole, by that name, and stays usable
    monkeypatch.setenv("NRV_FIT_MAX_FULL_ROWS", "1000")
    rv = Reviser(*species_models["ecoli"])
    monkeypatch.delenv("NRV_FIT_MAX_FULL_ROWS")
    rv.fit_set_depth("full")
    labels = _labels_for(short_reads)
    with pytest.raises(NrvError) as e:
        rv.fit_add_packed(_pack(rv, short_reads), labels)
    assert e.value.code == -1 and "nrv_fit_add_reads_raw: the call would pass the row cap" in str(e.value) and "NRV_FIT_MAX_FULL_ROWS" in str(e.value)
    assert rv.fit_count() == 0
    with pytest.raises(NrvError, match="NRV_FIT_MAX_FULL_ROWS"):
        rv.fit_set_rows_full(np.zeros((1001, 11, 50), np.float32), np.zeros((1001, 11, 6), np.float32), np.zeros(1001, np.uint8),
                             np.zeros(1001, np.uint8))
    n0 = len(short_reads[0].starts)
    lab = labels[:n0].copy()
    lab[400:] = 0xFF
    assert 0 < rv.fit_add_packed(_pack(rv, short_reads[:1]), lab) == rv.fit_count() <= 1000
    rv.fit_reset()
    rv.fit_set_depth("signal")                             # the signal depth's cap is its own
    assert rv.fit_add_packed(_pack(rv, short_reads), labels) > 1000
    rv.close()


# ---- 2. the gradient -------------------------------------------------------------------------------------------------------
WORST = {}


def _check_gradient(rv, case, grade_bound):
    T, model, n, kind, act = case
    C_ = fc.n_class(model)
    feat, sig, y, th = _set_case(rv, case)
    fz = _frozen(model)
    rv.fit_begin(model, th)
    g, st = rv.fit_grad(model, np.arange(n))
    ref = fc.grad_reference(*case)
    grades = fc.device_grades(g, st.ce_sum, st.center_sum, ref, T, C_)
    WORST[case] = max(grades.values())
    print(case, {k: round(v, 3) for k, v in grades.items()}, "bounds", round(grade_bound, 3), fc.K_RECORDED, "worst so far",
          round(max(WORST.values()), 3))
    assert g.size == ff.n_params(T, C_) and np.isfinite(g).all() and len(grades) == 43
    assert max(grades.values()) <= grade_bound, grades
    assert max(grades.values()) <= fc.K_RECORDED, grades
    s64 = ref["st64"]
    assert (st.rows, st.correct, st.steps, st.nonfinite) == (n, s64.correct, 0, 0)
    assert rv.fit_params(model)[0].tobytes() == th.tobytes() and rv.fit_params(model)[1] == 0     # nothing was updated
    g1, st1 = rv.fit_grad(model, np.arange(n))
    assert g1.tobytes() == g.tobytes() and st1 == st                                           # the same call, the same bytes
    sp = fc.spans(T, C_)
    for k in U_TENSORS:
        if T == 1:                                         # no step has a step before it: gU is exactly zero
            assert g[sp[k]].tobytes() == bytes(4 * (sp[k].stop - sp[k].start)), k
        else:
            assert g[sp[k]].any(), k
    assert all(g[sp[k]].any() for k in fc.READ_TENSORS + sc_.SIG_TENSORS if k not in U_TENSORS)
    # forward only: p is the definition's within f32, the same counts and sums as the gradient call's
    p, se = rv.fit_eval(model, np.arange(n))
    p64 = ff.forward(feat, sig, th, *fz, T, C_, act, np.float64)[7]
    print(case, "nrv_fit_eval: max |p - p64| =", float(np.abs(p - p64).max()), "bound", 64 * tc.EPS32)
    assert np.abs(p - p64).max() <= 64 * tc.EPS32
    assert (se.rows, se.correct, se.ce_sum, se.center_sum) == (n, st.correct, st.ce_sum, st.center_sum)


@pytest.mark.parametrize("case", fc.GRAD_CASES, ids=IDS)
def test_gradient_against_the_definition(handles, grade_bound, case):
    _check_gradient(handles(case[0], case[4]), case, grade_bound)


def test_a_batch_of_two_scratch_chunks(handles, grade_bound):
    """No handle has a chunk setting, so the chunked batch is held to the definition as every other case is."""
    _check_gradient(handles(CHUNK_CASE[0], CHUNK_CASE[4]), CHUNK_CASE, grade_bound)


# ---- 3. real windows -------------------------------------------------------------------------------------------------------
def test_real_windows_gather_and_forward(species_models, short_reads, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    from oracle import nrv_oracle as O
    from oracle import torch_cpu as TC
    from test_gpu_lstm3fit import _xin_numpy, _xin_torch
    m1, m2 = species_models["ecoli"]
    labels = _labels_for(short_reads)
    w, y1, y2 = tf.labelled_windows(labels, [len(r.starts) for r in short_reads], 11)
    sets, ps = {}, []
    for mode in ("f32", "f16x2"):
        rv = _engine(monkeypatch, m1, m2, precision=mode)
        assert rv.fit_add_packed(_pack(rv, short_reads), labels) == rv.fit_count() == w.size > 1000
        assert rv.precision == mode
        sets[mode] = rv.fit_get_rows_full()
        if mode == "f16x2":
            for k in (0, 1):
                rv.fit_begin(k)                            # the handle's own tensors
                p, st = rv.fit_eval(k, _all_rows(rv))
                assert st.rows == w.size and st.steps == 0 and st.nonfinite == 0
                ps.append(p)
                th, _ = rv.fit_params(k)
                assert th.tobytes() == ff.params_from_model((m1, m2)[k]).tobytes()               # as the file has them
            rv.fit_reset()
            rv.fit_set_depth("signal")                     # the same handle's rows at signal depth
            assert rv.fit_add_packed(_pack(rv, short_reads), labels) == w.size
            rows_s = rv.fit_get_rows_signal()
        rv.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(sets["f32"], sets["f16x2"]))
    sig_set, feat_set = sets["f32"][:2]
    assert np.array_equal(sets["f32"][2], y1) and np.array_equal(sets["f32"][3], y2) and feat_set.shape == (w.size, 11, 6)
    feat_ev = np.concatenate([r.feat_ev for r in short_reads]).astype(np.float32)
    all_idx = w[:, None] + np.arange(11)[None, :]
    assert sig_set.tobytes() == rows_s[2].tobytes()        # what the signal depth gathers
    assert feat_set.tobytes() == np.ascontiguousarray(feat_ev[all_idx]).tobytes()
    rp = Reviser(m1, m2, precision="f32")
    pred = rp.predict_reads_raw(*_args(short_reads))
    rp.close()
    pick = np.linspace(0, w.size - 1, 128).astype(np.int64)
    sig, rd = sig_set[pick], feat_set[pick]
    q64 = O.predict_pair(m1.tensors, m2.tensors, sig, rd, np.float64)
    q32 = O.predict_pair(m1.tensors, m2.tensors, sig, rd, np.float32)
    qt = TC.predict_pair(TC.TorchCpuModel(m1.tensors), TC.TorchCpuModel(m2.tensors), sig.astype(np.float32), rd.astype(np.float32))
    for k, m in enumerate((m1, m2)):
        # X2b by the definition at float64 against the x2 the signal depth gathered (the inference kernels' own output), within
        # the f32 floor two CPU restatements of those columns form against the fp64 oracle's
        with np.errstate(over="ignore"):
            f64 = _xin_numpy(m.tensors, sig, rd, np.float64)[:, :, :128].reshape(128, -1)
            d_np = np.abs(_xin_numpy(m.tensors, sig, rd, np.float32)[:, :, :128].reshape(128, -1) - f64).max(-1)
        d_t = np.abs(_xin_torch(m.tensors, sig, rd)[:, :, :128].reshape(128, -1) - f64).max(-1)
        scale = np.abs(f64).max(-1)
        K = _row_bound(d_np, d_t, scale)
        X2b = ff.forward(rd, sig, ff.params_from_model(m), ff.read_bn(m), sf.conv_bn(m), *l4.bn_scale_shift(m), 11, m.n_class, 0,
                         np.float64)[0].reshape(128, -1)
        d_dev = np.abs(rows_s[k][pick].reshape(128, -1).astype(np.float64) - X2b).max(-1)
        grades = [tc.grade_of(d, max(a, b), s) for d, a, b, s in zip(d_dev, d_np, d_t, scale)]
        print(f"model{k + 1}: X2b of the definition against the signal depth's x2, worst grade {max(grades):.3g} (bound {K:.3g})")
        assert max(grades) <= K, (k, max(grades), K)
        p64 = q64[k]
        e_np, e_t = np.abs(q32[k] - p64).max(-1), np.abs(qt[k] - p64).max(-1)
        Kp = _row_bound(e_np, e_t, np.ones(128))
        p_fit, p_pred = ps[k][pick], pred[k][w][pick]
        for name, p in (("nrv_fit_eval", p_fit), ("nrv_predict", p_pred)):
            gr = [tc.grade_of(d, max(a, b), 1.0) for d, a, b in zip(np.abs(p - p64).max(-1), e_np, e_t)]
            print(f"model{k + 1}: {name} p, worst grade {max(gr):.3g} (bound {Kp:.3g})")
            assert max(gr) <= Kp, (k, name, max(gr), Kp)
        nf = np.maximum(e_np, e_t)
        srt = np.sort(p64, -1)
        margin = srt[:, -1] - srt[:, -2]
        for i in np.nonzero(p_fit.argmax(-1) != p_pred.argmax(-1))[0]:
            assert margin[i] <= 2 * max(nf[i], 1e-6), (k, int(i), float(margin[i]), float(nf[i]))


# ---- 4. one update ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(11, 1, 33, "plain", 0), (1, 0, 33, "plain", 0), (11, 0, 33, "edges", 0)], ids=IDS)
def test_one_step_is_numpy_f32_adam_bit_for_bit(handles, case):
    T, model, n, kind, act = case
    rv = handles(T, act)
    feat, sig, y, th = _set_case(rv, case)
    opts = tf.default_opts(model)
    rv.fit_begin(model, th, opts)
    g, _ = rv.fit_grad(model, np.arange(n))
    st = rv.fit_epoch(model, np.arange(n))
    got, t = rv.fit_params(model)
    want = tc.adam_f32(th, np.zeros_like(th), np.zeros_like(th), g, opts, 1)[0]
    assert (t, st.steps, st.rows, st.nonfinite) == (1, 1, n, 0)
    assert got.size == ff.n_params(T, 6 - model) and got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8].tolist()
    sp = fc.spans(T, 6 - model)
    moved = {k: not np.array_equal(got[sp[k]], th[sp[k]]) for k in fc.TENSORS}
    assert all(v for k, v in moved.items() if not (T == 1 and k in U_TENSORS)), moved


EPOCH_CASE = (11, 0, 1100, "plain", 0)


def _epoch(rv, th, order, opts):
    rv.fit_begin(0, th, opts)
    st = rv.fit_epoch(0, order)
    return rv.fit_params(0)[0], st


def test_epoch_twice_and_poisoned_give_the_same_bytes(species_models, handles, monkeypatch):
    T, model, n, _, _ = EPOCH_CASE
    rv = handles(T)
    feat, sig, y, th = _set_case(rv, EPOCH_CASE)
    opts = tf.default_opts(model, B=512)                   # batches of 512, 512, 76
    order = np.random.default_rng(4).permutation(n).astype(np.uint32)
    got, st = _epoch(rv, th, order, opts)
    assert (st.steps, st.rows, st.nonfinite) == (3, n, 0) and rv.fit_params(0)[1] == 3 and np.isfinite(got).all()
    again, st2 = _epoch(rv, th, order, opts)
    assert again.tobytes() == got.tobytes() and st2 == st
    # the host loop of nrv_fit_grad + NumPy-f32 Adam is the epoch
    cur, m, v = th.copy(), np.zeros_like(th), np.zeros_like(th)
    for k, s in enumerate(range(0, n, 512), 1):
        rv.fit_begin(0, cur, opts)
        g, _ = rv.fit_grad(0, order[s:s + 512])
        cur, m, v = tc.adam_f32(cur, m, v, g, opts, k)
    assert cur.tobytes() == got.tobytes(), np.argwhere(cur != got)[:8].tolist()
    for poison in sorted(PATTERNS):
        m1, m2 = species_models["ecoli"]
        pv = _engine(monkeypatch, m1, m2, poison=poison)
        _set_case(pv, EPOCH_CASE)
        pg, pst = _epoch(pv, th, order, opts)
        pv.close()
        assert pg.tobytes() == got.tobytes() and pst == st, poison


# ---- 5. a non-finite batch -------------------------------------------------------------------------------------------------
def test_nonfinite_batch_is_skipped_and_counted(handles):
    T, model, n = 11, 0, 1100
    rv = handles(T)
    feat, sig, y, th = fc.rows_case(*EPOCH_CASE)
    feat = feat.copy()
    feat[600, 3, 2] = np.inf                               # the second batch of 512
    rv.fit_set_rows_full(sig, feat, y, np.minimum(y, 4))
    opts = tf.default_opts(model, B=512)
    order = np.arange(n, dtype=np.uint32)
    rv.fit_begin(model, th, opts)
    st = rv.fit_epoch(model, order[512:1024])              # that batch alone: counted, and the parameters keep their bytes
    got, t = rv.fit_params(model)
    assert (t, st.steps, st.nonfinite, st.rows) == (0, 0, 1, 0) and got.tobytes() == th.tobytes()
    st = rv.fit_epoch(model, order)
    got, t = rv.fit_params(model)
    assert (t, st.steps, st.nonfinite, st.rows) == (2, 2, 1, 588) and np.isfinite(got).all()
    assert math.isfinite(st.ce_sum) and math.isfinite(st.center_sum) and not np.array_equal(got, th)
    g, sg = rv.fit_grad(model, order[512:1024])
    assert sg.nonfinite == 1 and not np.isfinite(g).all()
    keep = np.concatenate([order[:512], order[1024:]])     # the same epoch without the batch: the same bytes, t included
    rv.fit_begin(model, th, opts)
    st2 = rv.fit_epoch(model, keep)
    assert rv.fit_params(model)[0].tobytes() == got.tobytes() and rv.fit_params(model)[1] == 2 and st2.nonfinite == 0


# ---- 6. it learns ----------------------------------------------------------------------------------------------------------
LEARN_E = 4


def test_it_learns_from_perturbed_read_lstms_and_the_written_model_runs(species_models, short_reads, monkeypatch, tmp_path):
    """The shipped ecoli model with lstm1 and lstm2 perturbed (every one of their 52 608 weights x 0.9 .. 1.1, seeded), every window
    of the two shortest fixture reads labelled with the answers the UNPERTURBED model gives in f32 mode, LEARN_E epochs at the
    defaults.  Asserted: the last epoch's training loss is below the first's; the forty fitted tensors all moved while the
    twenty BatchNorm tensors keep their bytes; the written model runs in a new handle in every precision mode, and its f32
    nrv_predict* agrees with nrv_fit_eval under the tie rule."""
    from nanoreviser_amd.engine import Reviser
    from nanoreviser_amd.weights import load_model
    m1, m2 = species_models["ecoli"]
    el = [len(r.starts) for r in short_reads]
    labels = np.full(sum(el), 5, np.uint8)                 # every window of either read is labelled ...
    w = tf.labelled_windows(labels, el, 11)[0]
    teacher = Reviser(m1, m2, precision="f32")
    _, _, a1, a2 = teacher.predict_reads_raw(*_args(short_reads))
    teacher.close()
    y1, y2 = a1[w].astype(np.uint8), a2[w].astype(np.uint8)
    rv = _engine(monkeypatch, m1, m2)
    n = rv.fit_add_packed(_pack(rv, short_reads), labels)
    assert n == w.size == sum(el) - 22
    sig, feat, _, _ = rv.fit_get_rows_full()
    rv.fit_set_rows_full(sig, feat, y1, y2)                # ... with the teacher's answers
    rng = np.random.default_rng(11)
    backs, finals = [], []
    for k, m in enumerate((m1, m2)):
        start = ff.params_from_model(m)
        start[:ff.N_READ] *= rng.uniform(0.9, 1.1, ff.N_READ).astype(np.float32)
        rv.fit_begin(k, start, tf.default_opts(k))
        before = rv.fit_eval(k, _all_rows(rv), want_p=False)[1].loss()[0]
        hist = [rv.fit_epoch(k, tf.epoch_order(n, 3, ep)) for ep in range(LEARN_E)]
        after = rv.fit_eval(k, _all_rows(rv), want_p=False)[1].loss()[0]
        loss = [h.loss()[0] for h in hist]
        print(f"model{k + 1}: loss before {before:.4f}, epochs {loss[0]:.4f} -> {loss[-1]:.4f}, after {after:.4f}, "
              f"acc {hist[0].acc():.4f} -> {hist[-1].acc():.4f}")
        assert all(h.nonfinite == 0 for h in hist) and loss[-1] < loss[0] and after < before
        theta, t = rv.fit_params(k)
        fm = ff.fitted_model(m, theta)
        assert all(fm.tensors[i].tobytes() == m.tensors[i].tobytes() for i in BN_IDS)
        assert all(not np.array_equal(fm.tensors[i], m.tensors[i]) for i in FITTED)               # all forty were fitted
        tf.write_f32(fm, str(tmp_path / f"m{k}"))
        backs.append(load_model(str(tmp_path / f"m{k}.f32")))
        finals.append(rv.fit_eval(k, _all_rows(rv))[0])
    rv.close()
    preds = {}
    for mode in ("f32", "f16x2", "bf16x3"):
        rv2 = Reviser(backs[0], backs[1], precision=mode)
        preds[mode] = rv2.predict_reads_raw(*_args(short_reads))
        rv2.close()
        assert all(np.isfinite(preds[mode][k]).all() for k in (0, 1)), mode
    for k in (0, 1):
        p_fit, p_pred = finals[k], preds["f32"][k][w]
        d = np.abs(p_fit - p_pred).max(-1)
        print(f"model{k + 1}: written model against nrv_fit_eval, max |dp| = {float(d.max()):.3g}")
        assert d.max() <= 1e-4                             # (two f32 evaluations of one model; 64 roundings of a probability are 8e-6)
        srt = np.sort(p_fit.astype(np.float64), -1)
        margin = srt[:, -1] - srt[:, -2]
        for i in np.nonzero(p_fit.argmax(-1) != p_pred.argmax(-1))[0]:
            assert margin[i] <= 2 * max(d[i], 1e-6), (k, int(i), float(margin[i]), float(d[i]))


# ---- 7. the other depths ---------------------------------------------------------------------------------------------------
def test_signal_depth_keeps_its_bytes_after_this_depth(species_models, handles, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    case = (11, 1, 33, "plain", 0)
    x2, sig, y, th = sc_.rows_case(*case)

    def grad_s(rv):
        rv.fit_set_rows_signal(x2, x2, sig, np.minimum(y, 4), y)
        rv.fit_begin(1, th)
        return rv.fit_grad(1, np.arange(33))

    used = handles(11)                                     # a handle this depth has run on
    _set_case(used, case)
    used.fit_begin(1, fc.rows_case(*case)[3])
    used.fit_grad(1, np.arange(33))
    used.fit_reset()
    used.fit_set_depth("signal")
    g_used, st_used = grad_s(used)
    used.fit_reset()
    used.fit_set_depth("full")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    fresh = Reviser(*species_models["ecoli"])
    fresh.fit_set_depth("signal")
    g_fresh, st_fresh = grad_s(fresh)
    fresh.close()
    assert g_used.tobytes() == g_fresh.tobytes() and st_used == st_fresh


# ---- 8. command line -------------------------------------------------------------------------------------------------------
def test_command_line_trains_the_whole_model_that_model_dir_runs(tmp_path, monkeypatch, species_models):
    """tests/test_gpu_lstm4fit.py's command-line run at the last depth: --labels, NanoReviser_train.py --fit_depth full -e 1, then
    NanoReviser.py --model_dir on the written directory, in the default precision mode and with --score."""
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
    assert train_cli.main(["-d", str(d), "-S", "ecoli", "-M", mdir, "-e", "1", "--fit_depth", "full", "--labels_from", ldir],
                          reviser_factory=factory) == 0
    rv = made[0]
    try:
        assert rv.fit_depth() == 32 and rv.fit_count() > 1000
        for k, m in enumerate(species_models["ecoli"]):
            stem = train_cli.stem(mdir, "ecoli", k + 1)
            back = load_model(stem + ".f32")
            assert back.T == 11 and back.n_class == m.n_class and np.isfinite(back.flat()).all()
            assert all(back.tensors[i].tobytes() == m.tensors[i].tobytes() for i in BN_IDS)
            assert all(not np.array_equal(back.tensors[i], m.tensors[i]) for i in FITTED)             # all forty were fitted
            theta, t = rv.fit_params(k)
            assert theta.size == ff.n_params(11, m.n_class) and t > 0
            assert all(back.tensors[i].tobytes() == a.tobytes() for i, a in zip(FITTED, ff.unpack(theta, 11, m.n_class)[:40]))
            s = json.load(open(stem + "_summary.json"))
            assert s["rows"] == rv.fit_count() and s["options"]["init"] == "transfer" and s["options"]["fit_depth"] == "full"
    finally:
        Reviser.close(rv)
    sc = str(tmp_path / "score.tsv")
    assert cli.main(common + ["-o", str(tmp_path / "B") + "/", "--model_dir", mdir, "--score", sc, "--labels_from", ldir]) == 0
    lines = open(sc).read().split("\n")
    assert lines[0] == cli.SCORE_HEADER and [ln.split("\t")[1] for ln in lines[1:3]] == ["scored", "scored"]
    assert all(os.path.getsize(str(tmp_path / "B" / f"s{i:02d}_out.fasta")) > 1000 for i in range(2))
