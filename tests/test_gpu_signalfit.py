"""Fitting the signal branch with lstm3 and everything behind it on the device (MI355X only, -m gpu): csrc/nrv_signalfit.h through
the nrv_fit_* entry points at depth NRV_FIT_SIGNAL.  nanoreviser_amd/signalfit.py is the definition; tests/signalfit_cases.py
holds the cases, the two f32 restatements and the floors.  Every tolerance is sized from CPU restatements against the float64
definition.
  1. doors and refusals: the _signal doors round-trip bytes; every door refused by name at the four other depths and in flight;
     depth 16 accepted, 10 .. 15 and 17 refused; NRV_FIT_MAX_SIGNAL_ROWS; a parameter count of another depth;
  2. gradient: every case through the unit doors and nrv_fit_grad, per tensor (29) and sum within cpu_bound(); counts exact;
     T = 1 gives gU3 and gU4 bytes of zero; `edges`, all-zero rows and a batch of two scratch chunks (4130 rows) the same way;
  3. real windows: the set gathered from the short fixture reads is the same bytes from f32 and f16x2 mode; x2 is columns 0 .. 127
     of the rows the same handle gathers at depth lstm3, sig the windows of nrv_segment_reads' event signals, byte for byte; S
     recomputed by signalfit.forward at float64 within the f32 floor of columns 128 .. 191; nrv_fit_eval at the handle's own
     tensors within the bound of the fp64 oracle and equal to the f32 mode's nrv_predict* under the tie rule;
  4. one update = tailfit_cases.adam_f32 on nrv_fit_grad's vector, byte for byte; a three-batch epoch twice and under poison;
  5. a row holding inf in sig: its batch is counted in nonfinite and the parameters keep their bytes;
  6. it learns from the shipped start with a perturbed conv block, and the written model runs in a new handle in every mode;
  7. the lstm3 depth's nrv_fit_grad gives a fresh handle's bytes after this depth has been used in the process."""
import math

import numpy as np
import pytest

import lstm3fit_cases as l3c
import signalfit_cases as sc_
import tailfit_cases as tc
from nanoreviser_amd import headfit as hf
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import lstm3fit as l3
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.engine import FIT_SIGNAL, NrvError
from test_gpu_headfit import _all_rows, _args, _labels_for, _pack
from test_gpu_lstm4fit import _row_bound

pytestmark = pytest.mark.gpu

PATTERNS = {"qnan": 0x7FC00000, "m1500": 0xC4BB8000}
ENV = ("NRV_PRECISION", "NRV_COALESCE", "NRV_LANES", "NRV_POISON", "NRV_FIT_MAX_ROWS", "NRV_FIT_MAX_HEAD_ROWS", "NRV_FIT_MAX_LSTM4_ROWS",
       "NRV_FIT_MAX_LSTM3_ROWS", "NRV_FIT_MAX_SIGNAL_ROWS")
IDS = lambda c: "T%d-m%d-n%d-%s-act%d" % c      # noqa: E731
CHUNK_CASE = sc_.CHUNK_CASE                     # 8260 (row, t) pairs: one scratch chunk of 4096 rows and a second of 34, the last tile short
SIG_IDS = (0, 1, 6, 7, 32, 33)
FITTED = list(SIG_IDS) + list(range(34, 40)) + list(range(44, 60))
FROZEN = [i for i in range(60) if i not in FITTED]
U_TENSORS = ("U3f", "U3b", "U4f", "U4b")


def _engine(monkeypatch, m1, m2, poison=None, **kw):
    from nanoreviser_amd.engine import Reviser
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if poison is not None:
        monkeypatch.setenv("NRV_POISON", f"{PATTERNS[poison]:08x}")
    rv = Reviser(m1, m2, **kw)
    monkeypatch.delenv("NRV_POISON", raising=False)
    rv.fit_set_depth("signal")
    assert rv.fit_depth() == FIT_SIGNAL == 16
    assert rv.fit_n_params(0) == sf.n_params(rv.T, 6) and rv.fit_n_params(1) == sf.n_params(rv.T, 5)
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
    """One signal-depth handle per (window length, recurrent_act), made on first use and shared.  Their frozen BatchNorms are the
    shipped ecoli ones, as signalfit_cases.conv_bn and .bn are."""
    from nanoreviser_amd.engine import Reviser
    made = {}

    def get(T, act=0):
        if (T, act) not in made:
            m1, m2 = species_models["ecoli"]
            made[T, act] = Reviser(m1.with_window(T), m2.with_window(T), recurrent_activation="sigmoid" if act else "hard_sigmoid")
            made[T, act].fit_set_depth("signal")
        return made[T, act]
    yield get
    for rv in made.values():
        rv.close()


def _set_case(rv, case):
    T, model, n, kind, act = case
    x2, sig, y, th = sc_.rows_case(*case)
    other = np.minimum(y, 4)
    rv.fit_set_rows_signal(x2, x2, sig, y if model == 0 else other, other if model == 0 else y)
    assert rv.fit_count() == n
    return x2, sig, y, th


@pytest.fixture(scope="module")
def grade_bound():
    K, worst = sc_.cpu_bound()
    print(f"signal depth: gradient bound sized on the CPU: K = {K:.3g} (worst restatement grade {worst:.3g})")
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
    xin = rng.normal(0, 1, (n, 11, 192)).astype(np.float32)
    xb = rng.normal(0, 1, (n, 11, 256)).astype(np.float32)
    F = rng.uniform(0, 1, (n, 66)).astype(np.float32)
    y1, y2 = rng.integers(0, 6, n).astype(np.uint8), rng.integers(0, 5, n).astype(np.uint8)
    none4, none5 = (None,) * 4, (None,) * 5
    # the four other depths: the _signal doors are refused under their own names
    for depth, word in (("tail", "tail depth"), ("head", "head depth"), ("lstm4", "lstm4 depth"), ("lstm3", "lstm3 depth")):
        rv.fit_set_depth(depth)
        with pytest.raises(NrvError, match="nrv_fit_set_rows_signal: the set is at " + word):
            rv.fit_set_rows_signal(x1, x2, sg, y1, y2)
        refused(lib.nrv_fit_get_rows_signal(h, 0, 0, *none5), "nrv_fit_get_rows_signal", word)
    rv.fit_set_depth("tail")
    for bad in (2, 3, 5, 6, 7, 9, -1, 10, 11, 12, 13, 14, 15, 17):
        refused(lib.nrv_fit_set_depth(h, bad), "nrv_fit_set_depth", "NRV_FIT_TAIL or NRV_FIT_HEAD")
        assert "NRV_FIT_SIGNAL" in lib.nrv_last_error(h).decode()
    # signal depth: 16 is accepted on the empty set; the four other depths' doors are refused
    assert lib.nrv_fit_set_depth(h, 16) == 0 and rv.fit_depth() == 16 and rv.fit_count() == 0
    with pytest.raises(NrvError, match="nrv_fit_set_rows: the set is at signal depth"):
        rv.fit_set_rows(F, F, y1, y2)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_head: the set is at signal depth"):
        rv.fit_set_rows_head(x1, x1, y1, y2)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_lstm4: the set is at signal depth"):
        rv.fit_set_rows_lstm4(xb, xb, y1, y2)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_lstm3: the set is at signal depth"):
        rv.fit_set_rows_lstm3(xin, xin, y1, y2)
    for name in ("nrv_fit_get_rows", "nrv_fit_get_rows_head", "nrv_fit_get_rows_lstm4", "nrv_fit_get_rows_lstm3"):
        refused(getattr(lib, name)(h, 0, 0, *none4), name, "signal depth")
    refused(lib.nrv_fit_set_rows_signal(h, None, None, None, None, None, 4), "nrv_fit_set_rows_signal", "null rows")
    with pytest.raises(NrvError, match="nrv_fit_set_rows_signal: a label outside"):
        rv.fit_set_rows_signal(x1, x2, sg, np.full(n, 6, np.uint8), y2)
    refused(lib.nrv_fit_params(h, 0, None, None), "nrv_fit_params", "nrv_fit_begin")          # the depth change forgot any begin
    # the doors round-trip bytes, sub-ranges too
    rv.fit_set_rows_signal(x1, x2, sg, y1, y2)
    assert rv.fit_count() == n
    got = rv.fit_get_rows_signal()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, (x1, x2, sg, y1, y2)))
    for first, count in ((0, 1), (31, 33), (76, 1), (77, 0)):
        sub = rv.fit_get_rows_signal(first, count)
        assert all(a.tobytes() == b[first:first + count].tobytes() for a, b in zip(sub, (x1, x2, sg, y1, y2))), (first, count)
    with pytest.raises(NrvError, match="nrv_fit_get_rows_signal: rows outside the training set"):
        rv.fit_get_rows_signal(70, 8)
    with pytest.raises(ValueError):
        rv.fit_set_rows_signal(xin, xin, sg, y1, y2)
    for d in (0, 1, 4, 8):
        refused(lib.nrv_fit_set_depth(h, d), "nrv_fit_set_depth", "not empty")
    # a parameter count of another depth is refused
    for other in (tf.n_params(11, 6), hf.n_params(11, 6), l4.n_params(11, 6), l3.n_params(11, 6)):
        with pytest.raises(ValueError, match=f"expected {sf.n_params(11, 6)} parameters, got {other}"):
            rv.fit_begin(0, np.zeros(other, np.float32))
    rv.fit_begin(0)
    rows = np.arange(33, dtype=np.uint32)
    want_g, want_st = rv.fit_grad(0, rows)
    assert want_g.size == sf.n_params(11, 6) == 25896 + 328704 + 164352 + 20838 + tf.n_params(11, 6)
    # in flight: the depth cannot change and the doors are refused under their own names
    t = rv.begin_packed_raw(_pack(rv, short_reads[:1]))
    refused(lib.nrv_fit_set_depth(h, 0), "nrv_fit_set_depth", "in flight")
    refused(lib.nrv_fit_set_rows_signal(h, None, None, None, None, None, 0), "nrv_fit_set_rows_signal", "in flight")
    refused(lib.nrv_fit_get_rows_signal(h, 0, 0, *none5), "nrv_fit_get_rows_signal", "in flight")
    assert lib.nrv_fit_depth(h) == 16
    rv.end_packed_raw(t)
    g3, st3 = rv.fit_grad(0, rows)
    assert g3.tobytes() == want_g.tobytes() and st3 == want_st and rv.fit_count() == n          # the handle stayed usable
    rv.close()
    # a handle under NRV_FIT_MAX_SIGNAL_ROWS = 1000 refuses an adding call whole, by that name, and stays usable
    monkeypatch.setenv("NRV_FIT_MAX_SIGNAL_ROWS", "1000")
    rv = Reviser(*species_models["ecoli"])
    monkeypatch.delenv("NRV_FIT_MAX_SIGNAL_ROWS")
    rv.fit_set_depth("signal")
    labels = _labels_for(short_reads)
    with pytest.raises(NrvError) as e:
        rv.fit_add_packed(_pack(rv, short_reads), labels)
    assert e.value.code == -1 and "nrv_fit_add_reads_raw: the call would pass the row cap" in str(e.value) and "NRV_FIT_MAX_SIGNAL_ROWS" in str(e.value)
    assert rv.fit_count() == 0
    z = np.zeros((1001, 11, 128), np.float32)
    with pytest.raises(NrvError, match="NRV_FIT_MAX_SIGNAL_ROWS"):
        rv.fit_set_rows_signal(z, z, np.zeros((1001, 11, 50), np.float32), np.zeros(1001, np.uint8), np.zeros(1001, np.uint8))
    n0 = len(short_reads[0].starts)
    lab = labels[:n0].copy()
    lab[400:] = 0xFF
    assert 0 < rv.fit_add_packed(_pack(rv, short_reads[:1]), lab) == rv.fit_count() <= 1000
    rv.fit_reset()
    rv.fit_set_depth("lstm3")                              # the lstm3 depth's cap is its own
    assert rv.fit_add_packed(_pack(rv, short_reads), labels) > 1000
    rv.close()


# ---- 2. the gradient -------------------------------------------------------------------------------------------------------
WORST = {}


def _check_gradient(rv, case, grade_bound):
    T, model, n, kind, act = case
    C_ = sc_.n_class(model)
    x2, sig, y, th = _set_case(rv, case)
    cb = sc_.conv_bn(model)
    sc, sh = sc_.bn(model)
    rv.fit_begin(model, th)
    g, st = rv.fit_grad(model, np.arange(n))
    ref = sc_.grad_reference(*case)
    grades = sc_.device_grades(g, st.ce_sum, st.center_sum, ref, T, C_)
    WORST[case] = max(grades.values())
    print(case, {k: round(v, 3) for k, v in grades.items()}, "bound", round(grade_bound, 3), "worst so far", round(max(WORST.values()), 3))
    assert g.size == sf.n_params(T, C_) and np.isfinite(g).all() and len(grades) == 31
    assert max(grades.values()) <= grade_bound, grades
    s64 = ref["st64"]
    assert (st.rows, st.correct, st.steps, st.nonfinite) == (n, s64.correct, 0, 0)
    assert rv.fit_params(model)[0].tobytes() == th.tobytes() and rv.fit_params(model)[1] == 0     # nothing was updated
    g1, st1 = rv.fit_grad(model, np.arange(n))
    assert g1.tobytes() == g.tobytes() and st1 == st                                           # the same call, the same bytes
    sp = sc_.spans(T, C_)
    for k in U_TENSORS:
        if T == 1:                                         # no step has a step before it: gU is exactly zero
            assert g[sp[k]].tobytes() == bytes(4 * (sp[k].stop - sp[k].start)), k
        else:
            assert g[sp[k]].any(), k
    assert all(g[sp[k]].any() for k in sc_.SIG_TENSORS)
    # forward only: p is the definition's within f32, the same counts and sums as the gradient call's
    p, se = rv.fit_eval(model, np.arange(n))
    p64 = sf.forward(x2, sig, th, cb, sc, sh, T, C_, act, np.float64)[6]
    print(case, "nrv_fit_eval: max |p - p64| =", float(np.abs(p - p64).max()), "bound", 64 * tc.EPS32)
    assert np.abs(p - p64).max() <= 64 * tc.EPS32
    assert (se.rows, se.correct, se.ce_sum, se.center_sum) == (n, st.correct, st.ce_sum, st.center_sum)


@pytest.mark.parametrize("case", sc_.GRAD_CASES, ids=IDS)
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
        sets[mode] = rv.fit_get_rows_signal()
        if mode == "f16x2":
            for k in (0, 1):
                rv.fit_begin(k)                            # the handle's own tensors
                p, st = rv.fit_eval(k, _all_rows(rv))
                assert st.rows == w.size and st.steps == 0 and st.nonfinite == 0
                ps.append(p)
                th, _ = rv.fit_params(k)
                assert th.tobytes() == sf.params_from_model((m1, m2)[k]).tobytes()               # as the file has them
            rv.fit_reset()
            rv.fit_set_depth("lstm3")                      # the same handle's rows at depth lstm3
            assert rv.fit_add_packed(_pack(rv, short_reads), labels) == w.size
            rows3 = rv.fit_get_rows_lstm3()
        rv.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(sets["f32"], sets["f16x2"]))
    x2s, sig_set = sets["f32"][:2], sets["f32"][2]
    assert np.array_equal(sets["f32"][3], y1) and np.array_equal(sets["f32"][4], y2) and x2s[0].shape == (w.size, 11, 128)
    rp = Reviser(m1, m2, precision="f32")
    pred = rp.predict_reads_raw(*_args(short_reads))
    raws, starts, _, shifts, scales = _args(short_reads)
    sig_ev = rp.segment_reads(raws, starts, shifts, scales)           # nrv_segment_reads: the event signals of both reads
    rp.close()
    feat_ev = np.concatenate([r.feat_ev for r in short_reads])
    all_idx = w[:, None] + np.arange(11)[None, :]
    for k in (0, 1):
        assert x2s[k].tobytes() == np.ascontiguousarray(rows3[k][:, :, :128]).tobytes(), k
    assert sig_set.tobytes() == np.ascontiguousarray(sig_ev[all_idx]).tobytes()
    pick = np.linspace(0, w.size - 1, 128).astype(np.int64)
    idx = all_idx[pick]
    sig, rd = sig_ev[idx], feat_ev[idx]
    q64 = O.predict_pair(m1.tensors, m2.tensors, sig, rd, np.float64)
    q32 = O.predict_pair(m1.tensors, m2.tensors, sig, rd, np.float32)
    qt = TC.predict_pair(TC.TorchCpuModel(m1.tensors), TC.TorchCpuModel(m2.tensors), sig.astype(np.float32), rd.astype(np.float32))
    for k, m in enumerate((m1, m2)):
        # S by the definition at float64 against columns 128 .. 191 of the lstm3 rows, within the f32 floor two CPU
        # restatements of those columns form against the fp64 oracle's
        with np.errstate(over="ignore"):
            f64 = _xin_numpy(m.tensors, sig, rd, np.float64)[:, :, 128:].reshape(128, -1)
            d_np = np.abs(_xin_numpy(m.tensors, sig, rd, np.float32)[:, :, 128:].reshape(128, -1) - f64).max(-1)
        d_t = np.abs(_xin_torch(m.tensors, sig, rd)[:, :, 128:].reshape(128, -1) - f64).max(-1)
        scale = np.abs(f64).max(-1)
        K = _row_bound(d_np, d_t, scale)
        S = sf.forward(x2s[k][pick], sig_set[pick], sf.params_from_model(m), sf.conv_bn(m), *l4.bn_scale_shift(m), 11, m.n_class, 0,
                       np.float64)[0].reshape(128, -1)
        d_dev = np.abs(rows3[k][pick][:, :, 128:].reshape(128, -1).astype(np.float64) - S).max(-1)
        grades = [tc.grade_of(d, max(a, b), s) for d, a, b, s in zip(d_dev, d_np, d_t, scale)]
        print(f"model{k + 1}: S of the definition against the lstm3 rows, worst grade {max(grades):.3g} (bound {K:.3g})")
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
    x2, sig, y, th = _set_case(rv, case)
    opts = tf.default_opts(model)
    rv.fit_begin(model, th, opts)
    g, _ = rv.fit_grad(model, np.arange(n))
    st = rv.fit_epoch(model, np.arange(n))
    got, t = rv.fit_params(model)
    want = tc.adam_f32(th, np.zeros_like(th), np.zeros_like(th), g, opts, 1)[0]
    assert (t, st.steps, st.rows, st.nonfinite) == (1, 1, n, 0)
    assert got.size == sf.n_params(T, 6 - model) and got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8].tolist()
    sp = sc_.spans(T, 6 - model)
    moved = {k: not np.array_equal(got[sp[k]], th[sp[k]]) for k in sc_.TENSORS}
    assert all(v for k, v in moved.items() if not (T == 1 and k in U_TENSORS)), moved


EPOCH_CASE = (11, 0, 1100, "plain", 0)


def _epoch(rv, th, order, opts):
    rv.fit_begin(0, th, opts)
    st = rv.fit_epoch(0, order)
    return rv.fit_params(0)[0], st


def test_epoch_twice_and_poisoned_give_the_same_bytes(species_models, handles, monkeypatch):
    T, model, n, _, _ = EPOCH_CASE
    rv = handles(T)
    x2, sig, y, th = _set_case(rv, EPOCH_CASE)
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
    x2, sig, y, th = sc_.rows_case(*EPOCH_CASE)
    sig = sig.copy()
    sig[600, 3, 7] = np.inf                                # the second batch of 512
    rv.fit_set_rows_signal(x2, x2, sig, y, np.minimum(y, 4))
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


def test_it_learns_from_a_perturbed_conv_block_and_the_written_model_runs(species_models, short_reads, monkeypatch, tmp_path):
    """The shipped ecoli model with its conv block perturbed (kernels and biases of both convolutions x 0.9 .. 1.1, seeded), every
    window of the two shortest fixture reads labelled with the answers the UNPERTURBED model gives in f32 mode, LEARN_E epochs at
    the defaults.  Asserted: the last epoch's training loss is below the first's; the twenty-eight fitted tensors all moved while
    the frozen ones keep their bytes; the written model runs in a new handle in every precision mode, and its f32 nrv_predict*
    agrees with nrv_fit_eval under the tie rule."""
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
    x1, x2, sig, _, _ = rv.fit_get_rows_signal()
    rv.fit_set_rows_signal(x1, x2, sig, y1, y2)            # ... with the teacher's answers
    rng = np.random.default_rng(11)
    backs, finals = [], []
    for k, m in enumerate((m1, m2)):
        start = sf.params_from_model(m)
        start[:sf.N_SIGNAL - 25664] *= rng.uniform(0.9, 1.1, 232).astype(np.float32)
        rv.fit_begin(k, start, tf.default_opts(k))
        hist = [rv.fit_epoch(k, tf.epoch_order(n, 3, ep)) for ep in range(LEARN_E)]
        loss = [h.loss()[0] for h in hist]
        print(f"model{k + 1}: loss {loss[0]:.4f} -> {loss[-1]:.4f}, acc {hist[0].acc():.4f} -> {hist[-1].acc():.4f}")
        assert all(h.nonfinite == 0 for h in hist) and loss[-1] < loss[0]
        theta, t = rv.fit_params(k)
        fm = sf.fitted_model(m, theta)
        assert all(fm.tensors[i].tobytes() == m.tensors[i].tobytes() for i in FROZEN)
        assert all(not np.array_equal(fm.tensors[i], m.tensors[i]) for i in FITTED)               # all twenty-eight were fitted
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
def test_lstm3_depth_keeps_its_bytes_after_this_depth(species_models, handles, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    case = (11, 1, 33, "plain", 0)
    X, y, th = l3c.rows_case(*case)

    def grad3(rv):
        rv.fit_set_rows_lstm3(X, X, np.minimum(y, 4), y)
        rv.fit_begin(1, th)
        return rv.fit_grad(1, np.arange(33))

    used = handles(11)                                     # a handle this depth has run on
    _set_case(used, (11, 1, 33, "plain", 0))
    used.fit_begin(1, sc_.rows_case(11, 1, 33, "plain", 0)[3])
    used.fit_grad(1, np.arange(33))
    used.fit_reset()
    used.fit_set_depth("lstm3")
    g_used, st_used = grad3(used)
    used.fit_reset()
    used.fit_set_depth("signal")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    fresh = Reviser(*species_models["ecoli"])
    fresh.fit_set_depth("lstm3")
    g_fresh, st_fresh = grad3(fresh)
    fresh.close()
    assert g_used.tobytes() == g_fresh.tobytes() and st_used == st_fresh
