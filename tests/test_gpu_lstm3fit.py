"""Fitting the 192 -> 128 Bi-LSTM with everything behind it on the device (MI355X only, -m gpu): csrc/nrv_lstm3fit.h through the
nrv_fit_* entry points at depth NRV_FIT_LSTM3.  nanoreviser_amd/lstm3fit.py is the definition; tests/lstm3fit_cases.py holds the
cases, the two f32 restatements and the floors.  Every tolerance is sized from CPU restatements against the float64 definition.
  1. doors and refusals: the _lstm3 doors round-trip bytes; every refusal by name at each of the four depths and in flight;
     depth 8 accepted, 6, 7 and 9 refused; NRV_FIT_MAX_LSTM3_ROWS; a parameter count of another depth;
  2. gradient: every case through the unit doors and nrv_fit_grad, per tensor (23) and sum within cpu_bound(); counts exact;
     T = 1 gives gU3 and gU4 bytes of zero; the sigmoid cases and a batch of more than one scratch chunk (4130 rows) the same way;
  3. real windows: the set gathered from the short fixture reads is the same bytes from f32 and f16x2 mode, rows within the f32
     floor of the fp64 oracle's [BN(lstm2) | signal_x_out], nrv_fit_eval at the handle's own tensors within the same kind of
     bound of the fp64 oracle and equal to the f32 mode's nrv_predict* under the tie rule;
  4. one update = tailfit_cases.adam_f32 on nrv_fit_grad's vector, byte for byte; a three-batch epoch twice and under poison;
  5. a row holding inf: its batch is counted in nonfinite and the parameters keep their bytes;
  6. it learns from the shipped start, and the written model runs in a new handle.
The training command line does not offer this depth yet (Left out)."""
import ctypes as C
import math

import numpy as np
import pytest

import lstm3fit_cases as lc
import tailfit_cases as tc
from nanoreviser_amd import headfit as hf
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import lstm3fit as lf
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.engine import FIT_LSTM3, NrvError
from test_gpu_headfit import _all_rows, _args, _labels_for, _pack
from test_gpu_lstm4fit import _row_bound

pytestmark = pytest.mark.gpu

PATTERNS = {"qnan": 0x7FC00000, "m1500": 0xC4BB8000}
ENV = ("NRV_PRECISION", "NRV_COALESCE", "NRV_LANES", "NRV_POISON", "NRV_FIT_MAX_ROWS", "NRV_FIT_MAX_HEAD_ROWS", "NRV_FIT_MAX_LSTM4_ROWS",
       "NRV_FIT_MAX_LSTM3_ROWS")
IDS = lambda c: "T%d-m%d-n%d-%s-act%d" % c      # noqa: E731
CHUNK_CASE = lc.CHUNK_CASE                      # 130 tiles: one scratch chunk of 128 and a second of two, the last tile short
FITTED = list(range(34, 40)) + list(range(44, 60))
FROZEN = list(range(0, 34)) + list(range(40, 44))
U_TENSORS = ("U3f", "U3b", "U4f", "U4b")


def _engine(monkeypatch, m1, m2, poison=None, **kw):
    from nanoreviser_amd.engine import Reviser
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if poison is not None:
        monkeypatch.setenv("NRV_POISON", f"{PATTERNS[poison]:08x}")
    rv = Reviser(m1, m2, **kw)
    monkeypatch.delenv("NRV_POISON", raising=False)
    rv.fit_set_depth("lstm3")
    assert rv.fit_depth() == FIT_LSTM3 == 8
    assert rv.fit_n_params(0) == lf.n_params(rv.T, 6) and rv.fit_n_params(1) == lf.n_params(rv.T, 5)
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
    """One lstm3-depth handle per (window length, recurrent_act), made on first use and shared.  Their BatchNorm between lstm3
    and lstm4 is the shipped ecoli one, as lstm3fit_cases.bn is."""
    from nanoreviser_amd.engine import Reviser
    made = {}

    def get(T, act=0):
        if (T, act) not in made:
            m1, m2 = species_models["ecoli"]
            made[T, act] = Reviser(m1.with_window(T), m2.with_window(T), recurrent_activation="sigmoid" if act else "hard_sigmoid")
            made[T, act].fit_set_depth("lstm3")
        return made[T, act]
    yield get
    for rv in made.values():
        rv.close()


def _set_case(rv, case):
    T, model, n, kind, act = case
    X, y, th = lc.rows_case(*case)
    other = np.minimum(y, 4)
    rv.fit_set_rows_lstm3(X, X, y if model == 0 else other, other if model == 0 else y)
    assert rv.fit_count() == n
    return X, y, th


@pytest.fixture(scope="module")
def grade_bound():
    K, worst = lc.cpu_bound()
    print(f"lstm3 depth: gradient bound sized on the CPU: K = {K:.3g} (worst restatement grade {worst:.3g})")
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
    x1, x2 = (rng.normal(0, 1, (n, 11, 192)).astype(np.float32) for _ in range(2))
    xb = rng.normal(0, 1, (n, 11, 256)).astype(np.float32)
    x4 = xb[:, :, :128].copy()
    F = rng.uniform(0, 1, (n, 66)).astype(np.float32)
    y1, y2 = rng.integers(0, 6, n).astype(np.uint8), rng.integers(0, 5, n).astype(np.uint8)
    none4 = (None, None, None, None)
    # tail depth: the _lstm3 doors are refused under their own names
    assert rv.fit_depth() == 0
    with pytest.raises(NrvError, match="nrv_fit_set_rows_lstm3: the set is at tail depth"):
        rv.fit_set_rows_lstm3(x1, x2, y1, y2)
    refused(lib.nrv_fit_get_rows_lstm3(h, 0, 0, *none4), "nrv_fit_get_rows_lstm3", "tail depth")
    for bad in (2, 3, 5, 6, 7, 9, -1):
        refused(lib.nrv_fit_set_depth(h, bad), "nrv_fit_set_depth", "NRV_FIT_TAIL or NRV_FIT_HEAD")
        assert "NRV_FIT_LSTM4" in lib.nrv_last_error(h).decode() and "NRV_FIT_LSTM3" in lib.nrv_last_error(h).decode()
    # head depth and lstm4 depth: the same
    rv.fit_set_depth("head")
    with pytest.raises(NrvError, match="nrv_fit_set_rows_lstm3: the set is at head depth"):
        rv.fit_set_rows_lstm3(x1, x2, y1, y2)
    refused(lib.nrv_fit_get_rows_lstm3(h, 0, 0, *none4), "nrv_fit_get_rows_lstm3", "head depth")
    rv.fit_set_depth("lstm4")
    with pytest.raises(NrvError, match="nrv_fit_set_rows_lstm3: the set is at lstm4 depth"):
        rv.fit_set_rows_lstm3(x1, x2, y1, y2)
    refused(lib.nrv_fit_get_rows_lstm3(h, 0, 0, *none4), "nrv_fit_get_rows_lstm3", "lstm4 depth")
    # lstm3 depth: depth 8 is accepted on the empty set; the other three depths' doors are refused
    assert lib.nrv_fit_set_depth(h, 8) == 0 and rv.fit_depth() == 8 and rv.fit_count() == 0
    with pytest.raises(NrvError, match="nrv_fit_set_rows: the set is at lstm3 depth"):
        rv.fit_set_rows(F, F, y1, y2)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_head: the set is at lstm3 depth"):
        rv.fit_set_rows_head(x4, x4, y1, y2)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_lstm4: the set is at lstm3 depth"):
        rv.fit_set_rows_lstm4(xb, xb, y1, y2)
    refused(lib.nrv_fit_get_rows(h, 0, 0, *none4), "nrv_fit_get_rows", "lstm3 depth")
    refused(lib.nrv_fit_get_rows_head(h, 0, 0, *none4), "nrv_fit_get_rows_head", "lstm3 depth")
    refused(lib.nrv_fit_get_rows_lstm4(h, 0, 0, *none4), "nrv_fit_get_rows_lstm4", "lstm3 depth")
    refused(lib.nrv_fit_set_rows_lstm3(h, None, None, None, None, 4), "nrv_fit_set_rows_lstm3", "null rows")
    with pytest.raises(NrvError, match="nrv_fit_set_rows_lstm3: a label outside"):
        rv.fit_set_rows_lstm3(x1, x2, np.full(n, 6, np.uint8), y2)
    refused(lib.nrv_fit_params(h, 0, None, None), "nrv_fit_params", "nrv_fit_begin")          # the depth change forgot any begin
    # the doors round-trip bytes, sub-ranges too
    rv.fit_set_rows_lstm3(x1, x2, y1, y2)
    assert rv.fit_count() == n
    got = rv.fit_get_rows_lstm3()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, (x1, x2, y1, y2)))
    for first, count in ((0, 1), (31, 33), (76, 1), (77, 0)):
        sub = rv.fit_get_rows_lstm3(first, count)
        assert all(a.tobytes() == b[first:first + count].tobytes() for a, b in zip(sub, (x1, x2, y1, y2))), (first, count)
    with pytest.raises(NrvError, match="nrv_fit_get_rows_lstm3: rows outside the training set"):
        rv.fit_get_rows_lstm3(70, 8)
    with pytest.raises(ValueError):
        rv.fit_set_rows_lstm3(xb, xb, y1, y2)
    for d in (0, 1, 4):
        refused(lib.nrv_fit_set_depth(h, d), "nrv_fit_set_depth", "not empty")
    # a parameter count of another depth is refused
    for other in (tf.n_params(11, 6), hf.n_params(11, 6), l4.n_params(11, 6)):
        with pytest.raises(ValueError, match=f"expected {lf.n_params(11, 6)} parameters, got {other}"):
            rv.fit_begin(0, np.zeros(other, np.float32))
    rv.fit_begin(0)
    rows = np.arange(33, dtype=np.uint32)
    want_g, want_st = rv.fit_grad(0, rows)
    assert want_g.size == lf.n_params(11, 6) == 328704 + 164352 + 20838 + tf.n_params(11, 6)
    refused(lib.nrv_fit_grad(h, 0, rows.ctypes.data_as(C.POINTER(C.c_uint32)), 0, want_g.ctypes.data_as(C.POINTER(C.c_float)), None),
            "nrv_fit_grad", "b outside")
    # in flight: the depth cannot change and the doors are refused under their own names
    t = rv.begin_packed_raw(_pack(rv, short_reads[:1]))
    refused(lib.nrv_fit_set_depth(h, 0), "nrv_fit_set_depth", "in flight")
    refused(lib.nrv_fit_set_rows_lstm3(h, None, None, None, None, 0), "nrv_fit_set_rows_lstm3", "in flight")
    refused(lib.nrv_fit_get_rows_lstm3(h, 0, 0, *none4), "nrv_fit_get_rows_lstm3", "in flight")
    assert lib.nrv_fit_depth(h) == 8
    rv.end_packed_raw(t)
    g3, st3 = rv.fit_grad(0, rows)
    assert g3.tobytes() == want_g.tobytes() and st3 == want_st and rv.fit_count() == n          # the handle stayed usable
    rv.close()
    # a handle under NRV_FIT_MAX_LSTM3_ROWS = 1000 refuses an adding call whole, by that name, and stays usable
    monkeypatch.setenv("NRV_FIT_MAX_LSTM3_ROWS", "1000")
    rv = Reviser(*species_models["ecoli"])
    monkeypatch.delenv("NRV_FIT_MAX_LSTM3_ROWS")
    rv.fit_set_depth("lstm3")
    labels = _labels_for(short_reads)
    with pytest.raises(NrvError) as e:
        rv.fit_add_packed(_pack(rv, short_reads), labels)
    assert e.value.code == -1 and "nrv_fit_add_reads_raw: the call would pass the row cap" in str(e.value) and "NRV_FIT_MAX_LSTM3_ROWS" in str(e.value)
    assert rv.fit_count() == 0
    z = np.zeros((1001, 11, 192), np.float32)
    with pytest.raises(NrvError, match="NRV_FIT_MAX_LSTM3_ROWS"):
        rv.fit_set_rows_lstm3(z, z, np.zeros(1001, np.uint8), np.zeros(1001, np.uint8))
    n0 = len(short_reads[0].starts)
    lab = labels[:n0].copy()
    lab[400:] = 0xFF
    assert 0 < rv.fit_add_packed(_pack(rv, short_reads[:1]), lab) == rv.fit_count() <= 1000
    rv.fit_reset()
    rv.fit_set_depth("lstm4")                              # the lstm4 depth's cap is its own
    assert rv.fit_add_packed(_pack(rv, short_reads), labels) > 1000
    rv.close()


# ---- 2. the gradient -------------------------------------------------------------------------------------------------------
def _check_gradient(rv, case, grade_bound):
    T, model, n, kind, act = case
    C_ = lc.n_class(model)
    X, y, th = _set_case(rv, case)
    sc, sh = lc.bn(model)
    rv.fit_begin(model, th)
    g, st = rv.fit_grad(model, np.arange(n))
    ref = lc.grad_reference(*case)
    grades = lc.device_grades(g, st.ce_sum, st.center_sum, ref, T, C_)
    print(case, {k: round(v, 3) for k, v in grades.items()}, "bound", round(grade_bound, 3))
    assert g.size == lf.n_params(T, C_) and np.isfinite(g).all() and len(grades) == 25
    assert max(grades.values()) <= grade_bound, grades
    s64 = ref["st64"]
    assert (st.rows, st.correct, st.steps, st.nonfinite) == (n, s64.correct, 0, 0)
    assert rv.fit_params(model)[0].tobytes() == th.tobytes() and rv.fit_params(model)[1] == 0     # nothing was updated
    g1, st1 = rv.fit_grad(model, np.arange(n))
    assert g1.tobytes() == g.tobytes() and st1 == st                                           # the same call, the same bytes
    sp = lc.spans(T, C_)
    for k in U_TENSORS:
        if T == 1:                                         # no step has a step before it: gU is exactly zero
            assert g[sp[k]].tobytes() == bytes(4 * (sp[k].stop - sp[k].start)), k
        else:
            assert g[sp[k]].any(), k
    # forward only: p is the definition's within f32, the same counts and sums as the gradient call's
    p, se = rv.fit_eval(model, np.arange(n))
    p64 = lf.forward(X, th, sc, sh, T, C_, act, np.float64)[5]
    print(case, "nrv_fit_eval: max |p - p64| =", float(np.abs(p - p64).max()), "bound", 64 * tc.EPS32)
    assert np.abs(p - p64).max() <= 64 * tc.EPS32
    assert (se.rows, se.correct, se.ce_sum, se.center_sum) == (n, st.correct, st.ce_sum, st.center_sum)


@pytest.mark.parametrize("case", lc.HARD_CASES, ids=IDS)
def test_gradient_against_the_definition(handles, grade_bound, case):
    _check_gradient(handles(case[0], 0), case, grade_bound)


@pytest.mark.parametrize("case", lc.SIGMOID_CASES, ids=IDS)
def test_gradient_with_the_sigmoid_gates(handles, grade_bound, case):
    _check_gradient(handles(case[0], 1), case, grade_bound)


def test_a_batch_of_more_than_one_scratch_chunk(handles, grade_bound):
    """No handle has a chunk setting, so the chunked batch is held to the definition as every other case is."""
    _check_gradient(handles(CHUNK_CASE[0], 1), CHUNK_CASE, grade_bound)


# ---- 3. real windows -------------------------------------------------------------------------------------------------------
def _xin_numpy(w, sig, rd, dtype):
    """[BN(lstm2) | signal_x_out] in front of lstm3 from oracle.nrv_oracle's own pieces."""
    from oracle import nrv_oracle as O
    dt = np.dtype(dtype)
    w = [np.asarray(t, dtype=dt) for t in w]
    rd = np.asarray(rd, np.float32).astype(dt)
    B, T, _ = rd.shape
    s = O.signal_branch(w, np.asarray(sig, np.float32).astype(dt).reshape(B * T, 50)).reshape(B, T, 64)
    act = O.hard_sigmoid
    r = O._bn(O.bilstm(rd, w[12:18], act), *w[18:22])
    r = O._bn(O.bilstm(r, w[22:28], act), *w[28:32])
    return np.concatenate([r, s], axis=-1)


def _xin_torch(tensors, sig, rd):
    """The same from oracle/torch_cpu.py's pieces at float32."""
    import torch
    import torch.nn.functional as F
    from oracle import torch_cpu as TC
    m = TC.TorchCpuModel(tensors)
    w = m.w
    with torch.no_grad():
        sg = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float32))
        x = torch.from_numpy(np.ascontiguousarray(rd, dtype=np.float32))
        B, T, _ = x.shape
        s = sg.reshape(B * T, 1, 50)
        y = F.conv1d(s, m.k1, w[1], padding=1)
        y = TC._bn(F.relu(y).permute(0, 2, 1), w[2], w[3], w[4], w[5])
        y = F.conv1d(y.permute(0, 2, 1), m.k2, w[7], padding=1)
        y = TC._bn(F.relu(y).permute(0, 2, 1), w[8], w[9], w[10], w[11])
        y = y + s.permute(0, 2, 1)
        sx = (y.reshape(B * T, 400) @ w[32] + w[33]).reshape(B, T, 64)
        r = TC._bn(TC._bilstm(x, w[12:18]), *w[18:22])
        r = TC._bn(TC._bilstm(r, w[22:28]), *w[28:32])
        return torch.cat([r, sx], dim=-1).numpy()


def test_real_windows_gather_and_forward(species_models, short_reads, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    from oracle import nrv_oracle as O
    from oracle import torch_cpu as TC
    m1, m2 = species_models["ecoli"]
    labels = _labels_for(short_reads)
    w, y1, y2 = tf.labelled_windows(labels, [len(r.starts) for r in short_reads], 11)
    sets = {}
    for mode in ("f32", "f16x2"):
        rv = _engine(monkeypatch, m1, m2, precision=mode)
        assert rv.fit_add_packed(_pack(rv, short_reads), labels) == rv.fit_count() == w.size > 1000
        assert rv.precision == mode
        sets[mode] = rv.fit_get_rows_lstm3()
        if mode == "f16x2":
            ps = []
            for k in (0, 1):
                rv.fit_begin(k)                            # the handle's own tensors 34 .. 39 and 44 .. 59
                p, st = rv.fit_eval(k, _all_rows(rv))
                assert st.rows == w.size and st.steps == 0 and st.nonfinite == 0
                ps.append(p)
                th, _ = rv.fit_params(k)
                assert th.tobytes() == lf.params_from_model((m1, m2)[k]).tobytes()               # unfolded, as the file has them
        rv.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(sets["f32"], sets["f16x2"]))
    xin = sets["f32"][:2]
    assert np.array_equal(sets["f32"][2], y1) and np.array_equal(sets["f32"][3], y2) and xin[0].shape == (w.size, 11, 192)
    rp = Reviser(m1, m2, precision="f32")
    pred = rp.predict_reads_raw(*_args(short_reads))
    rp.close()
    sig_ev = np.concatenate([hs.segment_windows_f32(r.raw, r.starts, r.shift, r.scale) for r in short_reads])
    feat_ev = np.concatenate([r.feat_ev for r in short_reads])
    pick = np.linspace(0, w.size - 1, 128).astype(np.int64)
    idx = w[pick][:, None] + np.arange(11)[None, :]
    sig, rd = sig_ev[idx], feat_ev[idx]
    q64 = O.predict_pair(m1.tensors, m2.tensors, sig, rd, np.float64)
    q32 = O.predict_pair(m1.tensors, m2.tensors, sig, rd, np.float32)
    qt = TC.predict_pair(TC.TorchCpuModel(m1.tensors), TC.TorchCpuModel(m2.tensors), sig.astype(np.float32), rd.astype(np.float32))
    for k, m in enumerate((m1, m2)):
        with np.errstate(over="ignore"):
            f64 = _xin_numpy(m.tensors, sig, rd, np.float64).reshape(128, -1)
            d_np = np.abs(_xin_numpy(m.tensors, sig, rd, np.float32).reshape(128, -1) - f64).max(-1)
        d_t = np.abs(_xin_torch(m.tensors, sig, rd).reshape(128, -1) - f64).max(-1)
        scale = np.abs(f64).max(-1)
        K = _row_bound(d_np, d_t, scale)
        d_dev = np.abs(xin[k][pick].reshape(128, -1).astype(np.float64) - f64).max(-1)
        grades = [tc.grade_of(d, max(a, b), s) for d, a, b, s in zip(d_dev, d_np, d_t, scale)]
        print(f"model{k + 1}: gathered Xin rows, worst grade {max(grades):.3g} (bound {K:.3g})")
        assert max(grades) <= K, (k, max(grades), K)
        # nrv_fit_eval at the handle's own tensors and the f32 mode's nrv_predict*: both within the bound, equal under the tie rule
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
@pytest.mark.parametrize("case", [(11, 1, 33, "plain", 0), (1, 0, 33, "plain", 0), lc.GRAD_CASES[-1]], ids=IDS)
def test_one_step_is_numpy_f32_adam_bit_for_bit(handles, case):
    T, model, n, kind, act = case
    rv = handles(T, act)
    X, y, th = _set_case(rv, case)
    opts = tf.default_opts(model)
    rv.fit_begin(model, th, opts)
    g, _ = rv.fit_grad(model, np.arange(n))
    st = rv.fit_epoch(model, np.arange(n))
    got, t = rv.fit_params(model)
    want = tc.adam_f32(th, np.zeros_like(th), np.zeros_like(th), g, opts, 1)[0]
    assert (t, st.steps, st.rows, st.nonfinite) == (1, 1, n, 0)
    assert got.size == lf.n_params(T, 6 - model) and got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8].tolist()
    sp = lc.spans(T, 6 - model)
    moved = {k: not np.array_equal(got[sp[k]], th[sp[k]]) for k in lc.TENSORS}
    assert all(v for k, v in moved.items() if not (T == 1 and k in U_TENSORS)), moved


EPOCH_CASE = (11, 0, 1100, "plain", 0)


def _epoch(rv, th, order, opts):
    rv.fit_begin(0, th, opts)
    st = rv.fit_epoch(0, order)
    return rv.fit_params(0)[0], st


def test_epoch_twice_and_poisoned_give_the_same_bytes(species_models, handles, monkeypatch):
    T, model, n, _, _ = EPOCH_CASE
    rv = handles(T)
    X, y, th = _set_case(rv, EPOCH_CASE)
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
    X, y, th = lc.rows_case(*EPOCH_CASE)
    X = X.copy()
    X[600, 3, 7] = np.inf                                  # the second batch of 512
    rv.fit_set_rows_lstm3(X, X, y, np.minimum(y, 4))
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


def test_it_learns_from_the_shipped_start_and_the_written_model_runs(species_models, short_reads, monkeypatch, tmp_path):
    """Adapting the shipped ecoli model to another teacher: every window of the two shortest fixture reads, labelled with the
    answers the shipped HUMAN model gives in f32 mode, LEARN_E epochs at the defaults from the ecoli handle's own tensors.
    Asserted: the last epoch's training loss is below the first's, the training accuracy ends above the majority-class rate,
    tensors 34 .. 39 and 44 .. 59 all moved while 0 .. 33 and the BatchNorm 40 .. 43 keep their bytes, and the written model,
    loaded by a new f32-mode handle, answers those windows with nrv_fit_eval's probabilities within the bound of test 3."""
    from nanoreviser_amd.engine import Reviser
    from nanoreviser_amd.weights import load_model
    m1, m2 = species_models["ecoli"]
    el = [len(r.starts) for r in short_reads]
    labels = np.full(sum(el), 5, np.uint8)                 # every window of either read is labelled ...
    w = tf.labelled_windows(labels, el, 11)[0]
    teacher = Reviser(*species_models["human"], precision="f32")
    _, _, a1, a2 = teacher.predict_reads_raw(*_args(short_reads))
    teacher.close()
    y1, y2 = a1[w].astype(np.uint8), a2[w].astype(np.uint8)
    rv = _engine(monkeypatch, m1, m2)
    n = rv.fit_add_packed(_pack(rv, short_reads), labels)
    assert n == w.size == sum(el) - 22
    x1, x2, _, _ = rv.fit_get_rows_lstm3()
    rv.fit_set_rows_lstm3(x1, x2, y1, y2)                  # ... with the teacher's answers
    backs, finals = [], []
    for k, (m, y) in enumerate(((m1, y1), (m2, y2))):
        C_ = 6 - k
        majority = np.bincount(y, minlength=C_).max() / n
        rv.fit_begin(k, None, tf.default_opts(k))
        hist = [rv.fit_epoch(k, tf.epoch_order(n, 3, ep)) for ep in range(LEARN_E)]
        loss = [h.loss()[0] for h in hist]
        print(f"model{k + 1}: majority {majority:.4f}, loss {loss[0]:.4f} -> {loss[-1]:.4f}, acc {hist[0].acc():.4f} -> {hist[-1].acc():.4f}")
        assert all(h.nonfinite == 0 for h in hist) and loss[-1] < loss[0]
        assert hist[-1].acc() > majority, (k, hist[-1].acc(), majority)
        theta, t = rv.fit_params(k)
        fm = lf.fitted_model(m, theta)
        assert all(fm.tensors[i].tobytes() == m.tensors[i].tobytes() for i in FROZEN)
        assert all(not np.array_equal(fm.tensors[i], m.tensors[i]) for i in FITTED)               # all twenty-two were fitted
        tf.write_f32(fm, str(tmp_path / f"m{k}"))
        backs.append(load_model(str(tmp_path / f"m{k}.f32")))
        finals.append(rv.fit_eval(k, _all_rows(rv))[0])
    rv.close()
    rv2 = Reviser(backs[0], backs[1], precision="f32")
    pred = rv2.predict_reads_raw(*_args(short_reads))
    rv2.close()
    # the bound, sized on the CPU on the fitted tensors: the oracle at float32 and torch_cpu against the oracle at float64
    from oracle import nrv_oracle as O
    from oracle import torch_cpu as TC
    sig_ev = np.concatenate([hs.segment_windows_f32(r.raw, r.starts, r.shift, r.scale) for r in short_reads])
    feat_ev = np.concatenate([r.feat_ev for r in short_reads])
    pick = np.linspace(0, w.size - 1, 128).astype(np.int64)
    idx = w[pick][:, None] + np.arange(11)[None, :]
    sig, rd = sig_ev[idx], feat_ev[idx]
    t1, t2 = backs[0].tensors, backs[1].tensors
    q64 = O.predict_pair(t1, t2, sig, rd, np.float64)
    q32 = O.predict_pair(t1, t2, sig, rd, np.float32)
    qt = TC.predict_pair(TC.TorchCpuModel(t1), TC.TorchCpuModel(t2), sig.astype(np.float32), rd.astype(np.float32))
    for k in (0, 1):
        e_np, e_t = np.abs(q32[k] - q64[k]).max(-1), np.abs(qt[k] - q64[k]).max(-1)
        Kp = _row_bound(e_np, e_t, np.ones(128))
        for name, p in (("nrv_fit_eval", finals[k][pick]), ("the written model", pred[k][w][pick])):
            gr = [tc.grade_of(d, max(a, b), 1.0) for d, a, b in zip(np.abs(p - q64[k]).max(-1), e_np, e_t)]
            print(f"model{k + 1}: {name} p, worst grade {max(gr):.3g} (bound {Kp:.3g})")
            assert max(gr) <= Kp, (k, name, max(gr), Kp)
