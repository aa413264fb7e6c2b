"""Fitting the per-window tail on the device (MI355X only, -m gpu): csrc/nrv_tailfit.h through the nrv_fit_* entry points.
nanoreviser_amd/tailfit.py is the definition; tests/tailfit_cases.py holds the cases, the two f32 restatements and the floors.
  1. gather, bit for bit: nrv_fit_add_reads_raw on the two shortest fixture reads in one call, seeded label bytes with 0xFF;
     the count and y1 / y2 are the definition's labelled windows in window order, and nrv_fit_eval's p over all rows equals the
     labelled rows of nrv_predict_reads_raw's p1 / p2 of an f32-mode handle; the same from a handle in f16x2 or bf16x3 mode, and
     with the reads split over two adding calls;
  2. gather against fp64: nrv_fit_get_rows against main_out recomputed here from the oracle's own pieces in float64, held to
     the f32 floor (the NumPy-f32 evaluation of the same pieces) with precision_cases' f32-mode bounds;
  3. gradient: nrv_fit_grad against the float64 definition per tensor in units of the floor both f32 restatements form; the
     bound is sized at run time on the CPU alone (tailfit_cases.cpu_bound); rows, correct, steps, nonfinite exact;
  4. Adam, bit for bit: one epoch of a single batch = NumPy-f32 Adam on the gradient nrv_fit_grad returned;
  5. epoch, bit for bit: 1100 rows at B = 512 against the host loop of nrv_fit_grad + NumPy-f32 Adam; two runs, the same bytes;
  6. a NaN row: its batch is skipped and counted, the others update;
  7. it learns: labels = the handle's own answers, a fresh tail, loss falls and accuracy beats the majority class;
  8. handles created under NRV_POISON: 1 and 5 unchanged;
  9. refusals by name, the handle usable afterwards;
 10. the command line: --labels, NanoReviser_train.py -w 13, NanoReviser.py --score on the written model directory."""
import ctypes as C
import glob
import math
import os
import shutil

import numpy as np
import pytest

import tailfit_cases as tc
from conftest import GOLD
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.engine import NrvError
from score_cases import VALID

pytestmark = pytest.mark.gpu

PATTERNS = {"qnan": 0x7FC00000, "m1500": 0xC4BB8000}


def _engine(monkeypatch, m1, m2, poison=None, **kw):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_PRECISION", "NRV_COALESCE", "NRV_LANES", "NRV_POISON", "NRV_FIT_MAX_ROWS"):
        monkeypatch.delenv(k, raising=False)
    if poison is not None:
        monkeypatch.setenv("NRV_POISON", f"{PATTERNS[poison]:08x}")
    rv = Reviser(m1, m2, **kw)
    monkeypatch.delenv("NRV_POISON", raising=False)
    return rv


@pytest.fixture(scope="module")
def short_reads(reads):
    out = []
    for k in reads.keys:
        _, rd, _ = reads(k)
        out.append(hs.read_tensors_raw(rd))
    return sorted(out, key=lambda r: len(r.starts))[:2]


def _labels_for(rrs, seed=91):
    """Seeded random valid bytes, one per event, with 0xFF clips at both ends of every read, a run inside and bytes whose code
    is 0, 6 or 7 (tests/test_gpu_device_score.py makes them this way)."""
    rng = np.random.default_rng(seed)
    parts = []
    for r in rrs:
        n = len(r.starts)
        lab = np.array(VALID, np.uint8)[rng.integers(0, 20, n)]
        lab[:int(rng.integers(8, 40))] = 0xFF
        lab[n - int(rng.integers(8, 40)):] = 0xFF
        lab[n // 2:n // 2 + 25] = 0xFF
        lab[n // 3:n // 3 + 4] = [0x00, 0x06, 0x0F, 0xE3]
        parts.append(lab)
    return np.concatenate(parts)


def _args(rrs):
    return ([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs], [r.shift for r in rrs], [r.scale for r in rrs])


def _pack(rv, rrs):
    return rv.pack_reads_raw(*_args(rrs), rv.T)


@pytest.fixture(scope="module")
def f32_calls(species_models, short_reads):
    """Computed once: the f32-mode handle's own answers on the two reads, the labels and the definition's labelled windows."""
    from nanoreviser_amd.engine import Reviser
    rv = Reviser(*species_models["ecoli"], precision="f32")
    p1, p2, a1, a2 = rv.predict_reads_raw(*_args(short_reads))
    rv.close()
    labels = _labels_for(short_reads)
    w, y1, y2 = tf.labelled_windows(labels, [len(r.starts) for r in short_reads], 11)
    return {"p": (p1, p2), "a": (a1, a2), "labels": labels, "w": w, "y": (y1, y2)}


def _all_rows(rv):
    return np.arange(rv.fit_count(), dtype=np.uint32)


def _gathered(rv, rrs, c, split=False):
    """The set after adding the two reads (in one call, or one call each) -> (flat1, flat2, p1 rows, p2 rows)."""
    rv.fit_reset()
    assert rv.fit_count() == 0
    if split:
        n0 = len(rrs[0].starts)
        added = rv.fit_add_packed(_pack(rv, rrs[:1]), c["labels"][:n0]) + rv.fit_add_packed(_pack(rv, rrs[1:]), c["labels"][n0:])
    else:
        added = rv.fit_add_packed(_pack(rv, rrs), c["labels"])
    assert added == rv.fit_count() == c["w"].size > 1000
    f1, f2, y1, y2 = rv.fit_get_rows()
    assert np.array_equal(y1, c["y"][0]) and np.array_equal(y2, c["y"][1])
    ps = []
    for k in (0, 1):
        rv.fit_begin(k)                                    # the handle's own tail: the model nrv_predict* runs
        p, st = rv.fit_eval(k, _all_rows(rv))
        assert st.rows == added and st.steps == 0 and st.nonfinite == 0
        assert st.correct == int((c["a"][k][c["w"]] == c["y"][k]).sum())
        ps.append(p)
    return f1, f2, ps[0], ps[1]


def _check_gather(rv, rrs, c, what):
    got = _gathered(rv, rrs, c)
    for k in (0, 1):
        want = c["p"][k][c["w"]]
        assert got[2 + k].dtype == np.float32 and got[2 + k].tobytes() == want.tobytes(), (what, k, np.argwhere(got[2 + k] != want)[:4].tolist())
    return got


# ---- 1. gather, bit for bit ----------------------------------------------------------------------------------------------
def test_gather_is_the_f32_modes_rows_bit_for_bit(species_models, short_reads, f32_calls, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    assert rv.precision == "f16x2"
    ref = None
    for mode in ("f32", "f16x2", "bf16x3"):
        rv.set_precision(mode)
        got = _check_gather(rv, short_reads, f32_calls, mode)
        assert rv.precision == mode                        # the adding call selected the f32 kernels for itself alone
        ref = ref or got
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)), mode
        two = _gathered(rv, short_reads, f32_calls, split=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(two, ref)), (mode, "two adding calls")
    # a labelled window's row is not another window's: rows differ from their neighbours
    assert not np.array_equal(ref[0][0], ref[0][1]) and not np.array_equal(ref[0], ref[1])
    # N <= T adds nothing; a predict on the same handle afterwards returns its usual bytes
    r0 = short_reads[0]
    p = rv.pack_reads_raw([r0.raw], [r0.starts[:11]], [r0.feat_ev[:11]], [r0.shift], [r0.scale], rv.T)
    assert rv.fit_add_packed(p, np.full(11, 5, np.uint8)) == 0 and rv.fit_count() == f32_calls["w"].size
    rv.set_precision("f32")
    again = rv.predict_reads_raw(*_args(short_reads))
    assert again[0].tobytes() == f32_calls["p"][0].tobytes() and again[1].tobytes() == f32_calls["p"][1].tobytes()
    rv.close()


def test_row_cap_refuses_the_call_whole(species_models, short_reads, f32_calls, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    monkeypatch.setenv("NRV_FIT_MAX_ROWS", str(f32_calls["w"].size - 1))
    rv = Reviser(*species_models["ecoli"])
    monkeypatch.delenv("NRV_FIT_MAX_ROWS")
    with pytest.raises(NrvError) as e:
        rv.fit_add_packed(_pack(rv, short_reads), f32_calls["labels"])
    assert e.value.code == -1 and "nrv_fit_add_reads_raw: the call would pass the row cap" in str(e.value)
    assert rv.fit_count() == 0
    n0 = len(short_reads[0].starts)
    assert rv.fit_add_packed(_pack(rv, short_reads[:1]), f32_calls["labels"][:n0]) == rv.fit_count() > 0
    rv.close()


# ---- 2. gather against fp64 ----------------------------------------------------------------------------------------------
def _main_out(w, sig, rd, dtype):
    """Flatten(main_out) of these windows from oracle.nrv_oracle's own pieces (its `forward` up to line 131)."""
    from oracle import nrv_oracle as O
    dt = np.dtype(dtype)
    w = [np.asarray(t, dtype=dt) for t in w]
    rd = np.asarray(rd, np.float32).astype(dt)
    B, T, _ = rd.shape
    s = O.signal_branch(w, np.asarray(sig, np.float32).astype(dt).reshape(B * T, 50)).reshape(B, T, 64)
    act = O.hard_sigmoid
    r = O._bn(O.bilstm(rd, w[12:18], act), *w[18:22])
    r = O._bn(O.bilstm(r, w[22:28], act), *w[28:32])
    x = np.concatenate([r, s], axis=-1)
    x = O._bn(O.bilstm(x, w[34:40], act), *w[40:44])
    x = O.bilstm(x, w[44:50], act)
    x = np.maximum(x @ w[50] + w[51], 0)
    x = np.maximum(x @ w[52] + w[53], 0)
    x = np.maximum(x @ w[54] + w[55], 0)
    return x.reshape(B, T * 6)


def test_gathered_rows_against_fp64(species_models, short_reads, f32_calls, monkeypatch):
    from oracle import nrv_oracle as O
    import precision_cases as pc
    rv = _engine(monkeypatch, *species_models["ecoli"])
    f1, f2 = _gathered(rv, short_reads, f32_calls)[:2]
    rv.close()
    sig_ev = np.concatenate([hs.segment_windows_f32(r.raw, r.starts, r.shift, r.scale) for r in short_reads])
    feat_ev = np.concatenate([r.feat_ev for r in short_reads])
    pick = np.linspace(0, f32_calls["w"].size - 1, 256).astype(np.int64)      # 256 labelled rows across both reads
    idx = f32_calls["w"][pick][:, None] + np.arange(11)[None, :]
    sig, rd = sig_ev[idx], feat_ev[idx]
    for k, (m, flat) in enumerate(zip(species_models["ecoli"], (f1, f2))):
        with np.errstate(over="ignore"):
            f64, f32 = _main_out(m.tensors, sig, rd, np.float64), _main_out(m.tensors, sig, rd, np.float32)
        floor = np.abs(f32 - f64).max(-1)
        r = np.abs(flat[pick].astype(np.float64) - f64).max(-1) / np.maximum(floor, np.median(floor))
        K = pc.K_for(pc.key("fixture", "ecoli", k + 1, "hard_sigmoid"), "f32")
        print(f"model{k + 1}: gathered rows over the f32 floor: median {np.median(r):.3g} (bound {K['med_r']}), "
              f"q90 {np.quantile(r, 0.9):.3g} (bound {K['q90_r']})")
        assert np.median(r) <= K["med_r"] and np.quantile(r, 0.9) <= K["q90_r"], (k, float(np.median(r)), float(np.quantile(r, 0.9)))


# ---- 3 .. 6. the step on host-supplied rows ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles(species_models):
    """One handle per window length, made on first use and shared by the tests below (nrv_fit_set_rows replaces the set)."""
    from nanoreviser_amd.engine import Reviser
    made = {}

    def get(T):
        if T not in made:
            m1, m2 = species_models["ecoli"]
            made[T] = Reviser(m1.with_window(T), m2.with_window(T))
        return made[T]
    yield get
    for rv in made.values():
        rv.close()


def _set_case(rv, case):
    T, model, n, kind = case
    F, y, th = tc.rows_case(*case)
    other = np.minimum(y, 4)                               # the other model's labels only have to be valid
    rv.fit_set_rows(F, F, y if model == 0 else other, other if model == 0 else y)
    assert rv.fit_count() == n
    return F, y, th


@pytest.fixture(scope="module")
def grade_bound():
    K, worst = tc.cpu_bound()
    print(f"gradient bound sized on the CPU: K = {K:.3g} (worst restatement grade {worst:.3g})")
    return K


@pytest.mark.parametrize("case", tc.GRAD_CASES, ids=lambda c: "T%d-m%d-n%d-%s" % c)
def test_gradient_against_the_definition(handles, grade_bound, case):
    T, model, n, kind = case
    C = tc.n_class(model)
    rv = handles(T)
    F, y, th = _set_case(rv, case)
    f1, f2, y1, y2 = rv.fit_get_rows()
    assert f1.tobytes() == F.tobytes() and f2.tobytes() == F.tobytes() and np.array_equal((y1, y2)[model], y)
    rv.fit_begin(model, th)
    g, st = rv.fit_grad(model, np.arange(n))
    ref = tc.grad_reference(*case)
    grades = tc.device_grades(g, st.ce_sum, st.center_sum, ref, T, C)
    print(case, {k: round(v, 3) for k, v in grades.items()}, "bound", round(grade_bound, 3))
    assert np.isfinite(g).all() and max(grades.values()) <= grade_bound, grades
    s64 = ref["st64"]
    assert (st.rows, st.correct, st.steps, st.nonfinite) == (n, s64.correct, 0, 0)
    assert rv.fit_params(model)[0].tobytes() == th.tobytes() and rv.fit_params(model)[1] == 0     # nothing was updated
    # a permutation of the rows is the same batch: the same statistics, the gradient within the same bound
    perm = np.random.default_rng(n).permutation(n)
    g2, st2 = rv.fit_grad(model, perm)
    assert st2.correct == st.correct and max(tc.device_grades(g2, st2.ce_sum, st2.center_sum, ref, T, C).values()) <= grade_bound
    # forward only: p is the definition's within f32, the same counts
    p, se = rv.fit_eval(model, np.arange(n))
    p64 = tf.forward(F, th, T, C, np.float64)[1]
    assert np.abs(p - p64).max() <= 64 * tc.EPS32 and (se.rows, se.correct, se.ce_sum, se.center_sum) == (n, st.correct, st.ce_sum, st.center_sum)


@pytest.mark.parametrize("case", [(11, 0, 33, "plain"), (13, 1, 76, "plain"), (1, 1, 32, "absent"), (32, 0, 33, "zeros")],
                         ids=lambda c: "T%d-m%d-n%d-%s" % c)
def test_one_step_is_numpy_f32_adam_bit_for_bit(handles, case):
    T, model, n, kind = case
    rv = handles(T)
    F, y, th = _set_case(rv, case)
    opts = tf.default_opts(model)
    rv.fit_begin(model, th, opts)
    g, _ = rv.fit_grad(model, np.arange(n))
    st = rv.fit_epoch(model, np.arange(n))
    got, t = rv.fit_params(model)
    want = tc.adam_f32(th, np.zeros_like(th), np.zeros_like(th), g, opts, 1)[0]
    assert (t, st.steps, st.rows, st.nonfinite) == (1, 1, n, 0)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8].tolist()
    assert not np.array_equal(got, th)
    rv.fit_begin(model, th)                                # opts NULL: the engine's defaults are the definition's
    rv.fit_epoch(model, np.arange(n))
    assert rv.fit_params(model)[0].tobytes() == want.tobytes()


def _epoch_and_loop(rv, model, F, y, th, order, opts):
    """(the parameters after nrv_fit_epoch, its stats and t; the same by the host loop of nrv_fit_grad + NumPy-f32 Adam)."""
    rv.fit_begin(model, th, opts)
    st = rv.fit_epoch(model, order)
    got, t = rv.fit_params(model)
    cur, m, v = th.copy(), np.zeros_like(th), np.zeros_like(th)
    for k, s in enumerate(range(0, order.size, opts.B), 1):
        rv.fit_begin(model, cur, opts)
        g, _ = rv.fit_grad(model, order[s:s + opts.B])
        cur, m, v = tc.adam_f32(cur, m, v, g, opts, k)
    return got, st, t, cur


def test_epoch_is_the_host_loop_bit_for_bit(handles):
    T, model, n = 11, 0, 1100
    rv = handles(T)
    case = (T, model, n, "plain")
    F, y, th = _set_case(rv, case)
    opts = tf.default_opts(model, B=512)                   # batches of 512, 512, 76
    order = np.random.default_rng(4).permutation(n).astype(np.uint32)
    got, st, t, want = _epoch_and_loop(rv, model, F, y, th, order, opts)
    assert (t, st.steps, st.rows, st.nonfinite) == (3, 3, n, 0)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8].tolist()
    rv.fit_begin(model, th, opts)
    st2 = rv.fit_epoch(model, order)
    assert rv.fit_params(model)[0].tobytes() == got.tobytes() and st2 == st         # two runs: the same bytes
    st3 = rv.fit_epoch(model, order)                       # a second epoch goes on from t = 3
    assert rv.fit_params(model)[1] == 6 and st3.steps == 3 and st3.ce_sum != st.ce_sum
    # the definition's epoch in f64 from the same start: the statistics agree to f32, the counts nearly (argmax ties aside)
    s = tf.FitState(th.astype(np.float64))
    d = tf.epoch(F, y, s, order, T, 6, opts, np.float64)
    assert abs(st.ce_sum - d.ce_sum) <= 1e-4 * d.ce_sum and abs(st.center_sum - d.center_sum) <= 1e-4 * d.center_sum
    assert np.abs(got - s.theta).max() <= 1e-4             # three steps of lr 1e-3: an f32 rounding cannot move a step by a tenth


def test_nonfinite_batch_is_skipped_and_counted(handles):
    T, model, n = 11, 1, 1100
    rv = handles(T)
    F, y, th = tc.rows_case(T, model, n)
    F = F.copy()
    F[600, 7] = np.nan                                     # the second batch of 512
    other = np.minimum(y, 4)
    rv.fit_set_rows(F, F, other, y)
    opts = tf.default_opts(model, B=512)
    rv.fit_begin(model, th, opts)
    order = np.arange(n, dtype=np.uint32)
    st = rv.fit_epoch(model, order)
    got, t = rv.fit_params(model)
    assert (t, st.steps, st.nonfinite, st.rows) == (2, 2, 1, 588) and np.isfinite(got).all()
    assert math.isfinite(st.ce_sum) and math.isfinite(st.center_sum)
    g, sg = rv.fit_grad(model, order[512:1024])
    assert sg.nonfinite == 1 and not np.isfinite(g).all()
    keep = np.concatenate([order[:512], order[1024:]])     # the same epoch without the batch: the same bytes, t included
    rv.fit_begin(model, th, tf.default_opts(model, B=512))
    st2 = rv.fit_epoch(model, keep)
    assert rv.fit_params(model)[0].tobytes() == got.tobytes() and rv.fit_params(model)[1] == 2 and st2.nonfinite == 0


# ---- 7. it learns --------------------------------------------------------------------------------------------------------
LEARN_E, LEARN_SEED = 8, 3


def test_a_fresh_tail_recovers_the_teacher(species_models, short_reads, f32_calls, monkeypatch):
    """Teacher recovery: every window of the two shortest fixture reads labelled with the f32-mode handle's own a1 / a2, the
    tail re-drawn fresh (seed LEARN_SEED), LEARN_E epochs at the defaults.  Only conditions are asserted: the last epoch's
    training loss is below the first's, and the training accuracy is above the majority-class rate of those labels.
    E and the seed were chosen on the CPU with tailfit.py on main_out rows from the oracle (NumPy f32) of the same reads,
    13 525 rows, labels = that tail's own argmax.  Figures of that run (not asserted here), f32 and f64 runs alike to four digits:
      model 1  majority 0.2618; loss 1.9086 -> 0.9597; accuracy 0.1811 -> 0.9732: clears the majority by 0.7113, f32 - f64 0.0000
      model 2  majority 0.2696; loss 1.6027 -> 0.9432; accuracy 0.2909 -> 0.9736: clears the majority by 0.7040, f32 - f64 0.0000
    Both runs clear the majority rate by far more than twice their own difference."""
    a1, a2 = f32_calls["a"]
    el = [len(r.starts) for r in short_reads]
    lab = np.full(sum(el), 5, np.uint8)                    # every window of either read is labelled ...
    w = tf.labelled_windows(lab, el, 11)[0]
    rv = _engine(monkeypatch, *species_models["ecoli"])
    n = rv.fit_add_packed(_pack(rv, short_reads), lab)
    assert n == w.size == sum(el) - 22
    f1, f2, _, _ = rv.fit_get_rows()
    y1, y2 = a1[w].astype(np.uint8), a2[w].astype(np.uint8)
    rv.fit_set_rows(f1, f2, y1, y2)                        # ... and the labels are the handle's own answers (one byte cannot
    for k, y in enumerate((y1, y2)):                       # say a1 and a2 where the two models disagree; the rows can)
        C = 6 - k
        majority = np.bincount(y, minlength=C).max() / n
        rv.fit_begin(k, tf.fresh_params(11, C, LEARN_SEED + k), tf.default_opts(k))
        hist = [rv.fit_epoch(k, tf.epoch_order(n, LEARN_SEED, ep)) for ep in range(LEARN_E)]
        loss = [h.loss()[0] for h in hist]
        print(f"model{k + 1}: majority {majority:.4f}, loss {loss[0]:.4f} -> {loss[-1]:.4f}, acc {hist[0].acc():.4f} -> {hist[-1].acc():.4f}")
        assert all(h.nonfinite == 0 for h in hist) and loss[-1] < loss[0]
        assert hist[-1].acc() > majority, (k, hist[-1].acc(), majority)
    rv.close()


# ---- 8. poison -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", sorted(PATTERNS))
def test_poisoned_handles_give_the_same_bytes(species_models, short_reads, f32_calls, handles, monkeypatch, poison):
    rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
    _check_gather(rv, short_reads, f32_calls, poison)
    case = (11, 0, 1100, "plain")
    F, y, th = _set_case(rv, case)
    opts = tf.default_opts(0, B=512)
    order = np.random.default_rng(4).permutation(1100).astype(np.uint32)
    got, st, t, want = _epoch_and_loop(rv, 0, F, y, th, order, opts)
    assert got.tobytes() == want.tobytes() and (t, st.steps) == (3, 3)
    clean = handles(11)
    _set_case(clean, case)
    clean.fit_begin(0, th, opts)
    assert clean.fit_epoch(0, order) == st and clean.fit_params(0)[0].tobytes() == got.tobytes()
    rv.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_handle_usable(species_models, short_reads, f32_calls, monkeypatch):
    from nanoreviser_amd.engine import _FitStats
    rv = _engine(monkeypatch, *species_models["ecoli"], precision="f32")
    lib, h = rv._lib, rv._h
    case = (11, 0, 33, "plain")
    F, y, th = _set_case(rv, case)
    rows = np.arange(33, dtype=np.uint32)
    rp = rows.ctypes.data_as(C.POINTER(C.c_uint32))
    g = np.zeros(rv.fit_n_params(0), np.float32)
    gp = g.ctypes.data_as(C.POINTER(C.c_float))
    st = _FitStats()
    n_added = C.c_int64(0)

    def refused(rc, name):
        assert rc == -1 and lib.nrv_last_error(h).decode().startswith(name + ": "), (name, rc, lib.nrv_last_error(h))

    refused(lib.nrv_fit_epoch(h, 0, rp, 33, C.byref(st)), "nrv_fit_epoch")            # before nrv_fit_begin
    refused(lib.nrv_fit_grad(h, 0, rp, 33, gp, C.byref(st)), "nrv_fit_grad")
    refused(lib.nrv_fit_eval(h, 0, rp, 33, None, C.byref(st)), "nrv_fit_eval")
    refused(lib.nrv_fit_params(h, 0, gp, None), "nrv_fit_params")
    refused(lib.nrv_fit_begin(h, 2, None, None), "nrv_fit_begin")
    rv.fit_begin(0, th)
    want_g, want_st = rv.fit_grad(0, rows)
    for model in (-1, 2):
        refused(lib.nrv_fit_grad(h, model, rp, 33, gp, C.byref(st)), "nrv_fit_grad")
        refused(lib.nrv_fit_epoch(h, model, rp, 33, C.byref(st)), "nrv_fit_epoch")
        refused(lib.nrv_fit_eval(h, model, rp, 33, None, C.byref(st)), "nrv_fit_eval")
        refused(lib.nrv_fit_params(h, model, gp, None), "nrv_fit_params")
    for b in (0, -1, 65537):
        refused(lib.nrv_fit_grad(h, 0, rp, b, gp, C.byref(st)), "nrv_fit_grad")
    refused(lib.nrv_fit_grad(h, 0, None, 33, gp, C.byref(st)), "nrv_fit_grad")
    refused(lib.nrv_fit_grad(h, 0, rp, 33, None, C.byref(st)), "nrv_fit_grad")
    refused(lib.nrv_fit_epoch(h, 0, None, 33, C.byref(st)), "nrv_fit_epoch")
    refused(lib.nrv_fit_eval(h, 0, None, 33, None, C.byref(st)), "nrv_fit_eval")
    bad = rows.copy()
    bad[17] = 33                                           # >= nrv_fit_count
    bp = bad.ctypes.data_as(C.POINTER(C.c_uint32))
    refused(lib.nrv_fit_grad(h, 0, bp, 33, gp, C.byref(st)), "nrv_fit_grad")
    refused(lib.nrv_fit_epoch(h, 0, bp, 33, C.byref(st)), "nrv_fit_epoch")
    refused(lib.nrv_fit_eval(h, 0, bp, 33, None, C.byref(st)), "nrv_fit_eval")
    refused(lib.nrv_fit_set_rows(h, None, None, None, None, 4), "nrv_fit_set_rows")
    refused(lib.nrv_fit_get_rows(h, 30, 4, None, None, None, None), "nrv_fit_get_rows")
    y6 = np.full(33, 6, np.uint8)
    with pytest.raises(NrvError) as e:
        rv.fit_set_rows(F, F, y6, np.minimum(y, 4))
    assert e.value.code == -1 and "nrv_fit_set_rows: a label outside" in str(e.value) and rv.fit_count() == 33
    bad_opts = tf.default_opts(0, B=0)
    with pytest.raises(NrvError) as e:
        rv.fit_begin(0, th, bad_opts)
    assert "nrv_fit_begin: B outside" in str(e.value)
    pk = _pack(rv, short_reads[:1])
    refused(lib.nrv_fit_add_reads_raw(*rv._raw_head(pk), None, None, None, C.byref(n_added)), "nrv_fit_add_reads_raw")
    # the refused nrv_fit_begin(B = 0) left no fit in progress... the one before it is still there: the next call succeeds
    g2, st2 = rv.fit_grad(0, rows)
    assert g2.tobytes() == want_g.tobytes() and st2 == want_st
    # between a _begin and its _end every fit call is refused under its own name
    n0 = len(short_reads[0].starts)
    t = rv.begin_packed_raw(pk)
    lab = np.ascontiguousarray(f32_calls["labels"][:n0])
    refused(lib.nrv_fit_reset(h), "nrv_fit_reset")
    assert lib.nrv_fit_count(h) == -1 and lib.nrv_last_error(h).decode().startswith("nrv_fit_count: ")
    refused(lib.nrv_fit_add_reads_raw(*rv._raw_head(pk), None, None, lab.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(n_added)), "nrv_fit_add_reads_raw")
    refused(lib.nrv_fit_set_rows(h, None, None, None, None, 0), "nrv_fit_set_rows")
    refused(lib.nrv_fit_get_rows(h, 0, 0, None, None, None, None), "nrv_fit_get_rows")
    refused(lib.nrv_fit_begin(h, 0, None, None), "nrv_fit_begin")
    refused(lib.nrv_fit_grad(h, 0, rp, 33, gp, C.byref(st)), "nrv_fit_grad")
    refused(lib.nrv_fit_epoch(h, 0, rp, 33, C.byref(st)), "nrv_fit_epoch")
    refused(lib.nrv_fit_eval(h, 0, rp, 33, None, C.byref(st)), "nrv_fit_eval")
    refused(lib.nrv_fit_params(h, 0, gp, None), "nrv_fit_params")
    p1, p2, a1, a2 = rv.end_packed_raw(t)
    w0 = f32_calls["p"][0][:n0 - 11]
    assert p1.tobytes() == w0.tobytes()                    # the call in flight was not disturbed
    g3, st3 = rv.fit_grad(0, rows)
    assert g3.tobytes() == want_g.tobytes() and st3 == want_st and rv.fit_count() == 33
    again = rv.predict_reads_raw(*_args(short_reads))
    assert again[0].tobytes() == f32_calls["p"][0].tobytes() and again[3].tobytes() == f32_calls["a"][1].tobytes()
    rv.close()


# ---- 10. command line ----------------------------------------------------------------------------------------------------
def test_command_line_trains_a_window_13_model_that_score_runs(tmp_path, monkeypatch, species_models):
    from nanoreviser_amd import cli, train_cli
    from nanoreviser_amd.weights import load_model
    from test_gpu_infix import mutate, random_seq, revcomp
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_SUMMARY",
              "NRV_TRIM_Q", "NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES", "NRV_INFIX", "NRV_LABELS", "NRV_LABELS_BUDGET", "NRV_SCORE",
              "NRV_LABELS_FROM", "NRV_CLI_GROUPS", "NRV_POISON", "NRV_PRECISION", "NRV_FIT_MAX_ROWS"):
        monkeypatch.delenv(k, raising=False)
    d = tmp_path / "in"
    d.mkdir()
    src = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")) + glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))
    n = 3
    for i in range(n):
        shutil.copy(src[i % len(src)], d / f"s{i:02d}.fast5")
    fa, ldir, out = str(tmp_path / "regions.fa"), str(tmp_path / "labels"), str(tmp_path / "plain") + "/"
    common = ["-d", str(d), "-S", "ecoli", "--gpus", "1", "--thread", "2"]
    assert cli.main(common + ["-o", out]) == 0
    rng = np.random.default_rng(8)
    with open(fa, "w") as fp:                              # the regions: a seeded 5 % mutation of what the plain run wrote, between flanks
        for i in range(n):
            if i != 2:                                     # one read without a truth: it gets no labels file
                t = random_seq(rng, 64 + i) + mutate(rng, open(out + f"s{i:02d}_out.fasta", "rb").read().split(b"\n")[1], 0.05) + random_seq(rng, 80)
                t = (revcomp(t) if i % 2 else t).decode()
                fp.write(f">s{i:02d}\n" + "".join(t[k:k + 70] + "\n" for k in range(0, len(t), 70)))
    assert cli.main(common + ["-o", str(tmp_path / "A") + "/", "--device_merge", "--truth", fa, "--infix", str(tmp_path / "A.inf"), "--labels", ldir]) == 0
    mdir = str(tmp_path / "model")
    assert train_cli.main(["-d", str(d), "-S", "ecoli", "-M", mdir, "-e", "2", "-w", "13", "--labels_from", ldir]) == 0
    m1, m2 = species_models["ecoli"]
    for k, m in enumerate((m1, m2)):
        stem = train_cli.stem(mdir, "ecoli", k + 1)
        back = load_model(stem + ".f32")
        assert back.T == 13 and back.n_class == m.n_class
        assert all(a.tobytes() == b.tobytes() for a, b in zip(back.tensors[:56], m.tensors[:56]))
        assert not np.array_equal(back.tensors[56], m.with_window(13).tensors[56]) and np.isfinite(back.flat()).all()
        hist = open(stem + "_history.tsv").read().split("\n")
        assert hist[0] == train_cli.HISTORY_HEAD and len(hist) == 4 and all(len(ln.split("\t")) == 8 for ln in hist[1:3])
        import json
        s = json.load(open(stem + "_summary.json"))
        assert s["rows"] > 1000 and s["reads"] == 2 and [x[0] for x in s["skipped_reads"]] == ["s02.fast5"] and s["options"]["init"] == "fresh"
        assert np.fromfile(stem + "_centers.f32", "<f4").size == 16 * m.n_class
    sc = str(tmp_path / "score.tsv")
    assert cli.main(common + ["-o", str(tmp_path / "B") + "/", "--model_dir", mdir, "--score", sc, "--labels_from", ldir]) == 0
    lines = open(sc).read().split("\n")
    assert lines[0] == cli.SCORE_HEADER and [ln.split("\t")[1] for ln in lines[1:4]] == ["scored", "scored", "no_labels"]
    assert all(int(ln.split("\t")[2]) > 1000 for ln in lines[1:4]) and int(lines[1].split("\t")[3]) > 1000    # windows at T = 13, labelled
