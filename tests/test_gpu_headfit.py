"""Fitting the whole head on the device (MI355X only, -m gpu): csrc/nrv_headfit.h through the nrv_fit_* entry points at depth
NRV_FIT_HEAD.  nanoreviser_amd/headfit.py is the definition; tests/headfit_cases.py holds the cases, the two f32 restatements
and the floors.
  1. gather and forward, bit for bit: nrv_fit_add_reads_raw at head depth on the two shortest fixture reads, seeded label bytes
     with 0xFF clips; count and y1 / y2 are the definition's, and nrv_fit_eval's p over all rows at the handle's own tensors
     50 .. 59 equals the labelled rows of an f32-mode handle's nrv_predict_reads_raw; the same from f16x2 and bf16x3 mode (mode
     left as it was), with the reads split over two adding calls, and nrv_fit_get_rows_head identical across all of these;
  2. gather against fp64: x4 against lstm4's output recomputed from the oracle's pieces in float64, precision_cases' f32 bounds;
  3. unit doors: nrv_fit_set_rows_head / _get_rows_head round trip byte for byte, sub-ranges too;
  4. gradient: nrv_fit_grad per tensor and sum in units of the floor of the two CPU restatements, held to cpu_bound; counts exact;
  5. Adam, bit for bit: one epoch of one batch = tailfit_cases.adam_f32 on the vector nrv_fit_grad returned, whole head vector;
  6. epoch, bit for bit: 1100 rows at B = 512, T = 11 against the host loop of nrv_fit_grad + adam_f32; two runs, the same bytes;
  7. a NaN row: its batch is skipped and counted, t does not advance, the other batches update;
  8. it learns: labels = the handle's own answers, start fresh_head; loss falls, accuracy beats the majority class;
  9. depth and refusals by name; back at tail depth a tailfit_cases gradient case still meets its bound;
 10. handles created under NRV_POISON: 1 and 6 unchanged;
 11. the command line: --labels, NanoReviser_train.py --fit_depth head -e 2, NanoReviser.py --score on the written directory; a
     fresh f32-mode handle made from the written .f32 returns nrv_fit_eval's p at the final parameters for the labelled windows."""
import ctypes as C
import glob
import math
import os
import shutil

import numpy as np
import pytest

import headfit_cases as hc
import tailfit_cases as tc
from conftest import GOLD
from nanoreviser_amd import headfit as hf
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.engine import NrvError
from score_cases import VALID

pytestmark = pytest.mark.gpu

PATTERNS = {"qnan": 0x7FC00000, "m1500": 0xC4BB8000}
ENV = ("NRV_PRECISION", "NRV_COALESCE", "NRV_LANES", "NRV_POISON", "NRV_FIT_MAX_ROWS", "NRV_FIT_MAX_HEAD_ROWS")
IDS = lambda c: "T%d-m%d-n%d-%s" % c      # noqa: E731


def _engine(monkeypatch, m1, m2, poison=None, depth="head", **kw):
    from nanoreviser_amd.engine import Reviser
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if poison is not None:
        monkeypatch.setenv("NRV_POISON", f"{PATTERNS[poison]:08x}")
    rv = Reviser(m1, m2, **kw)
    monkeypatch.delenv("NRV_POISON", raising=False)
    assert rv.fit_depth() == 0 and rv.fit_n_params(0) == tf.n_params(rv.T, 6)          # the default is today's
    if depth == "head":
        rv.fit_set_depth("head")
        assert rv.fit_depth() == 1 and rv.fit_n_params(0) == hf.n_params(rv.T, 6) and rv.fit_n_params(1) == hf.n_params(rv.T, 5)
    return rv


@pytest.fixture(scope="module")
def short_reads(reads):
    out = []
    for k in reads.keys:
        _, rd, _ = reads(k)
        out.append(hs.read_tensors_raw(rd))
    return sorted(out, key=lambda r: len(r.starts))[:2]


def _labels_for(rrs, seed=91):
    """tests/test_gpu_tailfit.py's label bytes: seeded valid bytes with 0xFF clips at both ends of every read, a run inside and
    bytes whose code is 0, 6 or 7."""
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
    """The set after adding the two reads (in one call, or one call each) -> (x1, x2, p1 rows, p2 rows)."""
    rv.fit_reset()
    assert rv.fit_count() == 0 and rv.fit_depth() == 1
    if split:
        n0 = len(rrs[0].starts)
        added = rv.fit_add_packed(_pack(rv, rrs[:1]), c["labels"][:n0]) + rv.fit_add_packed(_pack(rv, rrs[1:]), c["labels"][n0:])
    else:
        added = rv.fit_add_packed(_pack(rv, rrs), c["labels"])
    assert added == rv.fit_count() == c["w"].size > 1000
    x1, x2, y1, y2 = rv.fit_get_rows_head()
    assert np.array_equal(y1, c["y"][0]) and np.array_equal(y2, c["y"][1])
    ps = []
    for k in (0, 1):
        rv.fit_begin(k)                                    # the handle's own tensors 50 .. 59: the model nrv_predict* runs
        p, st = rv.fit_eval(k, _all_rows(rv))
        assert st.rows == added and st.steps == 0 and st.nonfinite == 0
        assert st.correct == int((c["a"][k][c["w"]] == c["y"][k]).sum())
        ps.append(p)
    return x1, x2, ps[0], ps[1]


def _check_gather(rv, rrs, c, what):
    got = _gathered(rv, rrs, c)
    for k in (0, 1):
        want = c["p"][k][c["w"]]
        assert got[2 + k].dtype == np.float32 and got[2 + k].tobytes() == want.tobytes(), (what, k, np.argwhere(got[2 + k] != want)[:4].tolist())
    return got


# ---- 1. gather and forward, bit for bit ------------------------------------------------------------------------------------
def test_gather_and_forward_are_the_f32_modes_rows_bit_for_bit(species_models, short_reads, f32_calls, monkeypatch):
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
    x1 = ref[0]
    assert x1.shape == (f32_calls["w"].size, 11, 128) and np.isfinite(x1).all() and np.abs(x1).max() <= 1 and x1.std() > 0.05
    assert not np.array_equal(x1[0], x1[1]) and not np.array_equal(ref[0], ref[1])
    # N <= T adds nothing; a predict on the same handle afterwards returns its usual bytes
    r0 = short_reads[0]
    p = rv.pack_reads_raw([r0.raw], [r0.starts[:11]], [r0.feat_ev[:11]], [r0.shift], [r0.scale], rv.T)
    assert rv.fit_add_packed(p, np.full(11, 5, np.uint8)) == 0 and rv.fit_count() == f32_calls["w"].size
    rv.set_precision("f32")
    again = rv.predict_reads_raw(*_args(short_reads))
    assert again[0].tobytes() == f32_calls["p"][0].tobytes() and again[1].tobytes() == f32_calls["p"][1].tobytes()
    rv.close()


# ---- 2. gather against fp64 ------------------------------------------------------------------------------------------------
def _lstm4_out(w, sig, rd, dtype):
    """lstm4's output of these windows from oracle.nrv_oracle's own pieces: what tests/test_gpu_tailfit.py's _main_out passes
    through on its way to main_out."""
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
    return O.bilstm(x, w[44:50], act).reshape(B, T * 128)


def test_gathered_rows_against_fp64(species_models, short_reads, f32_calls, monkeypatch):
    import precision_cases as pc
    rv = _engine(monkeypatch, *species_models["ecoli"])
    x1, x2 = _gathered(rv, short_reads, f32_calls)[:2]
    rv.close()
    sig_ev = np.concatenate([hs.segment_windows_f32(r.raw, r.starts, r.shift, r.scale) for r in short_reads])
    feat_ev = np.concatenate([r.feat_ev for r in short_reads])
    pick = np.linspace(0, f32_calls["w"].size - 1, 256).astype(np.int64)      # 256 labelled rows across both reads
    idx = f32_calls["w"][pick][:, None] + np.arange(11)[None, :]
    sig, rd = sig_ev[idx], feat_ev[idx]
    for k, (m, x) in enumerate(zip(species_models["ecoli"], (x1, x2))):
        with np.errstate(over="ignore"):
            f64, f32 = _lstm4_out(m.tensors, sig, rd, np.float64), _lstm4_out(m.tensors, sig, rd, np.float32)
        floor = np.abs(f32 - f64).max(-1)
        r = np.abs(x[pick].reshape(256, -1).astype(np.float64) - f64).max(-1) / np.maximum(floor, np.median(floor))
        K = pc.K_for(pc.key("fixture", "ecoli", k + 1, "hard_sigmoid"), "f32")
        print(f"model{k + 1}: gathered lstm4 rows over the f32 floor: median {np.median(r):.3g} (bound {K['med_r']}), "
              f"q90 {np.quantile(r, 0.9):.3g} (bound {K['q90_r']})")
        assert np.median(r) <= K["med_r"] and np.quantile(r, 0.9) <= K["q90_r"], (k, float(np.median(r)), float(np.quantile(r, 0.9)))


# ---- 3 .. 7. the step on host-supplied rows --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles(species_models):
    """One head-depth handle per window length, made on first use and shared (nrv_fit_set_rows_head replaces the set)."""
    from nanoreviser_amd.engine import Reviser
    made = {}

    def get(T):
        if T not in made:
            m1, m2 = species_models["ecoli"]
            made[T] = Reviser(m1.with_window(T), m2.with_window(T))
            made[T].fit_set_depth("head")
        return made[T]
    yield get
    for rv in made.values():
        rv.close()


def _set_case(rv, case):
    T, model, n, kind = case
    X, y, th = hc.rows_case(*case)
    other = np.minimum(y, 4)                               # the other model's labels only have to be valid
    rv.fit_set_rows_head(X, X, y if model == 0 else other, other if model == 0 else y)
    assert rv.fit_count() == n
    return X, y, th


def test_unit_doors_round_trip(handles):
    rv = handles(13)
    rng = np.random.default_rng(12)
    n = 77
    x1, x2 = (rng.uniform(-1, 1, (n, 13, 128)).astype(np.float32) for _ in range(2))
    y1, y2 = rng.integers(0, 6, n).astype(np.uint8), rng.integers(0, 5, n).astype(np.uint8)
    rv.fit_set_rows_head(x1, x2, y1, y2)
    assert rv.fit_count() == n
    got = rv.fit_get_rows_head()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, (x1, x2, y1, y2)))
    for first, count in ((0, 1), (31, 33), (76, 1), (77, 0), (5, 0)):
        sub = rv.fit_get_rows_head(first, count)
        assert all(a.tobytes() == b[first:first + count].tobytes() for a, b in zip(sub, (x1, x2, y1, y2))), (first, count)
    with pytest.raises(NrvError, match="nrv_fit_get_rows_head: rows outside the training set"):
        rv.fit_get_rows_head(70, 8)
    rv.fit_set_rows_head(x2[:3], x1[:3], y1[:3], y2[:3])     # replaces the set
    assert rv.fit_count() == 3 and rv.fit_get_rows_head()[0].tobytes() == x2[:3].tobytes()
    with pytest.raises(ValueError):
        rv.fit_set_rows_head(x1[:, :11], x2[:, :11], y1, y2)
    rv.fit_reset()
    assert rv.fit_count() == 0


@pytest.fixture(scope="module")
def grade_bound():
    K, worst = hc.cpu_bound()
    print(f"head depth: gradient bound sized on the CPU: K = {K:.3g} (worst restatement grade {worst:.3g})")
    return K


@pytest.mark.parametrize("case", hc.GRAD_CASES, ids=IDS)
def test_gradient_against_the_definition(handles, grade_bound, case):
    T, model, n, kind = case
    C = hc.n_class(model)
    rv = handles(T)
    X, y, th = _set_case(rv, case)
    rv.fit_begin(model, th)
    g, st = rv.fit_grad(model, np.arange(n))
    ref = hc.grad_reference(*case)
    grades = hc.device_grades(g, st.ce_sum, st.center_sum, ref, T, C)
    print(case, {k: round(v, 3) for k, v in grades.items()}, "bound", round(grade_bound, 3))
    assert g.size == hf.n_params(T, C) and np.isfinite(g).all() and max(grades.values()) <= grade_bound, grades
    s64 = ref["st64"]
    assert (st.rows, st.correct, st.steps, st.nonfinite) == (n, s64.correct, 0, 0)
    assert rv.fit_params(model)[0].tobytes() == th.tobytes() and rv.fit_params(model)[1] == 0     # nothing was updated
    g1, st1 = rv.fit_grad(model, np.arange(n))
    assert g1.tobytes() == g.tobytes() and st1 == st                                           # the same call, the same bytes
    # a permutation of the rows is the same batch: the same statistics, the gradient within the same bound
    perm = np.random.default_rng(n).permutation(n)
    g2, st2 = rv.fit_grad(model, perm)
    assert st2.correct == st.correct and max(hc.device_grades(g2, st2.ce_sum, st2.center_sum, ref, T, C).values()) <= grade_bound
    # forward only: p is the definition's within f32, the same counts and sums as the gradient call's
    p, se = rv.fit_eval(model, np.arange(n))
    p64 = hf.forward(X, th, T, C, np.float64)[2]
    assert np.abs(p - p64).max() <= 64 * tc.EPS32 and (se.rows, se.correct, se.ce_sum, se.center_sum) == (n, st.correct, st.ce_sum, st.center_sum)


@pytest.mark.parametrize("case", [(11, 1, 33, "plain"), (1, 1, 32, "absent"), (32, 0, 33, "zeros"), (11, 0, 512, "plain")], ids=IDS)
def test_one_step_is_numpy_f32_adam_bit_for_bit(handles, case):
    T, model, n, kind = case
    rv = handles(T)
    X, y, th = _set_case(rv, case)
    opts = tf.default_opts(model)
    rv.fit_begin(model, th, opts)
    g, _ = rv.fit_grad(model, np.arange(n))
    st = rv.fit_epoch(model, np.arange(n))
    got, t = rv.fit_params(model)
    want = tc.adam_f32(th, np.zeros_like(th), np.zeros_like(th), g, opts, 1)[0]
    assert (t, st.steps, st.rows, st.nonfinite) == (1, 1, n, 0)
    assert got.size == hf.n_params(T, 6 - model) and got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8].tolist()
    sp = hc.spans(T, 6 - model)
    assert all(not np.array_equal(got[sp[k]], th[sp[k]]) for k in hc.TENSORS)                 # every tensor moved
    rv.fit_begin(model, th)                                # opts NULL: the engine's defaults are the definition's
    rv.fit_epoch(model, np.arange(n))
    assert rv.fit_params(model)[0].tobytes() == want.tobytes()


def _epoch_and_loop(rv, model, th, order, opts):
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


EPOCH_CASE = (11, 0, 1100, "plain")


def test_epoch_is_the_host_loop_bit_for_bit(handles):
    T, model, n, _ = EPOCH_CASE
    rv = handles(T)
    X, y, th = _set_case(rv, EPOCH_CASE)
    opts = tf.default_opts(model, B=512)                   # batches of 512, 512, 76
    order = np.random.default_rng(4).permutation(n).astype(np.uint32)
    got, st, t, want = _epoch_and_loop(rv, model, th, order, opts)
    assert (t, st.steps, st.rows, st.nonfinite) == (3, 3, n, 0)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8].tolist()
    rv.fit_begin(model, th, opts)
    st2 = rv.fit_epoch(model, order)
    assert rv.fit_params(model)[0].tobytes() == got.tobytes() and st2 == st         # two runs: the same bytes
    st3 = rv.fit_epoch(model, order)                       # a second epoch goes on from t = 3
    assert rv.fit_params(model)[1] == 6 and st3.steps == 3 and st3.ce_sum != st.ce_sum
    # the definition's epoch in f64 from the same start: the statistics agree to f32
    s = tf.FitState(th.astype(np.float64))
    d = hf.epoch(X, y, s, order, T, 6, opts, np.float64)
    assert abs(st.ce_sum - d.ce_sum) <= 1e-4 * d.ce_sum and abs(st.center_sum - d.center_sum) <= 1e-4 * d.center_sum


def test_nonfinite_batch_is_skipped_and_counted(handles):
    T, model, n = 11, 1, 1100
    rv = handles(T)
    X, y, th = hc.rows_case(T, model, n)
    X = X.copy()
    X[600, 3, 7] = np.nan                                  # the second batch of 512
    other = np.minimum(y, 4)
    rv.fit_set_rows_head(X, X, other, y)
    opts = tf.default_opts(model, B=512)
    rv.fit_begin(model, th, opts)
    order = np.arange(n, dtype=np.uint32)
    st = rv.fit_epoch(model, order)
    got, t = rv.fit_params(model)
    assert (t, st.steps, st.nonfinite, st.rows) == (2, 2, 1, 588) and np.isfinite(got).all()
    assert math.isfinite(st.ce_sum) and math.isfinite(st.center_sum) and not np.array_equal(got, th)
    g, sg = rv.fit_grad(model, order[512:1024])
    assert sg.nonfinite == 1 and not np.isfinite(g).all()
    keep = np.concatenate([order[:512], order[1024:]])     # the same epoch without the batch: the same bytes, t included
    rv.fit_begin(model, th, tf.default_opts(model, B=512))
    st2 = rv.fit_epoch(model, keep)
    assert rv.fit_params(model)[0].tobytes() == got.tobytes() and rv.fit_params(model)[1] == 2 and st2.nonfinite == 0


# ---- 8. it learns ----------------------------------------------------------------------------------------------------------
LEARN_E, LEARN_SEED = 8, 3


def test_a_fresh_head_recovers_the_teacher(species_models, short_reads, f32_calls, monkeypatch):
    """Teacher recovery as tests/test_gpu_tailfit.py has it, one depth further back: every window of the two shortest fixture
    reads, labels = the f32-mode handle's own a1 / a2, all five layers re-drawn (headfit.fresh_params, seed LEARN_SEED + model),
    LEARN_E epochs at the defaults.  Only conditions are asserted: the last epoch's training loss is below the first's and the
    training accuracy is above the majority-class rate of those labels.  E and the seed are the tail test's own, not chosen
    here.  Figures of one MI355X run (13 525 rows; not asserted):
      model 1  majority 0.2618; loss 1.9195 -> 1.0156; accuracy 0.4917 -> 0.9766
      model 2  majority 0.2696; loss 1.5319 -> 0.6371; accuracy 0.5418 -> 0.9975"""
    a1, a2 = f32_calls["a"]
    el = [len(r.starts) for r in short_reads]
    lab = np.full(sum(el), 5, np.uint8)                    # every window of either read is labelled ...
    w = tf.labelled_windows(lab, el, 11)[0]
    rv = _engine(monkeypatch, *species_models["ecoli"])
    n = rv.fit_add_packed(_pack(rv, short_reads), lab)
    assert n == w.size == sum(el) - 22
    x1, x2, _, _ = rv.fit_get_rows_head()
    y1, y2 = a1[w].astype(np.uint8), a2[w].astype(np.uint8)
    rv.fit_set_rows_head(x1, x2, y1, y2)                   # ... and the labels are the handle's own answers
    for k, y in enumerate((y1, y2)):
        C = 6 - k
        majority = np.bincount(y, minlength=C).max() / n
        th0 = hf.fresh_params(11, C, LEARN_SEED + k)
        first = tf.epoch_order(n, LEARN_SEED, 0)[:512]
        rv.fit_begin(k, th0, tf.default_opts(k))
        _, se = rv.fit_eval(k, first)
        s0 = rv.fit_epoch(k, first)                        # one batch: its statistics are those before the first update
        assert s0.steps == 1 and (s0.rows, s0.correct, s0.ce_sum, s0.center_sum) == (se.rows, se.correct, se.ce_sum, se.center_sum)
        assert s0.loss() == se.loss() and s0.loss()[0] > 0
        rv.fit_begin(k, th0, tf.default_opts(k))
        hist = [rv.fit_epoch(k, tf.epoch_order(n, LEARN_SEED, ep)) for ep in range(LEARN_E)]
        loss = [h.loss()[0] for h in hist]
        print(f"model{k + 1}: majority {majority:.4f}, loss {loss[0]:.4f} -> {loss[-1]:.4f}, acc {hist[0].acc():.4f} -> {hist[-1].acc():.4f}")
        assert all(h.nonfinite == 0 for h in hist) and loss[-1] < loss[0]
        assert hist[-1].acc() > majority, (k, hist[-1].acc(), majority)
    rv.close()


# ---- 9. depth and refusals -------------------------------------------------------------------------------------------------
def test_depth_and_refusals_by_name(species_models, short_reads, f32_calls, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    rv = _engine(monkeypatch, *species_models["ecoli"], depth="tail", precision="f32")
    lib, h = rv._lib, rv._h

    def refused(rc, name, word=""):
        err = lib.nrv_last_error(h).decode()
        assert rc == -1 and err.startswith(name + ": ") and word in err, (name, rc, err)

    # at tail depth the _head doors are refused, each under its own name
    case = (11, 0, 33, "plain")
    X, y, th = hc.rows_case(*case)
    y2 = np.minimum(y, 4)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_head: the set is at tail depth"):
        rv.fit_set_rows_head(X, X, y, y2)
    refused(lib.nrv_fit_get_rows_head(h, 0, 0, None, None, None, None), "nrv_fit_get_rows_head", "tail depth")
    refused(lib.nrv_fit_set_depth(h, 2), "nrv_fit_set_depth", "NRV_FIT_TAIL or NRV_FIT_HEAD")
    # a non-empty set keeps its depth
    F, yt, tht = tc.rows_case(11, 0, 33)
    rv.fit_set_rows(F, F, yt, np.minimum(yt, 4))
    refused(lib.nrv_fit_set_depth(h, 1), "nrv_fit_set_depth", "not empty")
    assert rv.fit_depth() == 0 and rv.fit_count() == 33
    rv.fit_begin(0, tht)
    g_tail, _ = rv.fit_grad(0, np.arange(33))              # the refusals left the handle usable
    rv.fit_reset()
    rv.fit_set_depth("head")
    assert rv.fit_depth() == 1 and rv.fit_count() == 0
    # it forgot the nrv_fit_begin
    rows = np.arange(33, dtype=np.uint32)
    rp = rows.ctypes.data_as(C.POINTER(C.c_uint32))
    refused(lib.nrv_fit_params(h, 0, None, None), "nrv_fit_params", "nrv_fit_begin")
    # at head depth the flat doors are refused
    with pytest.raises(NrvError, match="nrv_fit_set_rows: the set is at head depth"):
        rv.fit_set_rows(F, F, yt, np.minimum(yt, 4))
    refused(lib.nrv_fit_get_rows(h, 0, 0, None, None, None, None), "nrv_fit_get_rows", "head depth")
    refused(lib.nrv_fit_set_rows_head(h, None, None, None, None, 4), "nrv_fit_set_rows_head", "null rows")
    y6 = np.full(33, 6, np.uint8)
    with pytest.raises(NrvError, match="nrv_fit_set_rows_head: a label outside"):
        rv.fit_set_rows_head(X, X, y6, y2)
    rv.fit_set_rows_head(X, X, y, y2)
    refused(lib.nrv_fit_set_depth(h, 0), "nrv_fit_set_depth", "not empty")
    # a parameter count of the other depth is refused
    with pytest.raises(ValueError, match=f"expected {hf.n_params(11, 6)} parameters, got {tf.n_params(11, 6)}"):
        rv.fit_begin(0, tht)
    rv.fit_begin(0, th)
    want_g, want_st = rv.fit_grad(0, rows)
    assert want_g.size == hf.n_params(11, 6)
    # between a _begin and its _end the depth cannot change and the _head doors are refused under their own names
    pk = _pack(rv, short_reads[:1])
    n0 = len(short_reads[0].starts)
    t = rv.begin_packed_raw(pk)
    refused(lib.nrv_fit_set_depth(h, 0), "nrv_fit_set_depth", "in flight")
    refused(lib.nrv_fit_set_rows_head(h, None, None, None, None, 0), "nrv_fit_set_rows_head", "in flight")
    refused(lib.nrv_fit_get_rows_head(h, 0, 0, None, None, None, None), "nrv_fit_get_rows_head", "in flight")
    assert lib.nrv_fit_depth(h) == 1
    p1 = rv.end_packed_raw(t)[0]
    assert p1.tobytes() == f32_calls["p"][0][:n0 - 11].tobytes()                             # the call in flight was not disturbed
    g3, st3 = rv.fit_grad(0, rows)
    assert g3.tobytes() == want_g.tobytes() and st3 == want_st and rv.fit_count() == 33
    rv.close()
    # a handle under NRV_FIT_MAX_HEAD_ROWS = 1000 refuses an adding call whole, by that name, and stays usable
    monkeypatch.setenv("NRV_FIT_MAX_HEAD_ROWS", "1000")
    rv = Reviser(*species_models["ecoli"])
    monkeypatch.delenv("NRV_FIT_MAX_HEAD_ROWS")
    rv.fit_set_depth("head")
    with pytest.raises(NrvError) as e:
        rv.fit_add_packed(_pack(rv, short_reads), f32_calls["labels"])
    assert e.value.code == -1 and "nrv_fit_add_reads_raw: the call would pass the row cap" in str(e.value) and "NRV_FIT_MAX_HEAD_ROWS" in str(e.value)
    assert rv.fit_count() == 0
    with pytest.raises(NrvError, match="NRV_FIT_MAX_HEAD_ROWS"):
        rv.fit_set_rows_head(np.zeros((1001, 11, 128), np.float32), np.zeros((1001, 11, 128), np.float32), np.zeros(1001, np.uint8), np.zeros(1001, np.uint8))
    lab = f32_calls["labels"][:n0].copy()
    lab[400:] = 0xFF                                       # fewer than 1000 labelled windows: accepted
    assert 0 < rv.fit_add_packed(_pack(rv, short_reads[:1]), lab) == rv.fit_count() <= 1000
    # the tail depth's own cap is not the head's: back at tail depth the whole call fits
    rv.fit_reset()
    rv.fit_set_depth("tail")
    assert rv.fit_add_packed(_pack(rv, short_reads), f32_calls["labels"]) == f32_calls["w"].size
    # back at tail depth, one tail-depth gradient case of tailfit_cases still meets its bound
    rv.fit_reset()
    tcase = (11, 0, 33, "plain")
    rv.fit_set_rows(F, F, yt, np.minimum(yt, 4))
    rv.fit_begin(0, tht)
    g, st = rv.fit_grad(0, np.arange(33))
    K, _ = tc.cpu_bound()
    ref = tc.grad_reference(*tcase)
    grades = tc.device_grades(g, st.ce_sum, st.center_sum, ref, 11, 6)
    assert g.size == tf.n_params(11, 6) and max(grades.values()) <= K, grades
    assert g.tobytes() == g_tail.tobytes()                 # and is what the handle that never left tail depth gave
    rv.close()


# ---- 10. poison ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", sorted(PATTERNS))
def test_poisoned_handles_give_the_same_bytes(species_models, short_reads, f32_calls, handles, monkeypatch, poison):
    rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
    _check_gather(rv, short_reads, f32_calls, poison)
    X, y, th = _set_case(rv, EPOCH_CASE)
    opts = tf.default_opts(0, B=512)
    order = np.random.default_rng(4).permutation(1100).astype(np.uint32)
    got, st, t, want = _epoch_and_loop(rv, 0, th, order, opts)
    assert got.tobytes() == want.tobytes() and (t, st.steps) == (3, 3)
    clean = handles(11)
    _set_case(clean, EPOCH_CASE)
    clean.fit_begin(0, th, opts)
    assert clean.fit_epoch(0, order) == st and clean.fit_params(0)[0].tobytes() == got.tobytes()
    rv.close()


# ---- 11. command line ------------------------------------------------------------------------------------------------------
def test_command_line_trains_a_head_that_score_runs(tmp_path, monkeypatch, species_models):
    import json
    from nanoreviser_amd import cli, train_cli
    from nanoreviser_amd.engine import Reviser
    from nanoreviser_amd.weights import load_model
    from test_gpu_infix import mutate, random_seq, revcomp
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_SUMMARY",
              "NRV_TRIM_Q", "NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES", "NRV_INFIX", "NRV_LABELS", "NRV_LABELS_BUDGET", "NRV_SCORE",
              "NRV_LABELS_FROM", "NRV_CLI_GROUPS") + ENV:
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
    added, made = [], []

    class Kept(Reviser):                                   # the command line's own engine, kept open behind its close()
        def fit_add_packed(self, packed, labels):
            added.append((packed, np.array(labels, np.uint8)))
            return super().fit_add_packed(packed, labels)

        def close(self):
            pass

    def factory(a, m1, m2):
        made.append(Kept(m1, m2, device=0))
        return made[-1]
    assert train_cli.main(["-d", str(d), "-S", "ecoli", "-M", mdir, "-e", "2", "--fit_depth", "head", "--labels_from", ldir],
                          reviser_factory=factory) == 0
    rv = made[0]
    try:
        assert rv.fit_depth() == 1 and rv.fit_count() > 1000
        m1, m2 = species_models["ecoli"]
        backs, finals = [], []
        for k, m in enumerate((m1, m2)):
            stem = train_cli.stem(mdir, "ecoli", k + 1)
            back = load_model(stem + ".f32")
            assert back.T == 11 and back.n_class == m.n_class and np.isfinite(back.flat()).all()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(back.tensors[:50], m.tensors[:50]))
            assert all(not np.array_equal(a, b) for a, b in zip(back.tensors[50:], m.tensors[50:]))      # all ten were fitted
            theta, t = rv.fit_params(k)
            assert theta.size == hf.n_params(11, m.n_class) and t > 0
            assert all(a.tobytes() == b.tobytes() for a, b in zip(back.tensors[50:], hf.unpack(theta, 11, m.n_class)[:10]))
            hist = open(stem + "_history.tsv").read().split("\n")
            assert hist[0] == train_cli.HISTORY_HEAD and len(hist) == 4 and all(len(ln.split("\t")) == 8 for ln in hist[1:3])
            s = json.load(open(stem + "_summary.json"))
            assert s["rows"] == rv.fit_count() and s["reads"] == 2 and [x[0] for x in s["skipped_reads"]] == ["s02.fast5"]
            assert s["options"]["init"] == "transfer" and s["options"]["fit_depth"] == "head"
            assert np.fromfile(stem + "_centers.f32", "<f4").size == 16 * m.n_class
            backs.append(back)
            finals.append(rv.fit_eval(k, _all_rows(rv))[0])                                   # p at the final parameters
        # the written file IS the fitted vector: a fresh f32-mode handle made from it answers the labelled windows with those p
        rv2 = Reviser(backs[0], backs[1], precision="f32")
        got = [[], []]
        for packed, labels in added:
            descs, nr = packed[3], packed[4]
            w = tf.labelled_windows(labels, [descs[i].ev_len for i in range(nr)], 11)[0]
            p = rv2.run_packed_raw(packed)
            for k in (0, 1):
                got[k].append(np.array(p[k][w]))
        rv2.close()
        for k in (0, 1):
            g = np.concatenate(got[k])
            assert g.shape == finals[k].shape and g.tobytes() == finals[k].tobytes(), (k, np.argwhere(g != finals[k])[:4].tolist())
    finally:
        Reviser.close(rv)
    sc = str(tmp_path / "score.tsv")
    assert cli.main(common + ["-o", str(tmp_path / "B") + "/", "--model_dir", mdir, "--score", sc, "--labels_from", ldir]) == 0
    lines = open(sc).read().split("\n")
    assert lines[0] == cli.SCORE_HEADER and [ln.split("\t")[1] for ln in lines[1:4]] == ["scored", "scored", "no_labels"]
    assert all(int(ln.split("\t")[2]) > 1000 for ln in lines[1:4]) and int(lines[1].split("\t")[3]) > 1000
