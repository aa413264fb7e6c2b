"""Weights outside the shipped range in every arithmetic mode (MI355X only, -m gpu).

The default f16x2 arithmetic derives its power-of-two exponents from the weights at nrv_create (nrv_api.hip upload_model:
pow2_room, plan_exponent, bn_exp, pack_head_h2, the BatchNorm folds) and keeps four scales that no weight influences (the
signal branch's output x 2^6, the 400 -> 64 dense weights x 2^10, its bias x 2^16, the conv1 guard's room of 1000).  The
shipped weight files exercise one point of that plan.  tests/weight_cases.py moves the SAME function (tests/
test_weight_cases_host.py pins that: the oracle's answer does not change by one bit) to other points of it:

  * f32 and bf16x3 claim to hold no magnitude-dependent constant: power-of-two scaling commutes with every IEEE operation
    they perform (bn_fold, the double-precision sh.W fold, the exact three-term bf16 split), so their outputs on a
    reparametrised model must be the shipped model's outputs BIT FOR BIT;
  * f16x2 must meet the unchanged parity policy (parity_policy.BAR, at most 1 % ill-conditioned windows) against the fp64
    oracle and the f32 floors of the SHIPPED weights; it may hand a stage to the f32 kernels only where its fixed scales
    cannot hold the values (then the result is the f32 mode's, bit for bit), and must not where they can;
  * degenerate weights (zero tensors, BatchNorm scales of 0, a layer 2^-20 of its size) against their own live oracle.

The reparametrisations cannot change WHICH block of a layer sets its accumulator exponent (plan_exponent's minimum): every
exponent they move is matched by the weights it scales.  Two more families do, both against their own live oracle, in every
mode, with no stage handed to the f32 kernels (tests/test_weight_cases_host.py pins on the CPU that each case reaches the
branch it names, that the reference alone has no ill-conditioned window on it and that every value fits the fixed scales):

  * weight_cases.plan_case: input rows starved until the recurrent block (13 + room(U)) binds by three binades - it binds in
    no shipped model - or until the BatchNorm block of the 192 -> 128 layer does;
  * weight_cases.unseen: hybrids of the two species, their midpoint, jittered, pruned, outlier-ridden, recurrent-heavy,
    BatchNorm-shifted and freshly initialised weights.
"""
import numpy as np
import pytest

from nanoreviser_amd import hoststage as hs
from parity_policy import BAR, check_vs_fp64, f32_floor
from weight_cases import (DEGENERATE_CASES, LAYERS, PLAN_CASES, REPARAM_CASES, SIGMOID_ADMITTED, UNSEEN_ADMITTED, binding,
                          case_windows, degenerate, f16x2_must_not_rerun, f32_floor_act, plan_case, plan_terms, reparam, unseen)

pytestmark = pytest.mark.gpu

SPECIES = ["ecoli", "human"]
MODES = ["f16x2", "bf16x3", "f32"]
SCALED = [s for s in REPARAM_CASES if s != "lstm3_perm"]
CS = [2.0 ** -6, 2.0 ** -3, 2.0 ** 3, 2.0 ** 6]
CS_EXACT = (2.0 ** -6, 2.0 ** 6)                 # where the f32 / bf16x3 bit-identity is checked as well


@pytest.fixture(scope="module")
def shipped(reads, species_models):
    """Per species, computed once and left unchanged: the 256 windows, the fp64 oracle and the f32 floors of the shipped
    weights, and the shipped weights' outputs in every mode."""
    from nanoreviser_amd.engine import Reviser
    from oracle import nrv_oracle as O
    sw, fw = case_windows(reads)
    out = {"sw": sw, "fw": fw}
    for sp in SPECIES:
        m1, m2 = species_models[sp]
        q1, q2, _, _ = O.predict_pair(m1.tensors, m2.tensors, sw, fw, np.float64)
        nf1, nf2 = f32_floor(m1, m2, sw, fw, q1, q2)
        rv = Reviser(m1, m2)
        got = {}
        for mode in MODES:
            rv.set_precision(mode)
            got[mode] = rv.predict_pair(sw, fw)
        assert rv.saturated() == (0, 0)
        rv.close()
        out[sp] = {"q": (q1, q2), "nf": (nf1, nf2), "got": got}
    return out


def _policy(got, q, nf, what):
    r1 = check_vs_fp64(got[0], got[2], q[0], nf[0], what + " m1", max_ill=0.01, bar=BAR)
    r2 = check_vs_fp64(got[1], got[3], q[1], nf[1], what + " m2", max_ill=0.01, bar=BAR)
    return {"m1": r1, "m2": r2}


@pytest.mark.parametrize("sp", SPECIES)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("site", SCALED)
def test_reparametrised_weights(shipped, species_models, sp, site, c):
    from nanoreviser_amd.engine import Reviser
    m1, m2 = species_models[sp]
    k1, k2 = reparam(m1, site, c), reparam(m2, site, c)
    sw, fw, base = shipped["sw"], shipped["fw"], shipped[sp]
    rv = Reviser(k1, k2, precision="f16x2")
    got = rv.predict_pair(sw, fw)
    _, reruns = rv.saturated()
    rv.set_precision("f32")
    ref32 = rv.predict_pair(sw, fw)
    exact = {"f32": ref32}
    if c in CS_EXACT:
        rv.set_precision("bf16x3")
        exact["bf16x3"] = rv.predict_pair(sw, fw)
    assert rv.saturated() == (0, reruns)                       # (the count is cumulative: the guard belongs to f16x2 alone)
    rv.close()
    if c in CS_EXACT:
        # no instruction of these two modes breaks the commutation with a power of two: bit for bit the shipped model's result
        for mode, out in exact.items():
            for g, b in zip(out, base["got"][mode]):
                assert np.array_equal(g, b), f"{mode} {sp} {site} c={c:g}: not the shipped weights' bits"
    res = _policy(got, base["q"], base["nf"], f"f16x2 {sp} {site} c={c:g}")
    print(f"WEIGHTS {sp} {site} c={c:g}: reruns {reruns} {res}")
    if reruns > 0:
        for g, r in zip(got, ref32):
            assert np.array_equal(g, r)                        # a re-run stage IS the f32 kernels' result
    if f16x2_must_not_rerun(k1, k2, sw):
        assert reruns == 0, f"{sp} {site} c={c:g}: every value fits the f16x2 scales, yet {reruns} stage(s) ran in f32"


@pytest.mark.parametrize("sp", SPECIES)
def test_lstm3_hidden_units_permuted(shipped, species_models, sp):
    """The permutation changes the summation order of lstm3's recurrence and of its consumers: no bit-identity, the parity
    policy in every mode (oracle and floors of the shipped weights: the function is the same to 1e-12)."""
    from nanoreviser_amd.engine import Reviser
    m1, m2 = species_models[sp]
    k1, k2 = reparam(m1, "lstm3_perm"), reparam(m2, "lstm3_perm")
    sw, fw, base = shipped["sw"], shipped["fw"], shipped[sp]
    rv = Reviser(k1, k2)
    for mode in MODES:
        rv.set_precision(mode)
        got = rv.predict_pair(sw, fw)
        res = _policy(got, base["q"], base["nf"], f"{mode} {sp} lstm3_perm")
        print(f"WEIGHTS {sp} lstm3_perm {mode}: {res}")
    assert rv.saturated() == (0, 0)
    rv.close()


@pytest.mark.parametrize("sp", SPECIES)
@pytest.mark.parametrize("name", DEGENERATE_CASES)
def test_degenerate_weights(shipped, species_models, sp, name):
    from nanoreviser_amd.engine import Reviser
    from oracle import nrv_oracle as O
    m1, m2 = species_models[sp]
    k1, k2 = degenerate(m1, name), degenerate(m2, name)
    sw, fw = shipped["sw"], shipped["fw"]
    q1, q2, _, _ = O.predict_pair(k1.tensors, k2.tensors, sw, fw, np.float64)
    nf = f32_floor(k1, k2, sw, fw, q1, q2)
    rv = Reviser(k1, k2)
    for mode in MODES:
        rv.set_precision(mode)
        got = rv.predict_pair(sw, fw)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), mode
        res = _policy(got, (q1, q2), nf, f"{mode} {sp} {name}")
        _, reruns = rv.saturated()
        print(f"WEIGHTS {sp} {name} {mode}: reruns {reruns} {res}")
        assert reruns == 0, mode
    rv.close()


def _live_oracle_every_mode(k1, k2, sw, fw, what, act="hard_sigmoid"):
    """test_degenerate_weights' shape: the case's own fp64 oracle and f32 floors, every mode, finite, the policy, no re-run."""
    from nanoreviser_amd.engine import Reviser
    from oracle import nrv_oracle as O
    with np.errstate(over="ignore"):
        q1, q2, _, _ = O.predict_pair(k1.tensors, k2.tensors, sw, fw, np.float64, recurrent_act=act)
        nf = f32_floor(k1, k2, sw, fw, q1, q2) if act == "hard_sigmoid" else f32_floor_act(k1, k2, sw, fw, q1, q2, act)
    bind = "/".join(",".join(binding(plan_terms(k)[l])[0][:3] for l in LAYERS) for k in (k1, k2))
    rv = Reviser(k1, k2, recurrent_activation=act)
    try:
        for mode in MODES:
            rv.set_precision(mode)
            got = rv.predict_pair(sw, fw)
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), f"{what} {mode}"
            res = _policy(got, (q1, q2), nf, f"{mode} {what}")
            _, reruns = rv.saturated()
            print(f"WEIGHTS {what} {act} {mode}: binds {bind} reruns {reruns} {res}")
            assert reruns == 0, f"{what} {mode}"
    finally:
        rv.close()


def _acts(sp, name):
    return ["hard_sigmoid"] + (["sigmoid"] if sp in SIGMOID_ADMITTED.get(name, ()) else [])


@pytest.mark.parametrize("sp", SPECIES)
@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan_cases(shipped, species_models, sp, name):
    """The recurrent block, or the BatchNorm block of the 192 -> 128 layer, sets the accumulator exponent."""
    m1, m2 = species_models[sp]
    k1, k2 = plan_case(m1, name), plan_case(m2, name)
    assert f16x2_must_not_rerun(k1, k2, shipped["sw"])
    for act in _acts(sp, name):
        _live_oracle_every_mode(k1, k2, shipped["sw"], shipped["fw"], f"{sp} {name}", act)


@pytest.mark.parametrize("sp,name", [(sp, name) for sp in SPECIES for name in UNSEEN_ADMITTED[sp]])
def test_unseen_weights(shipped, species_models, sp, name):
    other = "human" if sp == "ecoli" else "ecoli"
    (m1, m2), (o1, o2) = species_models[sp], species_models[other]
    k1, k2 = unseen(m1, o1, name), unseen(m2, o2, name)
    assert f16x2_must_not_rerun(k1, k2, shipped["sw"])
    for act in _acts(sp, name):
        _live_oracle_every_mode(k1, k2, shipped["sw"], shipped["fw"], f"{sp} {name}", act)


def _raw_path_gives_predict_reads_bits(reads, k1, k2):
    from nanoreviser_amd.engine import Reviser
    _, rd, _ = reads("ch141_read5436")
    rr = hs.read_tensors_raw(rd)
    N = 400
    starts = rr.starts[:N].copy()
    raw = rr.raw[: int(starts[-1]) + 60].copy()
    feat = rr.feat_ev[:N]
    rv = Reviser(k1, k2, precision="f16x2")
    got = rv.predict_reads_raw([raw], [starts], [feat], [rr.shift], [rr.scale])
    _, reruns_raw = rv.saturated()
    sig_ev = rv.segment_reads([raw], [starts], [rr.shift], [rr.scale])
    want = rv.predict_read(sig_ev, feat)
    _, reruns_both = rv.saturated()
    rv.close()
    assert got[0].shape == (N - 11, 6) and reruns_both == 2 * reruns_raw
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    return reruns_raw


def test_recurrent_block_binding_through_the_raw_read_path(reads, species_models):
    """`all_rec_bind` through nrv_predict_reads_raw: nrv_predict_read's bits on the same weights, nothing re-run."""
    m1, m2 = species_models["human"]
    assert _raw_path_gives_predict_reads_bits(reads, plan_case(m1, "all_rec_bind"), plan_case(m2, "all_rec_bind")) == 0


def test_reparametrised_weights_through_the_raw_read_path(reads, species_models):
    """`all` at 2^6 through nrv_predict_reads_raw (the slot path: its own launch sequence, the same weight plan): the first
    400 events of a fixture read give nrv_predict_read's bits on the same weights."""
    m1, m2 = species_models["human"]
    _raw_path_gives_predict_reads_bits(reads, reparam(m1, "all", 64.0), reparam(m2, "all", 64.0))
