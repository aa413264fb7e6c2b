"""Every arithmetic mode held to the f32 FLOOR, not to 1e-4 (MI355X only, -m gpu).

parity_policy.check_vs_fp64 passes a well-conditioned window at |dp| <= 1e-4; the oracle's own f32 restatements sit 1e-7 to
1e-5 from fp64 on these windows, so that bar cannot tell the product's arithmetic from one a precision class worse (an operand
of one layer carried as a single f16 term passes it: tests/test_precision_grade_host.py pins that).  Here every window's error
is divided by the f32 floor of that window (precision_cases.grade: probability and log domain) and the median and the 0.9
quantile over the window set are bounded by K = sqrt(a b): a = the worst f32-grade evaluation of the reference, b = the
weakest single-term mutant of the family that threatens the mode.  K is sized on the CPU from the reference alone and pinned
(precision_cases.K_PINNED); the host test re-derives it and shows that `_check_model` below fails on every separated mutant.

Both species, both models, the 256 fixture windows (T = 11) and the synthetic 13-event windows of the goldens, every mode;
recurrent_activation="sigmoid" on the fixture set for E. coli; the weights reparametrised at all ten sites at once (c = 2^-6,
2^3: the oracle's answer is the shipped weights' bit for bit, so are K and the floors - a plan exponent that costs bits
without overflowing shows only here).  No stage may be handed to the f32 kernels: `saturated() == (0, 0)`.  The unchanged
parity policy stays in force next to it (tests/test_gpu_parity.py, test_gpu_weight_range.py)."""
import numpy as np
import pytest

import precision_cases as PC
from weight_cases import reparam

pytestmark = pytest.mark.gpu

REPARAM_CS = (2.0 ** -6, 2.0 ** 3)
_REFERENCES = {}


def _reference(k, model, sig, rd, T, act):
    """(fp64 oracle, (probability floor, log floor)) of one model on one window set: computed once for the three modes and
    every reparametrisation, left unchanged."""
    if k not in _REFERENCES:
        ref = PC.reference(model, sig, rd, T, act)
        fl = PC.floors(model, sig, rd, T, act, ref)
        for a in (ref["p64"],) + tuple(fl):
            a.setflags(write=False)
        _REFERENCES[k] = (ref["p64"], fl)
    return _REFERENCES[k]


def _check_model(p, p64, floor, k, mode, what):
    """One model's probabilities against the CPU-derived bound of its combination.  tests/test_precision_grade_host.py calls
    this with a mutant's output in place of the engine's."""
    return PC.check_grade(p, p64, floor, PC.K_for(k, mode), what)


def _run(models, shipped, ws, sp, act, mode, reads, model_goldens, what):
    from nanoreviser_amd.engine import Reviser
    sig, rd, T = PC.window_set(ws, reads, model_goldens)
    k1, k2 = (m.with_window(T) for m in models)
    rv = Reviser(k1, k2, precision=mode, recurrent_activation=act)
    try:
        assert rv.precision == mode
        got = rv.predict_pair(sig, rd)
        assert rv.saturated() == (0, 0), f"{what}: a stage was handed to the f32 kernels"
    finally:
        rv.close()
    for no, p in ((1, got[0]), (2, got[1])):
        k = PC.key(ws, sp, no, act)
        p64, fl = _reference(k, shipped[no - 1].with_window(T), sig, rd, T, act)
        s = PC.grade_stats(p, p64, fl)
        K = PC.K_for(k, mode)
        print(f"GRADE {what} m{no} {mode}: " + " ".join(f"{n} {s[n]:.3g} (K {K[n]:.3g})" for n in PC.STATS))
    for no, p in ((1, got[0]), (2, got[1])):
        k = PC.key(ws, sp, no, act)
        _check_model(p, *_REFERENCES[k], k, mode, f"{what} m{no} {mode}")


@pytest.mark.parametrize("mode", PC.MODES)
@pytest.mark.parametrize("ws,sp,act", PC.COMBOS)
def test_precision_grade(reads, model_goldens, species_models, ws, sp, act, mode):
    ms = species_models[sp]
    _run(ms, ms, ws, sp, act, mode, reads, model_goldens, f"{ws} {sp} {act}")


@pytest.mark.parametrize("mode", PC.MODES)
@pytest.mark.parametrize("c", REPARAM_CS)
@pytest.mark.parametrize("sp", PC.SPECIES)
def test_precision_grade_reparametrised(reads, model_goldens, species_models, sp, c, mode):
    """Oracle, floors and K of the shipped weights: tests/test_weight_cases_host.py pins that the oracle does not move."""
    ms = species_models[sp]
    _run([reparam(m, "all", c) for m in ms], ms, "fixture", sp, "hard_sigmoid", mode, reads, model_goldens,
         f"fixture {sp} all@{c:g}")
