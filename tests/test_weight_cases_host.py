"""The generator of tests/weight_cases.py, pinned on the CPU so that tests/test_gpu_weight_range.py can rely on it.

Reparametrised weights: the oracle's answer on the 256 test windows is the shipped weights' answer to the last bit, in fp64
and in f32 (power-of-two scaling commutes with every operation of the graph); the permutation of lstm3's hidden units changes
the summation order of its consumers and is held to 1e-12 in fp64.  Degenerate weights: finite, and as well-conditioned for
f32 arithmetic as the shipped weights are (so that the parity policy means something on them)."""
import numpy as np
import pytest

from parity_policy import BAR, f32_floor
from weight_cases import DEGENERATE_CASES, REPARAM_CASES, case_windows, degenerate, reparam

CS = [2.0 ** -6, 2.0 ** -3, 2.0 ** 3, 2.0 ** 6]
SPECIES = ["ecoli", "human"]


@pytest.fixture(scope="module")
def shipped(reads, species_models):
    from oracle import nrv_oracle as O
    sw, fw = case_windows(reads)
    out = {}
    for sp in SPECIES:
        m1, m2 = species_models[sp]
        out[sp] = {dt: O.predict_pair(m1.tensors, m2.tensors, sw, fw, dt) for dt in (np.float64, np.float32)}
    return sw, fw, out


def test_generators_leave_the_shipped_tensors_alone(species_models):
    m1, _ = species_models["ecoli"]
    before = [t.copy() for t in m1.tensors]
    reparam(m1, "all", 64.0), reparam(m1, "lstm3_perm"), degenerate(m1, "lstm4_tiny"), degenerate(m1, "conv1_ch0")
    for a, b in zip(before, m1.tensors):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        reparam(m1, "bn_l1", 3.0)
    # every case changes something, and `all` at c = 1 nothing
    for site in REPARAM_CASES:
        assert any(not np.array_equal(a, b) for a, b in zip(before, reparam(m1, site, 8.0).tensors)), site
    for name in DEGENERATE_CASES:
        assert any(not np.array_equal(a, b) for a, b in zip(before, degenerate(m1, name).tensors)), name
    assert all(np.array_equal(a, b) for a, b in zip(before, reparam(m1, "all", 1.0).tensors))


@pytest.mark.parametrize("sp", SPECIES)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("site", [s for s in REPARAM_CASES if s != "lstm3_perm"])
def test_reparametrisation_is_exact_in_fp64_and_f32(shipped, species_models, sp, site, c):
    from oracle import nrv_oracle as O
    sw, fw, base = shipped
    m1, m2 = species_models[sp]
    k1, k2 = reparam(m1, site, c), reparam(m2, site, c)
    for dt in (np.float64, np.float32):
        got = O.predict_pair(k1.tensors, k2.tensors, sw, fw, dt)
        for g, b in zip(got, base[sp][dt]):
            assert np.array_equal(g, b), (site, c, dt)


@pytest.mark.parametrize("sp", SPECIES)
def test_lstm3_permutation_preserves_the_function(shipped, species_models, sp):
    from oracle import nrv_oracle as O
    sw, fw, base = shipped
    m1, m2 = species_models[sp]
    k1, k2 = reparam(m1, "lstm3_perm"), reparam(m2, "lstm3_perm")
    got = O.predict_pair(k1.tensors, k2.tensors, sw, fw, np.float64)
    for g, b in zip(got[:2], base[sp][np.float64][:2]):
        assert np.abs(g - b).max() <= 1e-12
    assert np.array_equal(got[2], base[sp][np.float64][2]) and np.array_equal(got[3], base[sp][np.float64][3])


@pytest.mark.parametrize("sp", SPECIES)
@pytest.mark.parametrize("name", DEGENERATE_CASES)
def test_degenerate_weights_stay_finite_and_well_conditioned(shipped, species_models, sp, name):
    from oracle import nrv_oracle as O
    sw, fw, _ = shipped
    m1, m2 = species_models[sp]
    k1, k2 = degenerate(m1, name), degenerate(m2, name)
    q1, q2, _, _ = O.predict_pair(k1.tensors, k2.tensors, sw, fw, np.float64)
    assert np.isfinite(q1).all() and np.isfinite(q2).all()
    p1, p2, _, _ = O.predict_pair(k1.tensors, k2.tensors, sw, fw, np.float32)
    assert np.isfinite(p1).all() and np.isfinite(p2).all()
    nf1, nf2 = f32_floor(k1, k2, sw, fw, q1, q2)
    assert np.isfinite(nf1).all() and np.isfinite(nf2).all()
    ill1, ill2 = int((nf1 > BAR / 2).sum()), int((nf2 > BAR / 2).sum())
    print(f"DEGENERATE {sp} {name}: ill-conditioned {ill1} / {ill2} of {len(nf1)}")
    assert ill1 <= 0.01 * len(nf1) and ill2 <= 0.01 * len(nf2)
