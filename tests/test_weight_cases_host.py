"""The generator of tests/weight_cases.py, pinned on the CPU so that tests/test_gpu_weight_range.py can rely on it.

Reparametrised weights: the oracle's answer on the 256 test windows is the shipped weights' answer to the last bit, in fp64
and in f32 (power-of-two scaling commutes with every operation of the graph); the permutation of lstm3's hidden units changes
the summation order of its consumers and is held to 1e-12 in fp64.  Degenerate weights: finite, and as well-conditioned for
f32 arithmetic as the shipped weights are (so that the parity policy means something on them).

The plan cases and the unseen weights: plan_terms (the CPU mirror of the f16x2 exponent plan) shows the branch each case claims to
reach; the reference ALONE has 0 of the 256 windows above the f32 floor of BAR / 2 for every admitted (case, species), so that
the GPU policy's 1 % is left for the machine it runs on; the preconditions of `reruns == 0` hold."""
import numpy as np
import pytest

from parity_policy import BAR, f32_floor
from weight_cases import (DEGENERATE_CASES, LAYERS, PLAN_BINDING, PLAN_CASES, REC_GAP, REPARAM_CASES, SHIPPED_BINDING,
                          SIGMOID_ADMITTED, UNSEEN_ADMITTED, binding, case_windows, degenerate, extreme_windows,
                          f16x2_must_not_rerun, f32_floor_act, plan_case, plan_terms, reparam, unseen)

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


# ---- the f16x2 exponent plan: which term binds ------------------------------------------------------------------------------
OTHER = {"ecoli": "human", "human": "ecoli"}


def test_shipped_models_binding_terms(species_models):
    """The same term binds in all four shipped models: the input block in the 32->64 layer (U 4-5 binades away), the signal
    block (buffer exponent 6) in the 192->128 layer, the input block in the 256->64 layer (U 2-3 binades away); the
    recurrent term binds nowhere.  A later weight file that changes this says so here."""
    for sp in SPECIES:
        for m in species_models[sp]:
            t = plan_terms(m)
            assert {l: binding(t[l])[0] for l in LAYERS} == SHIPPED_BINDING, (sp, m.source, t)
            assert t["lstm2"]["recurrent"] - t["lstm2"]["E"] in (4, 5), (sp, m.source, t["lstm2"])
            assert t["lstm4"]["recurrent"] - t["lstm4"]["E"] in (2, 3), (sp, m.source, t["lstm4"])
            assert t["lstm3"]["recurrent"] - t["lstm3"]["E"] >= 6 and t["lstm2"]["signal"] is None and t["lstm4"]["signal"] is None
    # the mirror itself, on weights whose plan can be read off: unit BatchNorm, |W| = 1 / 4, |U| = 2, signal rows 2^-3
    m = species_models["ecoli"][0]
    ts = [np.zeros_like(t) for t in m.tensors]
    for b in (18, 28, 40):
        ts[b][...] = 1
        ts[b + 3][...] = 1 - 1e-3
    for b in (22, 25, 34, 37, 44, 47):
        ts[b][...] = 0.25
        ts[b + 1][...] = 2.0
    ts[34][128:] = 0.125
    ts[37][128:] = 0.125
    ts[50][...], ts[52][...], ts[54][...] = 0.5, 1.0, 3.0
    t = plan_terms(type(m)(ts, m.T, m.n_class))
    assert t["bn"] == (13, 13, 13)                                 # bound 1 = 0.5 x 2^1
    assert t["lstm2"] == {"input": 13 + 15, "signal": None, "recurrent": 13 + 12, "E": 25}
    assert t["lstm3"] == {"input": 13 + 15, "signal": 6 + 16, "recurrent": 13 + 12, "E": 22}
    assert t["lstm4"] == {"input": 13 + 15, "signal": None, "recurrent": 13 + 12, "E": 25}
    assert t["head"] == {"u1": 14, "u2": 13, "u3": 12, "s1": 14 - 7, "s2": 14 - 14}   # bounds 64 and 128 x 64


def test_plan_cases_reach_the_branch_they_claim(species_models):
    for sp in SPECIES:
        for m in species_models[sp]:
            base = plan_terms(m)
            for name in PLAN_CASES:
                t = plan_terms(plan_case(m, name))
                for l in LAYERS:
                    term, gap = binding(t[l])
                    assert term == PLAN_BINDING[name].get(l, SHIPPED_BINDING[l]), (sp, m.source, name, l, t[l])
                    if term == "recurrent":
                        assert gap >= REC_GAP, (sp, m.source, name, l, t[l])
                    if l not in PLAN_BINDING[name]:
                        assert t[l] == base[l]
                assert t["head"] == base["head"] and t["bn"] == base["bn"]
    # the shifts are the smallest: one binade less on any block misses the gap in at least one shipped model
    for name in ("lstm2_rec_binds", "lstm3_rec_binds", "lstm4_rec_binds"):
        for k, (layer, rows, shift) in enumerate(PLAN_CASES[name]):
            missed = False
            for sp in SPECIES:
                for m in species_models[sp]:
                    k1 = plan_case(m, name)
                    for d in range(2):
                        i = {"lstm2": 22, "lstm3": 34, "lstm4": 44}[layer] + 3 * d
                        k1.tensors[i][rows] *= np.float32(2.0)
                    term, gap = binding(plan_terms(k1)[layer])
                    missed |= term != "recurrent" or gap < REC_GAP
            assert missed, (name, k)


def _reference_alone(k1, k2, sw, fw, act="hard_sigmoid"):
    from oracle import nrv_oracle as O
    with np.errstate(over="ignore"):
        q1, q2, _, _ = O.predict_pair(k1.tensors, k2.tensors, sw, fw, np.float64, recurrent_act=act)
        p1, p2, _, _ = O.predict_pair(k1.tensors, k2.tensors, sw, fw, np.float32, recurrent_act=act)
        nf1, nf2 = f32_floor(k1, k2, sw, fw, q1, q2) if act == "hard_sigmoid" else f32_floor_act(k1, k2, sw, fw, q1, q2, act)
    for a in (q1, q2, p1, p2, nf1, nf2):
        assert np.isfinite(a).all()
    return int((nf1 > BAR / 2).sum()), int((nf2 > BAR / 2).sum()), float(max(nf1.max(), nf2.max()))


@pytest.mark.parametrize("sp", SPECIES)
@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan_cases_are_admissible(shipped, species_models, sp, name):
    sw, fw, _ = shipped
    m1, m2 = species_models[sp]
    k1, k2 = plan_case(m1, name), plan_case(m2, name)
    assert any(not np.array_equal(a, b) for a, b in zip(m1.tensors, k1.tensors))
    acts = ["hard_sigmoid"] + (["sigmoid"] if sp in SIGMOID_ADMITTED.get(name, ()) else [])
    for act in acts:
        ill1, ill2, top = _reference_alone(k1, k2, sw, fw, act)
        print(f"PLAN {sp} {name} {act}: ill-conditioned {ill1} / {ill2} of {len(sw)}, largest f32 floor {top:.2e}")
        assert (ill1, ill2) == (0, 0)
    assert f16x2_must_not_rerun(k1, k2, sw)


@pytest.mark.parametrize("sp,name", [(sp, name) for sp in SPECIES for name in UNSEEN_ADMITTED[sp]])
def test_unseen_weights_are_admissible(shipped, species_models, sp, name):
    sw, fw, _ = shipped
    (m1, m2), (o1, o2) = species_models[sp], species_models[OTHER[sp]]
    before = [t.copy() for t in m1.tensors + o1.tensors]
    k1, k2 = unseen(m1, o1, name), unseen(m2, o2, name)
    for a, b in zip(before, m1.tensors + o1.tensors):
        assert np.array_equal(a, b)                                # the generator leaves the shipped tensors alone
    for m, k in ((m1, k1), (m2, k2)):
        assert any(not np.array_equal(a, b) for a, b in zip(m.tensors, k.tensors))
        again = unseen(m, o1 if m is m1 else o2, name)
        assert all(np.array_equal(a, b) for a, b in zip(again.tensors, k.tensors))       # seeded
    acts = ["hard_sigmoid"] + (["sigmoid"] if sp in SIGMOID_ADMITTED.get(name, ()) else [])
    for act in acts:
        ill1, ill2, top = _reference_alone(k1, k2, sw, fw, act)
        print(f"UNSEEN {sp} {name} {act}: ill-conditioned {ill1} / {ill2} of {len(sw)}, largest f32 floor {top:.2e}")
        assert (ill1, ill2) == (0, 0)
    assert f16x2_must_not_rerun(k1, k2, sw)


def test_unseen_weights_move_the_plan_as_claimed(species_models):
    for sp in SPECIES:
        for m, o in zip(species_models[sp], species_models[OTHER[sp]]):
            base = plan_terms(m)
            t = plan_terms(unseen(m, o, "outlier"))
            assert binding(t["lstm3"])[0] == "input", (sp, t["lstm3"])
            # x 32 on the largest weight of a block costs it 5 binades; E follows as far as that block ends up binding
            assert base["lstm2"]["E"] - t["lstm2"]["E"] == 5 and base["lstm4"]["E"] - t["lstm4"]["E"] in (3, 4, 5), (sp, base, t)
            assert base["lstm3"]["E"] - t["lstm3"]["E"] in (1, 2, 3, 4, 5), (sp, base, t)
            t = plan_terms(unseen(m, o, "bn_shift"))
            moved = [a - b for a, b in zip(base["bn"], t["bn"])]
            assert all(d in (1, 2, 3) for d in moved) and max(moved) >= 2, (sp, base["bn"], t["bn"])
            t = plan_terms(unseen(m, o, "random_init"))
            assert [binding(t[l])[0] for l in LAYERS] == ["recurrent", "signal", "recurrent"], (sp, t)
            assert t["head"] == {"u1": 16, "u2": 16, "u3": 15, "s1": 10, "s2": 6} and t["bn"] == (14, 14, 14), (sp, t)
            t, to = plan_terms(unseen(m, o, "hybrid_lstm3")), plan_terms(o)
            assert all(t["lstm3"][k] == to["lstm3"][k] for k in ("signal", "recurrent")) and t["bn"] == base["bn"][:2] + to["bn"][2:]
    a = unseen(species_models["ecoli"][0], species_models["human"][0], "mean_species")
    b = unseen(species_models["human"][0], species_models["ecoli"][0], "mean_species")
    assert all(np.array_equal(x, y) for x, y in zip(a.tensors, b.tensors))                # one model: the GPU test runs it once


@pytest.mark.parametrize("act", ["hard_sigmoid", "sigmoid"])
@pytest.mark.parametrize("sp", SPECIES)
def test_extreme_windows_reference_alone(species_models, sp, act):
    """tests/test_gpu_parity.py holds these 256 windows to the fp64 oracle with max_ill = 0.01 (two windows) and asserts that
    no stage is re-run: the reference alone shows at most ONE ill-conditioned window per model here, and every sample and
    every |S| fits the fixed scales of the f16x2 signal branch."""
    sig, rd = extreme_windows()
    m1, m2 = species_models[sp]
    ill1, ill2, top = _reference_alone(m1, m2, sig, rd, act)
    print(f"EXTREME {sp} {act}: ill-conditioned {ill1} / {ill2} of {len(sig)}, largest f32 floor {top:.2e}")
    assert ill1 <= 1 and ill2 <= 1
    assert f16x2_must_not_rerun(m1, m2, sig)


@pytest.mark.parametrize("sp", SPECIES)
def test_sigmoid_windows_reference_alone(reads, species_models, sp):
    """The 200 windows of tests/test_gpu_parity.py's sigmoid test: at most one ill-conditioned window of the two that 1 % allows."""
    from nanoreviser_amd import hoststage as hs
    _, _, rt = reads("ch117_read6465")
    sw, fw = hs.sliding_windows(rt.sig_ev, rt.feat_ev, 11)
    sw, fw = np.ascontiguousarray(sw[:200]), np.ascontiguousarray(fw[:200])
    m1, m2 = species_models[sp]
    ill1, ill2, top = _reference_alone(m1, m2, sw, fw, "sigmoid")
    print(f"SIGMOID {sp}: ill-conditioned {ill1} / {ill2} of {len(sw)}, largest f32 floor {top:.2e}")
    assert ill1 <= 1 and ill2 <= 1
