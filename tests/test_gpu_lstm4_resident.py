"""lstm4_r_kernel (nrv_lstm4_r.h): the 256->64 Bi-LSTM of the f16x2 mode, one wave per SIMD, with its recurrent and its last input
weight k-blocks resident in registers, the first input blocks in LDS and the rest streamed through a ring.

Everything runs in f16x2 mode through the public entry points, at the shapes where this kernel can go wrong: a workgroup is 64
rows = two 32-row tiles, so n = 1, 31, 32, 33, 63, 64, 65, 129 windows hold a single row, a ragged and a full tile, a second
tile holding one row, a ragged and a full workgroup, and the first row of a second and of a third workgroup; T = 1 has no
recurrent phase (in(0) and the peeled last step only), T = 2 one recurrent step (the resident recurrent blocks are used exactly
once, one image of the double buffer), T = 3 both images, T = 13 is the shipped window.

  * parity with the fp64 oracle under the policy and the bar of tests/test_gpu_parity.py (parity_policy, imported), calls equal
    wherever the oracle's top-two margin exceeds that bar; the oracle's own f32 restatement (oracle/nrv_oracle.c) is held to
    the same bar on the same inputs, without a GPU;
  * grouping invariance, bit for bit: 129 windows in one launch group against groups of 64 and 32, and a 142-event read in
    read mode against window mode on the windows cut from it;
  * a poisoned workspace (NRV_POISON, the switch tests/test_gpu_poison.py uses) changes no bit at n = 33 and n = 129.
"""
import numpy as np
import pytest

from nanoreviser_amd import hoststage as hs
from parity_policy import BAR, check_vs_fp64, f32_floor

NS = (1, 31, 32, 33, 63, 64, 65, 129)
TS = (1, 2, 3, 13)
SPECIES = ("ecoli", "human")
POISON = 0xC4BB8000          # -1500.0f: finite, so no clamp, ReLU or v_med3 swallows it; as f16 halves 0xC4BB / 0x8000

_CACHE = {}


def _case(species_models, sp, T):
    """Inputs and references of (species, T), computed once: 129 windows (windows are independent: the first n of them are
    the case n), the fp64 arbiter, the f32 floor of the oracle's own f32 forms and the C port's probabilities."""
    key = (sp, T)
    if key not in _CACHE:
        from oracle import c_oracle as CO
        from oracle import nrv_oracle as O
        m1, m2 = (m.with_window(T) for m in species_models[sp])
        sig, rd = O.synth_windows(max(NS), T, seed=8100 + 16 * SPECIES.index(sp) + T)
        q1, q2, _, _ = O.predict_pair(m1.tensors, m2.tensors, sig, rd, np.float64)
        nf1, nf2 = f32_floor(m1, m2, sig, rd, q1, q2, T)
        c1, a1 = CO.predict(m1.flat(), T, 6, sig, rd, threads=8)
        c2, a2 = CO.predict(m2.flat(), T, 5, sig, rd, threads=8)
        _CACHE[key] = dict(m1=m1, m2=m2, sig=sig, rd=rd, q=(q1, q2), nf=(nf1, nf2), c=((c1, a1), (c2, a2)))
    return _CACHE[key]


def _calls_equal_where_decided(a, p64, what):
    srt = np.sort(p64, -1)
    decided = srt[:, -1] - srt[:, -2] > BAR
    assert np.array_equal(np.asarray(a)[decided], p64.argmax(-1)[decided]), what


def _engine(monkeypatch, m1, m2, poison=None, batch=4096):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_COALESCE", "NRV_LANES", "NRV_PRECISION", "NRV_POISON"):
        monkeypatch.delenv(k, raising=False)
    if poison is not None:
        monkeypatch.setenv("NRV_POISON", f"{poison:08x}")
    rv = Reviser(m1, m2, batch=batch, precision="f16x2")
    monkeypatch.delenv("NRV_POISON", raising=False)
    assert rv.backend == "hip" and rv.precision == "f16x2"
    return rv


def _same_bits(x, y, what):
    for i, (a, b) in enumerate(zip(x, y)):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, i)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("sp", SPECIES)
def test_f32_oracle_holds_the_bar_on_these_inputs(species_models, sp, T):
    """No GPU: oracle/nrv_oracle.c (f32) against oracle/nrv_oracle.py (fp64) on the inputs of the parity test, under the same
    policy - so a failure of the parity test is the engine's, not the bar's."""
    cs = _case(species_models, sp, T)
    for m in range(2):
        p, a = cs["c"][m]
        check_vs_fp64(p, a, cs["q"][m], cs["nf"][m], f"C oracle {sp} T={T} m{m + 1}")
        _calls_equal_where_decided(a, cs["q"][m], f"C oracle {sp} T={T} m{m + 1}")


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("sp", SPECIES)
def test_parity_at_tile_and_workgroup_edges(species_models, sp, T, monkeypatch):
    cs = _case(species_models, sp, T)
    rv = _engine(monkeypatch, cs["m1"], cs["m2"])
    for n in NS:
        out = rv.predict_pair(np.ascontiguousarray(cs["sig"][:n]), np.ascontiguousarray(cs["rd"][:n]))
        for m in range(2):
            what = f"{sp} T={T} n={n} m{m + 1}"
            seen = check_vs_fp64(out[m], out[2 + m], cs["q"][m][:n], cs["nf"][m][:n], what, max_ill=1.0)
            print(what, seen)
            _calls_equal_where_decided(out[2 + m], cs["q"][m][:n], what)
    for m in range(2):          # the share of ill-conditioned windows is a property of the inputs: asserted on all 129
        check_vs_fp64(out[m], out[2 + m], cs["q"][m], cs["nf"][m], f"{sp} T={T} m{m + 1}")
    assert rv.saturated() == (0, 0)              # the f16x2 kernels computed this: no f32 re-run by the range guard
    rv.close()


@pytest.mark.gpu
def test_grouping_is_invisible_bit_for_bit(species_models, monkeypatch):
    import torch
    T = 13
    cs = _case(species_models, "ecoli", T)
    n = max(NS)
    rv = _engine(monkeypatch, cs["m1"], cs["m2"])
    ref = rv.predict_pair(cs["sig"], cs["rd"])
    for batch in (64, 32):
        rv.set_batch(batch)
        _same_bits(ref, rv.predict_pair(cs["sig"], cs["rd"]), f"batch {batch}")
    rv.set_batch(4096)
    # a 142-event read: read mode on the device against window mode on its 129 windows
    from oracle import nrv_oracle as O
    s, f = O.synth_windows(n + T, 1, seed=8313)
    sig_ev, feat_ev = np.ascontiguousarray(s[:, 0]), np.ascontiguousarray(f[:, 0])
    sw, fw = hs.sliding_windows(sig_ev, feat_ev, T)
    win = rv.predict_pair(np.array(sw, order="C"), np.array(fw, order="C"))
    d_sig, d_feat = torch.from_numpy(sig_ev).cuda(), torch.from_numpy(feat_ev).cuda()
    r = (torch.full((n, 6), float("nan"), device="cuda"), torch.full((n, 5), float("nan"), device="cuda"),
         torch.full((n,), -7, dtype=torch.int8, device="cuda"), torch.full((n,), -7, dtype=torch.int8, device="cuda"))
    torch.cuda.synchronize()
    rv.predict_read_device(d_sig.data_ptr(), d_feat.data_ptr(), n + T, *[x.data_ptr() for x in r])
    rv.sync()
    torch.cuda.synchronize()
    _same_bits(win, [x.cpu().numpy() for x in r], "read mode")
    assert rv.saturated() == (0, 0)
    rv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T", (1, 13))
def test_poisoned_workspace_changes_no_bit(species_models, T, monkeypatch):
    cs = _case(species_models, "ecoli", T)
    clean = _engine(monkeypatch, cs["m1"], cs["m2"])
    dirty = _engine(monkeypatch, cs["m1"], cs["m2"], poison=POISON)
    for n in (33, 129):
        sig, rd = np.ascontiguousarray(cs["sig"][:n]), np.ascontiguousarray(cs["rd"][:n])
        ref = clean.predict_pair(sig, rd)
        assert not np.isnan(ref[0]).any() and not np.isnan(ref[1]).any()
        for p in range(2):                       # the second call finds the first call's leftovers, then the pattern again
            _same_bits(ref, dirty.predict_pair(sig, rd), f"T={T} n={n} pass {p}")
    assert clean.saturated() == (0, 0) and dirty.saturated() == (0, 0)
    clean.close(); dirty.close()
