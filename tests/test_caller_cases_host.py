"""tests/caller_cases.py without a GPU: the arithmetic of the bands the caller-contract tests hand to the engine, and the oracle's
own f32 form on the inputs those tests add.

  1. `banded` (torch, host memory) and `banded_np`: for every array of a call, at every alignment case and n, the payload's
     address modulo 16 is what ALIGNMENTS promises (4, 8, 12 for the float inputs, 4 modulo 8 for p1 / p2, odd for a1 / a2), the
     front guard is 64 rows plus the offset and the back guard 64 rows, payload and guards tile the buffer exactly, the guards
     hold 0xA5 and the payload its fill.
  2. `fill_guards`: a byte, a float and a decoy land in the guards and nowhere else; whole decoy rows touch the payload on both
     sides; `guards_hold` sees a single changed byte on either side.
  3. The T = 32 inputs (T32_SEED): oracle/nrv_oracle.c against the fp64 arbiter under parity_policy on all 129 windows - the
     twin of tests/test_gpu_lstm4_resident.py::test_f32_oracle_holds_the_bar_on_these_inputs, which covers T = 1 and 13 - so a
     failure of the GPU file's parity test is the engine's, not the bar's.  Seed 8132 was the first one tried.
  4. The cases are what they say: shapes, the case n of read mode is a prefix, decoys differ from the inputs everywhere it
     matters, and the alignment cases cover every residue the contract names."""
import numpy as np
import pytest

import caller_cases as CC
from parity_policy import check_vs_fp64

SHAPES = {"sig": lambda n, T: (n, T, 50), "feat": lambda n, T: (n, T, 6), "p1": lambda n, T: (n, 6), "p2": lambda n, T: (n, 5),
          "a1": lambda n, T: (n,), "a2": lambda n, T: (n,)}


def _np_dtype(name):
    return np.int8 if name[0] == "a" else np.float32


def _bands(kind, name, shape, k, fill):
    off = CC.offsets(k)[name]
    if kind == "numpy":
        return CC.banded_np(shape, _np_dtype(name), off, fill)
    import torch
    return CC.banded(shape, torch.int8 if name[0] == "a" else torch.float32, off, fill, device="cpu")


@pytest.mark.parametrize("kind", ("torch", "numpy"))
@pytest.mark.parametrize("T", CC.TS)
def test_band_arithmetic(kind, T):
    for k in CC.ALIGNMENTS:
        for n in CC.NS:
            for name in CC.ARRAYS:
                shape = SHAPES[name](n, T)
                item = 1 if name[0] == "a" else 4
                fill = -7 if name[0] == "a" else 2.5
                buf, pay = _bands(kind, name, shape, k, fill)
                what = (kind, T, k, n, name)
                assert tuple(pay.shape) == shape, what
                front, back = CC.guards(buf, pay)
                row = int(np.prod(shape[1:], dtype=np.int64)) * item
                off = CC.offsets(k)[name]
                assert CC._nbytes(front) == 64 * row + off * item and CC._nbytes(back) == 64 * row, what
                assert CC._nbytes(front) + CC._nbytes(pay) + CC._nbytes(back) == CC._nbytes(buf), what
                assert CC._addr(front) == CC._addr(buf) and CC._addr(pay) == CC._addr(buf) + CC._nbytes(front), what
                assert CC._addr(back) == CC._addr(pay) + CC._nbytes(pay), what
                assert CC._addr(buf) % 64 == 0, what
                assert CC._addr(pay) % 16 == (off * item) % 16, what
                if k and item == 4 and name in ("sig", "feat"):
                    assert CC._addr(pay) % 16 == 4 * k, what
                if k and name in ("p1", "p2"):
                    assert CC._addr(pay) % 8 == 4, what
                if k and name in ("a1", "a2"):
                    assert CC._addr(pay) % 2 == 1, what
                assert CC.guards_hold(buf, pay), what
                assert bool((pay == fill).all()), what


def test_alignment_cases_cover_the_contract():
    res = {name: {(CC.offsets(k)[name] * (1 if name[0] == "a" else 4)) % 16 for k in CC.ALIGNMENTS} for name in CC.ARRAYS}
    assert res["sig"] == res["feat"] == {0, 4, 8, 12}
    assert {r % 8 for r in res["p1"]} == {r % 8 for r in res["p2"]} == {0, 4}
    assert all(any(r % 2 for r in res[a]) for a in ("a1", "a2"))
    assert all(CC.offsets(k)["a1"] != CC.offsets(k)["a2"] for k in CC.ALIGNMENTS[1:])
    assert max(max(CC.offsets(k).values()) for k in CC.ALIGNMENTS) < 64          # a guard stays 64 rows and a few elements


@pytest.mark.parametrize("kind", ("torch", "numpy"))
def test_guard_fills_land_in_the_guards_only(kind):
    T, n = 13, 33
    w = CC.inputs("window", T, n)
    shape = (n, T, 50)
    buf, pay = _bands(kind, "sig", shape, 3, w["sig"])
    as_np = (lambda x: x) if kind == "numpy" else (lambda x: x.numpy())
    for what in (float("nan"), CC.BIG, w["decoy_sig"], 0x7F):
        CC.fill_guards(buf, pay, what)
        assert np.array_equal(as_np(pay).view(np.uint32), w["sig"].view(np.uint32))            # the payload is untouched
        front, back = (as_np(g) for g in CC.guards(buf, pay))
        if isinstance(what, int):
            assert (front == what).all() and (back == what).all() and CC.guards_hold(buf, pay, what)
            continue
        f, b = front.view(np.float32), back.view(np.float32)
        if isinstance(what, float):
            want = np.float32(what).view(np.uint32)
            assert (f.view(np.uint32) == want).all() and (b.view(np.uint32) == want).all()
            assert want in (np.uint32(0x7FC00000), np.float32(3.0e38).view(np.uint32))
        else:
            row = T * 50
            assert np.array_equal(b, what.reshape(-1)[:64 * row])                                # decoy rows 0 .. 63 behind
            assert np.array_equal(f[3:], what.reshape(-1)[-64 * row:])                           # ... and its last 64 in front
            assert np.array_equal(f[-row:], what[-1].reshape(-1)) and np.array_equal(b[:row], what[0].reshape(-1))
        assert not CC.guards_hold(buf, pay)
    CC.fill_guards(buf, pay, CC.GUARD_BYTE)
    assert CC.guards_hold(buf, pay)
    for g, at in ((0, 0), (0, -1), (1, 0), (1, -1)):                                            # one byte, next to the payload or far from it
        gv = CC.guards(buf, pay)[g]
        gv[at] = 0xA4
        assert not CC.guards_hold(buf, pay), (g, at)
        gv[at] = CC.GUARD_BYTE
    assert CC.guards_hold(buf, pay)


def test_cases_are_what_they_say():
    for T in CC.TS:
        w, e = CC.windows(T), CC.events(T)
        assert w["sig"].shape == (129, T, 50) and w["feat"].shape == (129, T, 6) and w["sig"].dtype == np.float32
        assert e["sig"].shape == (129 + T, 50) and e["feat"].shape == (129 + T, 6)
        for src in (w, e):
            assert src["decoy_sig"].shape == src["sig"].shape and src["decoy_feat"].shape == src["feat"].shape
            # a decoy is another draw: no row of it equals the row it stands in for
            assert not (src["decoy_sig"].reshape(len(src["sig"]), -1) == src["sig"].reshape(len(src["sig"]), -1)).all(1).any()
            assert np.isfinite(src["decoy_sig"]).all() and np.isfinite(src["decoy_feat"]).all()
        for n in CC.NS:
            r = CC.inputs("read", T, n)
            assert r["sig"].shape == (n + T, 50) and np.array_equal(r["sig"], e["sig"][:n + T]) and r["sig"].flags.writeable
            assert r["decoy_sig"].shape[0] == 129 + T                                            # whole: it fills 64-row guards
            x = CC.inputs("window", T, n)
            assert x["feat"].shape == (n, T, 6) and np.array_equal(x["feat"], w["feat"][:n])
    assert CC.case_seed(1) == 8101 and CC.case_seed(13) == 8113 and CC.case_seed(32) == CC.T32_SEED   # the cases of test_gpu_lstm4_resident.py


def test_f32_oracle_holds_the_bar_at_T32(species_models):
    T = 32
    ref = CC.reference(species_models, T)
    assert ref["q"][0].shape == (129, 6) and ref["q"][1].shape == (129, 5)
    for m in range(2):
        p, a = ref["c"][m]
        seen = check_vs_fp64(p, a, ref["q"][m], ref["nf"][m], f"C oracle ecoli T={T} m{m + 1}")
        print(f"T={T} m{m + 1}", seen)
        srt = np.sort(ref["q"][m], -1)
        decided = srt[:, -1] - srt[:, -2] > 1e-4
        assert np.array_equal(np.asarray(a)[decided], ref["q"][m].argmax(-1)[decided])
