"""No result may depend on memory that no kernel of its own launch group wrote (MI355X only, -m gpu).

The engine's debug switch NRV_POISON=<32-bit hex> (nrv_api.hip, read per handle by nrv_create) fills every workspace, staging
and output buffer the engine allocates with that pattern instead of zeros; it fills a launch group's activation set (S, X1, X2,
X3, MO: the handle's, or the stream lane's) again before the group runs, and the staging and output buffers of the host-pointer
and raw-read entry points (d_sig / d_feat, d_raw / d_starts / d_reads, the raw slots' d_in / d_out, d_out[st]) before each
upload or stage.  Weights and range-guard counters keep their meaning.  A kernel that reads a word nobody of its group wrote -
a recurrent state before the first step, a padding tap, the tail rows of a ragged 32-row tile, an f16 split plane, a staging
row past the upload - then reads the pattern, not a zero or the previous group's valid data.

What is asserted, in every arithmetic mode, for every entry point (nrv_predict / nrv_predict_read with host arrays pre-filled
with NaN / -7 sentinels, the device-pointer forms, nrv_predict_reads_raw, two nrv_reads_raw_begin / _end calls in flight,
nrv_segment_reads), every launch-group form (coalesced; NRV_COALESCE=0 on one stream; on stream lanes; NRV_LANES=0) and
ragged sizes (1, 31, 33, 4095, 4097, 10 037 windows; read-mode calls whose last tile holds 1 or 31 rows; T = 1, 11, 32):

  * the clean run agrees with the fp64 oracle (parity_policy.check_vs_fp64) on a slice that holds a 1-row last tile, and read
    mode, raw reads and device segmentation agree bit for bit with window mode / the host-cut windows;
  * under three patterns - a quiet NaN, FLT_MAX, and -1500.0f (finite: ReLU, v_med3 and the clamps swallow a NaN but not it),
    each also nasty as a pair of f16 / bf16 halves - every output is bit-identical to the clean run, on a first and a second
    call of the same handle;
  * f16x2 mode: the range guard never fires on these in-range inputs (a spurious f32 re-run would change bits).

test_round6_configuration_poisoned reruns the configuration of round 6's one unexplained mismatch (bf16x3, NRV_COALESCE=0,
batch 1000, one stream) under each pattern.  test_results_do_not_depend_on_stale_device_memory, the older test, poisons the
driver's free memory instead: it still covers the staging the engine does not fill itself when the switch is off."""
import ctypes as C

import numpy as np
import pytest

from nanoreviser_amd import hoststage as hs

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "bf16x3", "f32"]
PATTERNS = {"qnan": 0x7FC00000, "fltmax": 0x7F7FFFFF, "m1500": 0xC4BB8000}
# name -> (batch, NRV_COALESCE, NRV_LANES)
GROUPINGS = {"coalesced": (1000, None, None), "one_stream": (1000, "0", None), "lanes512": (512, "0", None),
             "lanes992": (992, "0", None), "no_lanes": (512, "0", "0")}
WINDOWS = (1, 31, 33, 4095, 4097, 10_037)
FP, I8 = C.POINTER(C.c_float), C.POINTER(C.c_int8)


def _engine(monkeypatch, m1, m2, mode, grouping, poison):
    from nanoreviser_amd.engine import Reviser
    batch, coalesce, lanes = GROUPINGS[grouping]
    for k, v in (("NRV_COALESCE", coalesce), ("NRV_LANES", lanes),
                 ("NRV_POISON", None if poison is None else f"{PATTERNS[poison]:08x}")):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    monkeypatch.delenv("NRV_PRECISION", raising=False)
    rv = Reviser(m1, m2, batch=batch, precision=mode)
    for k in ("NRV_COALESCE", "NRV_LANES", "NRV_POISON"):
        monkeypatch.delenv(k, raising=False)
    return rv


def _sentinels(k):
    return (np.full((k, 6), np.nan, np.float32), np.full((k, 5), np.nan, np.float32),
            np.full(k, -7, np.int8), np.full(k, -7, np.int8))


def _ptrs(out):
    return out[0].ctypes.data_as(FP), out[1].ctypes.data_as(FP), out[2].ctypes.data_as(I8), out[3].ctypes.data_as(I8)


def _raw_read(rng, n_ev, shift, scale):
    """A synthetic read: int16 samples around `shift`, event starts 4..14 samples apart (the last ones may lie past the end)."""
    starts = np.cumsum(rng.integers(4, 15, n_ev)).astype(np.int32) - 4
    raw = np.clip(rng.normal(shift, 1.2 * scale, int(starts[-1]) + 8 if n_ev else 0), -32768, 32767).astype(np.int16)
    return raw, starts


class Inputs:
    """Everything one pass over the entry points needs at window length T (seeded, host and device copies)."""

    def __init__(self, T, windows, seed):
        import torch
        from oracle import nrv_oracle as O
        self.T = T
        self.windows = windows
        N = max(windows) + T
        s, f = O.synth_windows(N, 1, seed=seed)
        self.sig_ev, self.feat_ev = np.ascontiguousarray(s[:, 0]), np.ascontiguousarray(f[:, 0])
        sw, fw = hs.sliding_windows(self.sig_ev, self.feat_ev, T)
        self.sw, self.fw = np.array(sw, order="C"), np.array(fw, order="C")     # copies: writable, contiguous
        self.d_sw, self.d_fw = torch.from_numpy(self.sw).cuda(), torch.from_numpy(self.fw).cuda()
        self.d_sig_ev, self.d_feat_ev = torch.from_numpy(self.sig_ev).cuda(), torch.from_numpy(self.feat_ev).cuda()
        rng = np.random.default_rng(seed)
        # raw calls: A = two reads whose windows leave a 1-row last tile (4097 windows), B = one read, a 31-row last tile
        self.raw = []
        for evs in ((2000, 2097 + T), (31 + T,)):
            raws, starts, feats, shifts, scales = [], [], [], [], []
            for n_ev in evs:
                sh, sc = float(rng.uniform(300, 600)), float(rng.uniform(40, 90))
                r, st = _raw_read(rng, n_ev, sh, sc)
                raws.append(r); starts.append(st); shifts.append(sh); scales.append(sc)
                feats.append(O.synth_windows(n_ev, 1, seed=int(rng.integers(1 << 30)))[1][:, 0])
            self.raw.append((raws, starts, feats, shifts, scales))

    def run(self, rv):
        """One pass over every entry point -> list of (name, array)."""
        import torch
        T, lib, h, out = self.T, rv._lib, rv._h, []
        for n in self.windows:                                      # host pointers, window and read mode
            o = _sentinels(n)
            rv._check(lib.nrv_predict(h, self.sw[:n].ctypes.data_as(FP), self.fw[:n].ctypes.data_as(FP), n, *_ptrs(o)))
            out += [(f"predict n={n} {i}", x) for i, x in enumerate(o)]
            o = _sentinels(n)
            rv._check(lib.nrv_predict_read(h, self.sig_ev.ctypes.data_as(FP), self.feat_ev.ctypes.data_as(FP), n + T, *_ptrs(o)))
            out += [(f"predict_read n={n} {i}", x) for i, x in enumerate(o)]
        for n in self.windows:                                      # device pointers
            w = (torch.full((n, 6), float("nan"), device="cuda"), torch.full((n, 5), float("nan"), device="cuda"),
                 torch.full((n,), -7, dtype=torch.int8, device="cuda"), torch.full((n,), -7, dtype=torch.int8, device="cuda"))
            r = tuple(torch.full_like(x, float("nan") if x.dtype == torch.float32 else -7) for x in w)
            torch.cuda.synchronize()
            rv.predict_device(self.d_sw.data_ptr(), self.d_fw.data_ptr(), n, *[x.data_ptr() for x in w])
            rv.predict_read_device(self.d_sig_ev.data_ptr(), self.d_feat_ev.data_ptr(), n + T, *[x.data_ptr() for x in r])
            rv.sync()
            torch.cuda.synchronize()
            out += [(f"predict_device n={n} {i}", x.cpu().numpy()) for i, x in enumerate(w)]
            out += [(f"predict_read_device n={n} {i}", x.cpu().numpy()) for i, x in enumerate(r)]
        packs = []
        for k, (raws, starts, feats, shifts, scales) in enumerate(self.raw):
            p = rv.pack_reads_raw(raws, starts, feats, shifts, scales, T)
            p = p[:6] + (_sentinels(p[6][0].shape[0]),)
            out += [(f"reads_raw {k} {i}", x) for i, x in enumerate(rv.run_packed_raw(p))]
            out.append((f"segment_reads {k}", rv.segment_reads(raws, starts, shifts, scales)))
            packs.append(rv.pack_reads_raw(raws, starts, feats, shifts, scales, T))
        packs = [p[:6] + (_sentinels(p[6][0].shape[0]),) for p in packs]
        tickets = [rv.begin_packed_raw(p) for p in packs]            # two calls in flight
        for k, t in enumerate(tickets):
            out += [(f"raw_begin_end {k} {i}", x) for i, x in enumerate(rv.end_packed_raw(t))]
        return out


def _same_bits(ref, got, what):
    assert [k for k, _ in ref] == [k for k, _ in got]
    for (k, x), (_, y) in zip(ref, got):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        if not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            bad = np.nonzero((x.reshape(len(x), -1).view(np.uint8) != y.reshape(len(y), -1).view(np.uint8)).any(1))[0]
            pytest.fail(f"{what}: {k}: {bad.size} of {len(x)} rows differ, first {bad[:8].tolist()}, last {bad[-4:].tolist()}; "
                        f"clean {x[bad[:2]].tolist()} got {y[bad[:2]].tolist()}")


def _check_clean(inp, ref, m1, m2, mode):
    """The clean pass: no sentinel survives; read mode / raw reads / segmentation agree with window mode / the host stage;
    a slice holding the 1-row last tile of the 4097-window call (and window 0) meets the fp64 policy."""
    from oracle import nrv_oracle as O
    from parity_policy import check_vs_fp64, f32_floor
    d = dict(ref)
    T = inp.T
    for k, x in ref:
        if x.dtype == np.float32:
            assert not np.isnan(x).any(), k
        else:
            assert (x != -7).all(), k
    for n in inp.windows:
        for i in range(4):
            for other in ("predict_read", "predict_device", "predict_read_device"):
                assert np.array_equal(d[f"predict n={n} {i}"].view(np.uint8), d[f"{other} n={n} {i}"].view(np.uint8)), (mode, T, n, other, i)
    for k, (raws, starts, feats, shifts, scales) in enumerate(inp.raw):
        want = np.concatenate([hs.segment_windows_f32(r, s, sh, sc) for r, s, sh, sc in zip(raws, starts, shifts, scales)])
        assert np.array_equal(d[f"segment_reads {k}"].view(np.uint32), want.view(np.uint32)), (mode, T, k)
        for i in range(4):
            assert np.array_equal(d[f"reads_raw {k} {i}"].view(np.uint8), d[f"raw_begin_end {k} {i}"].view(np.uint8)), (mode, T, k, i)
    n = max(w for w in inp.windows if w <= 4097)
    idx = np.r_[0, max(0, n - 33):n]
    sig, rd = inp.sw[idx], inp.fw[idx]
    q1, q2, _, _ = O.predict_pair(m1.tensors, m2.tensors, sig, rd, np.float64)
    nf1, nf2 = f32_floor(m1, m2, sig, rd, q1, q2, T)
    check_vs_fp64(d[f"predict n={n} 0"][idx], d[f"predict n={n} 2"][idx], q1, nf1, f"{mode} T={T} m1")
    check_vs_fp64(d[f"predict n={n} 1"][idx], d[f"predict n={n} 3"][idx], q2, nf2, f"{mode} T={T} m2")
    # raw reads = the oracle on the windows of the device-cut (= host-cut) signal: a slice of call A across its read boundary
    raws, starts, feats, shifts, scales = inp.raw[0]
    sig_ev = np.concatenate([hs.segment_windows_f32(r, s, sh, sc) for r, s, sh, sc in zip(raws, starts, shifts, scales)])
    sw, fw = hs.sliding_windows(sig_ev, np.concatenate(feats).astype(np.float32), T)
    j = np.r_[len(starts[0]) - T - 2:len(starts[0]) + 2, len(sw) - 1]
    q1, q2, _, _ = O.predict_pair(m1.tensors, m2.tensors, np.ascontiguousarray(sw[j]), np.ascontiguousarray(fw[j]), np.float64)
    nf1, nf2 = f32_floor(m1, m2, np.ascontiguousarray(sw[j]), np.ascontiguousarray(fw[j]), q1, q2, T)
    check_vs_fp64(d["reads_raw 0 0"][j], d["reads_raw 0 2"][j], q1, nf1, f"{mode} T={T} raw m1")
    check_vs_fp64(d["reads_raw 0 1"][j], d["reads_raw 0 3"][j], q2, nf2, f"{mode} T={T} raw m2")


def _no_guard(rv, mode, what):
    pending, reruns = rv.saturated()
    if mode == "f16x2":
        assert pending == 0 and reruns == 0, (what, pending, reruns)


def _poison_sweep(monkeypatch, m1, m2, mode, inp, groupings, passes_by_grouping):
    clean = _engine(monkeypatch, m1, m2, mode, "coalesced", None)
    ref = inp.run(clean)
    _no_guard(clean, mode, "clean")
    clean.close()
    _check_clean(inp, ref, m1, m2, mode)
    for grouping in groupings:
        for poison in (None,) + tuple(PATTERNS):
            rv = _engine(monkeypatch, m1, m2, mode, grouping, poison)
            for p in range(passes_by_grouping(grouping, poison)):
                _same_bits(ref, inp.run(rv), f"{mode} T={inp.T} {grouping} poison={poison} pass {p}")
            _no_guard(rv, mode, (grouping, poison))
            rv.close()


@pytest.mark.parametrize("mode", MODES)
def test_entry_points_poisoned_workspace_bit_identical(species_models, mode, monkeypatch):
    """T = 11, every grouping, every pattern; the poisoned handles of the one-stream and lane groupings run the whole pass
    twice (the second call finds the first call's leftovers, then the pattern again)."""
    m1, m2 = species_models["ecoli"]
    inp = Inputs(11, WINDOWS, seed=2611)
    _poison_sweep(monkeypatch, m1, m2, mode, inp, list(GROUPINGS),
                  lambda g, p: 2 if p is not None and g in ("one_stream", "lanes512") else 1)


@pytest.mark.parametrize("T", [1, 32])
@pytest.mark.parametrize("mode", MODES)
def test_entry_points_poisoned_workspace_other_T(species_models, mode, T, monkeypatch):
    """The step-loop edges: T = 1 (no recurrent product) and T = 32 (the largest buffers), ragged sizes, coalesced and lanes."""
    m1, m2 = (m.with_window(T) for m in species_models["ecoli"])
    inp = Inputs(T, (1, 33, 4097), seed=2600 + T)
    _poison_sweep(monkeypatch, m1, m2, mode, inp, ["coalesced", "lanes512"], lambda g, p: 1)


def _round6_inputs():
    import torch
    T, n, N = 11, 10_037, 30_011
    g = torch.Generator(device="cuda").manual_seed(77)
    sig = (torch.randn(n, T, 50, device="cuda", generator=g) * 1.36 - 0.10).clamp_(-8.4, 4.8)
    feat = torch.rand(n, T, 6, device="cuda", generator=g)
    sig_ev = (torch.randn(N, 50, device="cuda", generator=g) * 1.36 - 0.10).clamp_(-8.4, 4.8)
    feat_ev = torch.rand(N, 6, device="cuda", generator=g)
    return T, n, N, sig, feat, sig_ev, feat_ev


@pytest.mark.parametrize("poison", list(PATTERNS))
def test_round6_configuration_poisoned(species_models, poison, monkeypatch):
    """test_gpu_parity.py::test_small_groups_coalesced_or_on_lanes_bit_identical[bf16x3] failed once in round 6 with
    NRV_COALESCE=0, batch 1000 (one stream): its inputs and that configuration, the workspace poisoned, two calls."""
    import torch
    m1, m2 = species_models["ecoli"]
    T, n, N, sig, feat, sig_ev, feat_ev = _round6_inputs()

    def run(rv):
        w = (torch.full((n, 6), float("nan"), device="cuda"), torch.full((n, 5), float("nan"), device="cuda"),
             torch.full((n,), -7, dtype=torch.int8, device="cuda"), torch.full((n,), -7, dtype=torch.int8, device="cuda"))
        r = (torch.full((N - T, 6), float("nan"), device="cuda"), torch.full((N - T, 5), float("nan"), device="cuda"),
             torch.full((N - T,), -7, dtype=torch.int8, device="cuda"), torch.full((N - T,), -7, dtype=torch.int8, device="cuda"))
        torch.cuda.synchronize()
        rv.predict_device(sig.data_ptr(), feat.data_ptr(), n, *[x.data_ptr() for x in w])
        rv.predict_read_device(sig_ev.data_ptr(), feat_ev.data_ptr(), N, *[x.data_ptr() for x in r])
        rv.sync()
        torch.cuda.synchronize()
        return w + r

    monkeypatch.delenv("NRV_POISON", raising=False)
    monkeypatch.delenv("NRV_COALESCE", raising=False)
    monkeypatch.delenv("NRV_LANES", raising=False)
    from nanoreviser_amd.engine import Reviser
    ref_rv = Reviser(m1, m2, batch=4096, precision="bf16x3")
    ref = run(ref_rv)
    ref_rv.close()
    assert not any(torch.isnan(x).any() for x in ref[:2] + ref[4:6]) and all((x != -7).all() for x in ref[2:4] + ref[6:8])
    rv = _engine(monkeypatch, m1, m2, "bf16x3", "one_stream", poison)
    for p in range(2):
        for i, (x, y) in enumerate(zip(ref, run(rv))):
            if not torch.equal(x, y):
                bad = torch.nonzero((x != y) if x.dim() == 1 else (x != y).any(1)).flatten()
                pytest.fail(f"{poison} pass {p} output {i}: {bad.numel()} rows differ, first {bad[:8].tolist()}, last {bad[-4:].tolist()}")
    rv.close()


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3", "f32"])
def test_results_do_not_depend_on_stale_device_memory(species_models, mode, monkeypatch):
    """Free device memory filled with NaN / FLT_MAX, handed back to the driver; the engine (switch off) allocates in it."""
    import torch
    from nanoreviser_amd.engine import Reviser
    m1, m2 = species_models["ecoli"]
    T, n, N = 11, 6_037, 13_011
    g = torch.Generator(device="cuda").manual_seed(78)
    sig = (torch.randn(n, T, 50, device="cuda", generator=g) * 1.36 - 0.10).clamp_(-8.4, 4.8)
    feat = torch.rand(n, T, 6, device="cuda", generator=g)
    sig_ev = (torch.randn(N, 50, device="cuda", generator=g) * 1.36 - 0.10).clamp_(-8.4, 4.8)
    feat_ev = torch.rand(N, 6, device="cuda", generator=g)

    def outs(k):
        return (torch.full((k, 6), float("nan"), device="cuda"), torch.full((k, 5), float("nan"), device="cuda"),
                torch.full((k,), -7, dtype=torch.int8, device="cuda"), torch.full((k,), -7, dtype=torch.int8, device="cuda"))

    def run(rv):
        w, r = outs(n), outs(N - T)
        torch.cuda.synchronize()
        rv.predict_device(sig.data_ptr(), feat.data_ptr(), n, *[x.data_ptr() for x in w])
        rv.predict_read_device(sig_ev.data_ptr(), feat_ev.data_ptr(), N, *[x.data_ptr() for x in r])
        rv.sync()
        torch.cuda.synchronize()
        return [x.cpu() for x in w + r]

    def poison(bits):
        blocks = [torch.empty(1 << 28, dtype=torch.int32, device="cuda").fill_(bits) for _ in range(8)]     # 8 GiB
        torch.cuda.synchronize()
        del blocks
        torch.cuda.empty_cache()
        torch.cuda.synchronize()

    monkeypatch.setenv("NRV_PRECISION", mode)
    monkeypatch.delenv("NRV_COALESCE", raising=False)
    monkeypatch.delenv("NRV_POISON", raising=False)
    rv = Reviser(m1, m2, batch=4096)
    ref = run(rv)
    rv.close()
    for bits, coalesce, batch in ((0x7FC00000, "1", 1000), (0x7F7FFFFF, "0", 1000), (0x7FC00000, "0", 992)):
        poison(bits)
        monkeypatch.setenv("NRV_COALESCE", coalesce)
        rv = Reviser(m1, m2, batch=batch)
        for _ in range(2):
            for i, (x, y) in enumerate(zip(ref, run(rv))):
                assert torch.equal(x, y), (mode, hex(bits), coalesce, batch, i, int((x != y).sum()))
        rv.close()
