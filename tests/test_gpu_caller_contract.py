"""How the entry points treat memory and streams that belong to the CALLER (MI355X only, -m gpu): views into larger buffers,
pointers off the 16-byte grid, NULL outputs, a caller's stream, work still running in front of the call, the profiled path.

Inputs (tests/caller_cases.py): the E. coli pair at T = 1, 13 and 32 on the synthetic windows of tests/test_gpu_lstm4_resident.py
(T = 32 added with a seed of its own), read mode on per-event arrays of n + T events; n = 1, 33, 129; the three precision modes,
because different kernels touch caller memory in each.  THE BASELINE of a mode is its result on tight, fresh allocations with a
device synchronise before the call and nrv_sync after it.  Every comparison with it is an equality of bytes; nothing here has a
tolerance.  Two launch-group forms: the default (coalesced), and NRV_COALESCE=0 with batch = 32 - groups on the stream lanes,
every group's output pointer base + 32 g rows.

  0. The baseline against the fp64 oracle (parity_policy, bars unchanged), per mode and T, so that the baseline is not merely the
     code under test; the read-mode baseline equals window mode on the windows cut from its events.
  A1. Guard bands and views, device pointers, window and read mode: every array of the call is the payload of a band
     [64 rows | payload | 64 rows] (caller_cases.banded), at every alignment case (float inputs at 0, 4, 8, 12 modulo 16, p1 / p2
     at 4 modulo 8, a1 / a2 at odd addresses).  Output guards hold 0xA5 and the payloads NaN / -7; after the call the payload is
     the baseline, no sentinel survives and both guards are unchanged.  The same call runs with the INPUT guards holding quiet
     NaN, 3.0e38 and a decoy of valid windows: the baseline's bits all three times (read mode: the back guard starts at event N).
  A2. NULL outputs: each of the four in turn, then all four; the others are the baseline, their guards hold, the payload behind a
     NULL keeps its sentinels, nrv_saturated reports (0, 0).
  B1. The caller's stream: nrv_set_stream(s), s a torch stream (non-blocking); on s a slow producer (matrix products, then the
     copies that put the inputs where a decoy lay), the call, clones of the outputs; no host synchronisation before the final
     s.synchronize().  B2. The handle's own stream behind the legacy default stream: the producer on torch's default stream, the
     call, nrv_sync.  B3. nrv_set_stream(0) after B1, then B2 on the same handle.  In all three the producer's event must still be
     pending when the call returns - otherwise nothing was ordered; k doubles up to three times, then the test fails.  The k each
     case ended with is printed.
  C. The profiled path (nrv_prof_enable 1 and 3; the lanes are off there by design): the calls of A1 give the baseline's bits,
     guards hold, nrv_prof_read counts launches for every stage (1) or for the 192->128 layer (3).
  D. Two handles on two caller streams, B1 on both before either is synchronised.
  E. Host pointers through ctypes (nrv_predict, nrv_predict_read, nrv_predict_reads_raw, nrv_segment_reads, nrv_read_stats): every
     array a view into a larger NumPy array with the same guards, fills and offsets; results equal the engine wrappers' on tight
     arrays; and nrv_predict at T = 11, n = 2049 with the signal 4 bytes into a page-aligned buffer, so that the range
     hipHostRegister locks (4.5 MB, above HostPin's 4 MiB threshold) is not page-aligned and shares pages with its guards -
     and once more with NRV_HOST_REGISTER=0.

WHAT THE CODE SAYS about these accesses, read before the first run of the misaligned and NULL cases:
  * cnn_r_kernel (nrv_cnn_r.h:203-226; f16x2): args.signal is read with raw_buffer_load_b32 only (buf_load4), one float per load,
    through a descriptor whose base is the unit's first event and whose length is what is left of n_rows * T events; rows past
    n_rows and positions outside the window are addressed at offset >= 2^31, past the descriptor's end: the load returns 0 and
    touches no memory.  The descriptor's base is a byte address; nothing assumes more than 4-byte alignment.
  * cnn_kernel (nrv_cnn.h:155-167; bf16x3, f32): raw_buffer_load_b32 too, the descriptor open-ended (0xffffffff), so the bound is
    the index arithmetic: a row past n_rows or a tile past n_tiles is clamped to row 0 of a tile that exists, a position to
    0 .. 49, and the value masked to zero - every address lies in [0, n_rows) rows.  Its store side (finish(), line 204 on, and
    the f32 form) writes P.out = the handle's S buffer in whole 32-row tiles; S is sized in tiles (ensure_workspace).  No caller
    memory is stored to.
  * lstm1_unit (nrv_lstm1.h:58-66; fused into cnn_r_kernel in f16x2, lstm1_kernel otherwise): plain_in is read as two scalar
    floats per lane, src[q] and src[4 + q], under `row < n_rows`; read mode reads event row + t <= n + T - 2.
  * head_h2_kernel (nrv_head_f16x2.h:208-222) and head_final_kernel (nrv_head.h:320-334): prob is stored one float at a time in a
    loop over the run-time class count, argmax one byte, both under `row < args.n_rows`; nothing is read from them.
  * run_group's NULL substitution (nrv_api.hip:1425-1426) points the head at staging set 0, h->d_p[0][*] / h->d_a[0][*] inside
    d_out[0], laid out for cap_rows = stage_windows(read mode) padded to 128 rows (ensure_workspace); a launch group is at most
    group_windows <= stage_windows rows, with lanes batch <= lanes x batch.  The substitute is never smaller than a group.  On
    the lanes concurrent groups all write rows 0 .. 31 of it: unordered stores to a buffer nobody reads.
  * for_groups offsets the caller's pointers by whole groups only (s * T * 50, s * 6, s * 5, s floats / bytes).
So: 4-byte loads and stores for floats, byte stores for calls, row guards on every caller access, a substitute buffer of at least
a group.  The header now states this contract (alignment, extents, NULL outputs).  Every pointer these tests pass lies inside a
live allocation with 64 rows to spare on both sides."""
import ctypes as C

import numpy as np
import pytest

import caller_cases as CC
from nanoreviser_amd import hoststage as hs
from parity_policy import check_vs_fp64

pytestmark = pytest.mark.gpu

KINDS = ("window", "read")
GROUPINGS = ("default", "lanes")
FILLS = ("qnan", "big", "decoy")
NULLS = ((0,), (1,), (2,), (3,), (0, 1, 2, 3))
NAMES = ("p1", "p2", "a1", "a2")
K0 = 32                        # matrix products of the producer to start from: about 30 ms on an MI355X (16 of them take 16 ms)
FP, I8P, DP = C.POINTER(C.c_float), C.POINTER(C.c_int8), C.POINTER(C.c_double)
I16P, I32P = C.POINTER(C.c_int16), C.POINTER(C.c_int32)

_BASE = {}


def _engine(monkeypatch, species_models, T, mode, grouping="default", host_register=None):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_COALESCE", "NRV_LANES", "NRV_PRECISION", "NRV_POISON", "NRV_HOST_REGISTER"):
        monkeypatch.delenv(k, raising=False)
    if grouping == "lanes":
        monkeypatch.setenv("NRV_COALESCE", "0")
    if host_register is not None:
        monkeypatch.setenv("NRV_HOST_REGISTER", str(host_register))
    m1, m2 = species_models["ecoli"]
    if T != m1.T:
        m1, m2 = m1.with_window(T), m2.with_window(T)
    batch = 32 if grouping == "lanes" else 4096
    rv = Reviser(m1, m2, batch=batch, precision=mode)
    monkeypatch.delenv("NRV_COALESCE", raising=False)
    monkeypatch.delenv("NRV_HOST_REGISTER", raising=False)
    assert rv.backend == "hip" and rv.precision == mode and rv.batch == batch and rv.T == T
    return rv


def _sentinels(n):
    import torch
    return [torch.full((n, 6), float("nan"), device="cuda"), torch.full((n, 5), float("nan"), device="cuda"),
            torch.full((n,), -7, dtype=torch.int8, device="cuda"), torch.full((n,), -7, dtype=torch.int8, device="cuda")]


def _call(rv, kind, T, n, ins, outs):
    ptr = [0 if o is None else o.data_ptr() for o in outs]
    if kind == "read":
        rv.predict_read_device(ins[0].data_ptr(), ins[1].data_ptr(), n + T, *ptr)
    else:
        rv.predict_device(ins[0].data_ptr(), ins[1].data_ptr(), n, *ptr)


def _sentinel_free(o):
    """No NaN in a probability array, no -7 in a call array."""
    import torch
    return not bool(torch.isnan(o).any()) if o.is_floating_point() else bool((o != -7).all())


def _no_sentinel(outs):
    return all(_sentinel_free(o) for o in outs)


def _same(got, want):
    import torch
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.contiguous().view(torch.uint8), want.view(torch.uint8))


def _baseline(monkeypatch, species_models, mode, T, kind, n):
    """The mode's outputs on tight, fresh allocations, synchronised on both sides: four device tensors, made once."""
    import torch
    if (mode, T) not in _BASE:
        rv = _engine(monkeypatch, species_models, T, mode)
        d = {}
        for kd in KINDS:
            for m in CC.NS:
                x = CC.inputs(kd, T, m)
                ins = [torch.from_numpy(x["sig"]).cuda(), torch.from_numpy(x["feat"]).cuda()]
                outs = _sentinels(m)
                torch.cuda.synchronize()
                _call(rv, kd, T, m, ins, outs)
                rv.sync()
                torch.cuda.synchronize()
                assert _no_sentinel(outs), (mode, T, kd, m)
                d[(kd, m)] = outs
        assert rv.saturated() == (0, 0)
        rv.close()
        _BASE[(mode, T)] = d
    return _BASE[(mode, T)][(kind, n)]


def _in_shapes(kind, T, n):
    return ((n + T, 50), (n + T, 6)) if kind == "read" else ((n, T, 50), (n, T, 6))


def _bands(kind, T, n, k):
    """The six bands of a call in alignment case k: (inputs of the case, [sig, feat], [p1, p2, a1, a2]) as (buffer, payload)."""
    import torch
    x, off = CC.inputs(kind, T, n), CC.offsets(k)
    ss, fs = _in_shapes(kind, T, n)
    ins = [CC.banded(ss, torch.float32, off["sig"], x["sig"]), CC.banded(fs, torch.float32, off["feat"], x["feat"])]
    outs = [CC.banded((n, 6), torch.float32, off["p1"], float("nan")), CC.banded((n, 5), torch.float32, off["p2"], float("nan")),
            CC.banded((n,), torch.int8, off["a1"], -7), CC.banded((n,), torch.int8, off["a2"], -7)]
    for (_, p), name in zip(ins + outs, CC.ARRAYS):
        assert p.data_ptr() % 16 == (off[name] * p.element_size()) % 16
    return x, ins, outs


def _guarded_calls(rv, kind, T, n, k, base, what, fills=FILLS, null=()):
    """Section A's call in alignment case k, once per fill of the input guards; `null`: the outputs passed as NULL."""
    import torch
    x, ins, outs = _bands(kind, T, n, k)
    for fill in fills:
        for (buf, pay), decoy in zip(ins, (x["decoy_sig"], x["decoy_feat"])):
            CC.fill_guards(buf, pay, {"qnan": float("nan"), "big": CC.BIG, "decoy": decoy}[fill])
        for i, (_, pay) in enumerate(outs):
            pay.fill_(float("nan") if i < 2 else -7)
        torch.cuda.synchronize()
        _call(rv, kind, T, n, [p for _, p in ins], [None if i in null else p for i, (_, p) in enumerate(outs)])
        rv.sync()
        torch.cuda.synchronize()
        for i, (buf, pay) in enumerate(outs):
            tag = (what, f"k={k}", fill, f"null={null}", NAMES[i])
            assert CC.guards_hold(buf, pay), tag + ("a guard changed",)
            if i in null:
                assert bool(torch.isnan(pay).all() if i < 2 else (pay == -7).all()), tag + ("written although NULL was passed",)
            else:
                assert _sentinel_free(pay), tag + ("a sentinel survives",)
                assert _same(pay, base[i]), tag + ("differs from the baseline",)


# ---- 0. the baseline is right ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CC.TS)
@pytest.mark.parametrize("mode", CC.MODES)
def test_baseline_holds_the_fp64_bar(species_models, mode, T, monkeypatch):
    ref = CC.reference(species_models, T)
    n = CC.N_MAX
    base = [o.cpu().numpy() for o in _baseline(monkeypatch, species_models, mode, T, "window", n)]
    for m in range(2):
        what = f"{mode} T={T} m{m + 1}"
        seen = check_vs_fp64(base[m], base[2 + m], ref["q"][m], ref["nf"][m], what)
        print(what, seen)
        srt = np.sort(ref["q"][m], -1)
        decided = srt[:, -1] - srt[:, -2] > 1e-4
        assert np.array_equal(base[2 + m][decided], ref["q"][m].argmax(-1)[decided]), what
    # the smaller cases are rows of the same answer, and read mode is window mode on the windows cut from its events
    for k in CC.NS:
        small = [o.cpu().numpy() for o in _baseline(monkeypatch, species_models, mode, T, "window", k)]
        assert all(np.array_equal(s.view(np.uint8), b[:k].view(np.uint8)) for s, b in zip(small, base)), (mode, T, k)
    rv = _engine(monkeypatch, species_models, T, mode)
    for k in CC.NS:
        x = CC.inputs("read", T, k)
        sw, fw = hs.sliding_windows(x["sig"], x["feat"], T)
        win = rv.predict_pair(np.array(sw, order="C"), np.array(fw, order="C"))
        rd = [o.cpu().numpy() for o in _baseline(monkeypatch, species_models, mode, T, "read", k)]
        assert all(np.array_equal(w.view(np.uint8), r.view(np.uint8)) for w, r in zip(win, rd)), (mode, T, k)
    assert rv.saturated() == (0, 0)
    rv.close()


# ---- A. guard bands, views, NULL outputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", CC.TS)
@pytest.mark.parametrize("mode", CC.MODES)
def test_guard_bands_and_views(species_models, mode, T, kind, monkeypatch):
    for grouping in GROUPINGS:
        rv = _engine(monkeypatch, species_models, T, mode, grouping)
        for n in CC.NS:
            base = _baseline(monkeypatch, species_models, mode, T, kind, n)
            for k in CC.ALIGNMENTS:
                _guarded_calls(rv, kind, T, n, k, base, f"{mode} T={T} {kind} {grouping} n={n}")
        assert rv.saturated() == (0, 0)          # nothing behind a row guard reached the f16x2 range guard either
        rv.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", CC.TS)
@pytest.mark.parametrize("mode", CC.MODES)
def test_null_outputs(species_models, mode, T, kind, monkeypatch):
    for grouping in GROUPINGS:
        rv = _engine(monkeypatch, species_models, T, mode, grouping)
        for n in CC.NS:
            base = _baseline(monkeypatch, species_models, mode, T, kind, n)
            for k in CC.ALIGNMENTS:
                for null in NULLS:
                    _guarded_calls(rv, kind, T, n, k, base, f"{mode} T={T} {kind} {grouping} n={n}", fills=("decoy",), null=null)
        assert rv.saturated() == (0, 0)
        rv.close()


# ---- B. stream order without host synchronisation -------------------------------------------------------------------------------
def _stream_case(rv, kind, T, n, base, stream, what):
    """One ordered case.  stream: the torch stream the handle was pointed at (B1), or None: the producer runs on torch's default
    stream and the call on the handle's own (B2).  Returns the k it ended with."""
    import torch
    x = CC.inputs(kind, T, n)
    rows = n + T if kind == "read" else n
    src = [torch.from_numpy(x["sig"]).cuda(), torch.from_numpy(x["feat"]).cuda()]
    k = K0
    for _ in range(4):                                     # the first try and at most three doublings
        ins = [torch.from_numpy(x["decoy_sig"][:rows].copy()).cuda(), torch.from_numpy(x["decoy_feat"][:rows].copy()).cuda()]
        outs = _sentinels(n)
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            ev = CC.slow_producer(stream, list(zip(ins, src)), k)
            _call(rv, kind, T, n, ins, outs)
            pending = not ev.query()
            with torch.cuda.stream(stream):
                got = [o.clone() for o in outs]
            stream.synchronize()
        else:
            assert torch.cuda.current_stream().cuda_stream == 0            # torch's default stream is the legacy default stream
            ev = CC.slow_producer(torch.cuda.current_stream(), list(zip(ins, src)), k)
            _call(rv, kind, T, n, ins, outs)
            pending = not ev.query()
            rv.sync()
            got = outs
        torch.cuda.synchronize()
        assert _no_sentinel(got), (what, k, "a sentinel survives: the consumer ran ahead of the call")
        for i in range(4):
            assert _same(got[i], base[i]), (what, k, NAMES[i], "differs from the baseline: the call ran ahead of the producer")
        if pending:
            print(f"{what}: k = {k}")
            return k
        k *= 2
    pytest.fail("producer finished before the call was enqueued: nothing was ordered")


@pytest.mark.parametrize("grouping", GROUPINGS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", CC.MODES)
def test_own_stream_behind_the_default_stream(species_models, mode, kind, grouping, monkeypatch):
    T, n = 13, CC.N_MAX
    CC.producer_scratch()
    base = _baseline(monkeypatch, species_models, mode, T, kind, n)
    rv = _engine(monkeypatch, species_models, T, mode, grouping)
    _stream_case(rv, kind, T, n, base, None, f"B2 {mode} {kind} {grouping}")
    assert rv.saturated() == (0, 0)
    rv.close()


@pytest.mark.parametrize("grouping", GROUPINGS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", CC.MODES)
def test_callers_stream_then_back_on_its_own(species_models, mode, kind, grouping, monkeypatch):
    import torch
    T, n = 13, CC.N_MAX
    CC.producer_scratch()
    base = _baseline(monkeypatch, species_models, mode, T, kind, n)
    rv = _engine(monkeypatch, species_models, T, mode, grouping)
    s = torch.cuda.Stream()
    rv.set_stream(s.cuda_stream)
    _stream_case(rv, kind, T, n, base, s, f"B1 {mode} {kind} {grouping}")
    rv.set_stream(0)
    _stream_case(rv, kind, T, n, base, None, f"B3 {mode} {kind} {grouping}")
    assert rv.saturated() == (0, 0)
    rv.close()


# ---- C. the profiled path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", CC.TS)
@pytest.mark.parametrize("mode", CC.MODES)
def test_profiled_path_gives_the_same_bits(species_models, mode, T, kind, monkeypatch):
    for grouping in GROUPINGS:
        rv = _engine(monkeypatch, species_models, T, mode, grouping)
        try:
            for prof in (1, 3):
                rv.prof_enable(prof)
                for n in CC.NS:
                    base = _baseline(monkeypatch, species_models, mode, T, kind, n)
                    for k in CC.ALIGNMENTS:
                        _guarded_calls(rv, kind, T, n, k, base, f"{mode} T={T} {kind} {grouping} prof={prof} n={n}")
                counts = {name: cnt for name, (_, cnt) in rv.prof_read().items()}
                assert len(counts) == 6, counts
                if prof == 1:
                    assert all(c > 0 for c in counts.values()), (mode, grouping, prof, counts)
                else:
                    assert counts["lstm3 192->128"] > 0, (mode, grouping, prof, counts)
        finally:
            rv.prof_enable(0)
        _guarded_calls(rv, kind, T, CC.N_MAX, 1, _baseline(monkeypatch, species_models, mode, T, kind, CC.N_MAX),
                       f"{mode} T={T} {kind} {grouping} after profiling", fills=("decoy",))
        assert rv.saturated() == (0, 0)
        rv.close()


# ---- D. two handles, two caller streams -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouping", GROUPINGS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", CC.MODES)
def test_two_handles_on_two_streams(species_models, mode, kind, grouping, monkeypatch):
    import torch
    T, n = 13, CC.N_MAX
    CC.producer_scratch()
    base = _baseline(monkeypatch, species_models, mode, T, kind, n)
    x = CC.inputs(kind, T, n)
    rows = n + T if kind == "read" else n
    src = [torch.from_numpy(x["sig"]).cuda(), torch.from_numpy(x["feat"]).cuda()]
    rvs = [_engine(monkeypatch, species_models, T, mode, grouping) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    for rv, s in zip(rvs, streams):
        rv.set_stream(s.cuda_stream)
    k = K0
    for _ in range(4):
        ins = [[torch.from_numpy(x["decoy_sig"][:rows].copy()).cuda(), torch.from_numpy(x["decoy_feat"][:rows].copy()).cuda()] for _ in range(2)]
        outs = [_sentinels(n) for _ in range(2)]
        evs = []
        for h in range(2):
            streams[h].wait_stream(torch.cuda.current_stream())
            evs.append(CC.slow_producer(streams[h], list(zip(ins[h], src)), k))
            _call(rvs[h], kind, T, n, ins[h], outs[h])
        pending = [not e.query() for e in evs]
        got = []
        for h in range(2):
            with torch.cuda.stream(streams[h]):
                got.append([o.clone() for o in outs[h]])
        for s in streams:
            s.synchronize()
        torch.cuda.synchronize()
        for h in range(2):
            assert _no_sentinel(got[h]), (mode, kind, grouping, h, k)
            for i in range(4):
                assert _same(got[h][i], base[i]), (mode, kind, grouping, f"handle {h}", NAMES[i], k)
        if all(pending):
            print(f"D {mode} {kind} {grouping}: k = {k}")
            break
        k *= 2
    else:
        pytest.fail("producer finished before the call was enqueued: nothing was ordered")
    for rv in rvs:
        rv.set_stream(0)
        assert rv.saturated() == (0, 0)
        rv.close()


# ---- E. host pointers -----------------------------------------------------------------------------------------------------------
def _np_fill(fill, decoy, dtype):
    """What the guards of a host INPUT hold: floats NaN / 3.0e38 / the decoy; integer arrays the bytes 0xA5 / 0x7F / the decoy."""
    if fill == "decoy":
        return decoy
    if np.dtype(dtype).kind == "f":
        return float("nan") if fill == "qnan" else CC.BIG
    return CC.GUARD_BYTE if fill == "qnan" else 0x7F


def _out_bands(n, k):
    off = CC.offsets(k)
    return [CC.banded_np((n, 6), np.float32, off["p1"], np.nan), CC.banded_np((n, 5), np.float32, off["p2"], np.nan),
            CC.banded_np((n,), np.int8, off["a1"], -7), CC.banded_np((n,), np.int8, off["a2"], -7)]


def _check_host_outs(outs, want, what):
    for (buf, pay), w, name in zip(outs, want, NAMES):
        assert CC.guards_hold(buf, pay), (what, name, "a guard changed")
        assert pay.shape == w.shape and np.array_equal(pay.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (what, name)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", CC.MODES)
def test_host_pointer_calls_on_views(species_models, mode, kind, monkeypatch):
    T = 13
    rv = _engine(monkeypatch, species_models, T, mode)
    fn = rv._lib.nrv_predict_read if kind == "read" else rv._lib.nrv_predict
    for n in (33, 129):
        x = CC.inputs(kind, T, n)
        want = rv.predict_read(x["sig"], x["feat"]) if kind == "read" else rv.predict_pair(x["sig"], x["feat"])
        assert not np.isnan(want[0]).any() and not np.isnan(want[1]).any()
        ss, fs = _in_shapes(kind, T, n)
        for k in CC.ALIGNMENTS:
            off = CC.offsets(k)
            ins = [CC.banded_np(ss, np.float32, off["sig"], x["sig"]), CC.banded_np(fs, np.float32, off["feat"], x["feat"])]
            for fill in FILLS:
                for (buf, pay), decoy in zip(ins, (x["decoy_sig"], x["decoy_feat"])):
                    CC.fill_guards(buf, pay, _np_fill(fill, decoy, np.float32))
                outs = _out_bands(n, k)
                rv._check(fn(rv._h, ins[0][1].ctypes.data_as(FP), ins[1][1].ctypes.data_as(FP), n + T if kind == "read" else n,
                             outs[0][1].ctypes.data_as(FP), outs[1][1].ctypes.data_as(FP), outs[2][1].ctypes.data_as(I8P),
                             outs[3][1].ctypes.data_as(I8P)))
                _check_host_outs(outs, want, (mode, kind, n, k, fill))
    assert rv.saturated() == (0, 0)
    rv.close()


@pytest.mark.parametrize("mode", CC.MODES)
def test_raw_read_calls_on_views(species_models, reads, read_index, mode, monkeypatch):
    keys = [e["key"] for e in sorted(read_index, key=lambda e: e["n_bases"])]
    pick = []
    for key in keys[:3]:                                       # the two shortest reads; the third is the decoy
        _, rd, _ = reads(key)
        pick.append((hs.read_tensors_raw(rd), int(rd.length[-1])))
    two = pick[:2]
    args = ([r.raw for r, _ in two], [r.starts for r, _ in two], [r.feat_ev for r, _ in two], [r.shift for r, _ in two],
            [r.scale for r, _ in two])
    rv = _engine(monkeypatch, species_models, 11, mode)
    T = rv.T
    raw, st, feat, descs, nr, N, _ = rv.pack_reads_raw(*args, T)
    ld = np.array([d for _, d in two], np.int32)
    n = N - T
    want_calls = [a.copy() for a in rv.predict_reads_raw(*args)]
    want_sig = rv.segment_reads(args[0], args[1], args[3], args[4])
    want_stats = rv.read_stats(args[0], args[1], [d for _, d in two])
    dec = pick[2][0]
    decoys = (dec.raw, dec.starts, dec.feat_ev, np.arange(100, 300, dtype=np.int32))
    lib, h = rv._lib, rv._h
    for k in CC.ALIGNMENTS:
        ins = [CC.banded_np(raw.shape, np.int16, k, raw), CC.banded_np(st.shape, np.int32, k, st),
               CC.banded_np(feat.shape, np.float32, k, feat), CC.banded_np(ld.shape, np.int32, k, ld)]
        head = (h, ins[0][1].ctypes.data_as(I16P), raw.size, ins[1][1].ctypes.data_as(I32P))
        for fill in FILLS:
            what = (mode, k, fill)
            for (buf, pay), decoy in zip(ins, decoys):
                CC.fill_guards(buf, pay, _np_fill(fill, decoy, pay.dtype))
            outs = _out_bands(n, k)
            rv._check(lib.nrv_predict_reads_raw(*head, ins[2][1].ctypes.data_as(FP), N, descs, nr, outs[0][1].ctypes.data_as(FP),
                                                outs[1][1].ctypes.data_as(FP), outs[2][1].ctypes.data_as(I8P), outs[3][1].ctypes.data_as(I8P)))
            _check_host_outs(outs, want_calls, what + ("nrv_predict_reads_raw",))
            sb, sp = CC.banded_np((N, 50), np.float32, k, np.nan)
            rv._check(lib.nrv_segment_reads(*head, N, descs, nr, sp.ctypes.data_as(FP)))
            assert CC.guards_hold(sb, sp) and np.array_equal(sp.view(np.uint8), want_sig.view(np.uint8)), what + ("nrv_segment_reads",)
            so = [CC.banded_np((nr,), np.float64, k, np.nan), CC.banded_np((nr,), np.float64, k, np.nan),
                  CC.banded_np((N,), np.float64, k, np.nan), CC.banded_np((N,), np.float64, k, np.nan),
                  CC.banded_np((N, 2), np.float32, 2 * k - 1 if k else 0, np.nan)]
            rv._check(lib.nrv_read_stats(*head, N, descs, nr, ins[3][1].ctypes.data_as(I32P), *[p.ctypes.data_as(DP) for _, p in so[:4]],
                                         so[4][1].ctypes.data_as(FP)))
            for (buf, pay), w, name in zip(so, want_stats, ("shift", "scale", "mean", "std", "feat12")):
                assert CC.guards_hold(buf, pay), what + ("nrv_read_stats", name, "a guard changed")
                assert np.array_equal(pay.view(np.uint8), np.ascontiguousarray(w, pay.dtype).view(np.uint8)), what + ("nrv_read_stats", name)
    assert rv.saturated()[0] == 0
    rv.close()


def test_registered_signal_off_the_page_grid(species_models, monkeypatch):
    """nrv_predict, T = 11, n = 2049: the signal is 4.5 MB, above the 4 MiB from which HostPin::pin registers the caller's array
    in place; it starts 4 bytes behind a front guard in a page-aligned buffer, so the registered range begins and ends inside
    pages it shares with the guards.  The same call with NRV_HOST_REGISTER=0 (bounce copies)."""
    from oracle import nrv_oracle as O
    T, n = 11, 2049
    sig, feat = O.synth_windows(n, T, seed=8211)
    dsig, dfeat = O.synth_windows(129, T, seed=13211)
    assert sig.nbytes > (4 << 20) > feat.nbytes
    ref = None
    for reg in (1, 0):
        rv = _engine(monkeypatch, species_models, T, "f16x2", host_register=reg)
        tight = rv.predict_pair(sig, feat)
        ref = tight if ref is None else ref
        for a, b in zip(tight, ref):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), reg
        sb, sp = CC.banded_np(sig.shape, np.float32, 1, sig, align=4096)
        fb, fp = CC.banded_np(feat.shape, np.float32, 1, feat, align=4096)
        assert sb.ctypes.data % 4096 == 0 and sp.ctypes.data % 4096 == (64 * T * 200 + 4) % 4096 != 0
        assert (sp.ctypes.data + sp.nbytes) % 4096 != 0
        for fill in FILLS:
            CC.fill_guards(sb, sp, _np_fill(fill, dsig, np.float32))
            CC.fill_guards(fb, fp, _np_fill(fill, dfeat, np.float32))
            keep = [np.array(g) for g in CC.guards(sb, sp)]
            outs = _out_bands(n, 1)
            rv._check(rv._lib.nrv_predict(rv._h, sp.ctypes.data_as(FP), fp.ctypes.data_as(FP), n, outs[0][1].ctypes.data_as(FP),
                                          outs[1][1].ctypes.data_as(FP), outs[2][1].ctypes.data_as(I8P), outs[3][1].ctypes.data_as(I8P)))
            _check_host_outs(outs, ref, (reg, fill))
            assert all(np.array_equal(a, b) for a, b in zip(keep, CC.guards(sb, sp))), (reg, fill, "registration changed a guard")
            assert np.array_equal(sp.view(np.uint8), sig.view(np.uint8))
        assert rv.saturated() == (0, 0)
        rv.close()
