"""Merge, Phred and packing of revised reads on the device (MI355X only, -m gpu): csrc/nrv_merge.h through nrv_merge_calls,
nrv_revise_reads_raw_begin / nrv_revise_reads_raw and the command line's --device_merge.

Everything is compared BYTE FOR BYTE - nothing here has a tolerance.  hoststage.emit_calls with cli.phred_chars is the definition.
T = 11, the shipped weights (the same synthetic calls and the raw-read call at T = 1, 2, 12, 13, 32: tests/test_gpu_window_lengths.py):
  1. nrv_merge_calls on synthetic calls: all 6 x 5 class pairs x the 4 bases and an out-of-alphabet base, each at a read's first
     window, at its last window and either side of a tile boundary of the scan; confidences at every Phred threshold +- 1 ulp, the
     smaller one in p1 and in p2; reads of 0, 1, T, T + 1, T + 2, 4096 + T and 200 000 events; 1, 2 and 37 reads per call; empty
     reads at the start, in the middle and at the end of a call; all-drop calls and an all-two-character call (the output fills
     its capacity exactly); out-of-range labels; FASTA and FASTQ;
  2. nrv_revise_reads_raw on the fixture reads against nrv_predict_reads_raw + emit_calls: E. coli and human weights, f16x2 /
     bf16x3 / f32, one call, two calls in flight, with and without device statistics, a call without a window, and a read whose
     spikes trip the f16x2 range guard (the merge runs again behind the f32 re-run);
  3. 1 and 2 again on handles created under NRV_POISON (quiet NaN, FLT_MAX, -1500.0f): the same bytes;
  4. the command line with and without --device_merge, FASTA and FASTQ, alone and with --device_stats: the same bytes in every
     file; and with one read forced to fail: the original basecalls, the same exit code.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "bf16x3", "f32"]
PATTERNS = {"qnan": 0x7FC00000, "fltmax": 0x7F7FFFFF, "m1500": 0xC4BB8000}
FAST5 = os.path.join(GOLD, "fast5")
TILE = 256                                    # csrc/nrv_merge.h kMergeTile
ALPHABET = np.frombuffer(b"ACGTN", np.uint8)  # the four bases and one letter outside them
COMBOS = [(x, y, b) for x in range(6) for y in range(5) for b in range(5)]


def _engine(monkeypatch, m1, m2, poison=None, **kw):
    from nanoreviser_amd.engine import Reviser
    if poison is None:
        monkeypatch.delenv("NRV_POISON", raising=False)
    else:
        monkeypatch.setenv("NRV_POISON", f"{PATTERNS[poison]:08x}")
    for k in ("NRV_PRECISION", "NRV_COALESCE", "NRV_LANES"):
        monkeypatch.delenv(k, raising=False)
    rv = Reviser(m1, m2, **kw)
    monkeypatch.delenv("NRV_POISON", raising=False)
    return rv


@pytest.fixture(scope="module")
def fixture_reads(reads):
    out = []
    for k in reads.keys:
        _, rd, _ = reads(k)
        out.append((hs.read_tensors_raw(rd), int(rd.length[-1])))
    return out


# ---- 1. the merge alone ----------------------------------------------------------------------------------------------------------
def _random_call(rng, ev_len, T):
    N = int(np.sum(ev_len))
    n = max(N - T, 0)
    bases = rng.choice(ALPHABET[:4], N).astype(np.uint8)
    a1, a2 = rng.integers(0, 6, n).astype(np.int8), rng.integers(0, 5, n).astype(np.int8)
    p1, p2 = rng.random((n, 6), dtype=np.float32), rng.random((n, 5), dtype=np.float32)
    return {"bases": bases, "ev_len": np.asarray(ev_len, np.int64), "a1": a1, "a2": a2, "p1": p1, "p2": p2}


def _put(call, T, read_first_event, j, combo):
    """Window of event j of the read that starts at read_first_event := combo (classes and the original base)."""
    x, y, b = combo
    E = read_first_event + j
    call["a1"][E - (T - 1) // 2], call["a2"][E - (T - 1) // 2], call["bases"][E] = x, y, ALPHABET[b]


def _synthetic_calls(T):
    rng = np.random.default_rng(2610)
    o = (T - 1) // 2
    thr = cli.phred_thresholds()
    calls = {}
    # every combination as a read's first and as its last window: 150 reads of two windows, with the short reads between them
    ev_len = []
    for k in range(len(COMBOS)):
        ev_len += [T + 2] + ([[0], [1], [T], [T + 1], [0, 0]][k % 5] if k % 10 == 0 else [])
    c = _random_call(rng, [0, 0] + ev_len + [0], T)                      # empty reads in front, in the middle and at the end
    e0, k = 0, 0
    for el in c["ev_len"]:
        if el == T + 2:
            _put(c, T, e0, o, COMBOS[k])
            _put(c, T, e0, o + 1, COMBOS[(7 * k + 3) % len(COMBOS)])
            k += 1
        e0 += int(el)
    assert k == len(COMBOS)
    calls["class pairs, first and last window"] = c
    # ... and either side of a tile boundary of the scan: a long read behind a short one (so that its events are not tile-aligned)
    c = _random_call(rng, [3, TILE * (len(COMBOS) + 2) + T], T)
    for k, combo in enumerate(COMBOS):
        for E in ((k + 1) * TILE - 1, (k + 1) * TILE):
            _put(c, T, 3, E - 3, combo)
    calls["class pairs at tile boundaries"] = c
    # confidences at every threshold and one ulp either side, the smaller one in p1 and then in p2
    vals = np.concatenate([[t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(2))] for t in thr]).astype(np.float32)
    vals = np.concatenate([vals, [0.0, 1.0, np.nextafter(np.float32(1), np.float32(0))]]).astype(np.float32)
    c = _random_call(rng, [2 * len(vals) + T], T)
    for i, v in enumerate(vals):
        c["p1"][i, c["a1"][i]], c["p2"][i, c["a2"][i]] = v, 1.0
        c["p1"][len(vals) + i, c["a1"][len(vals) + i]], c["p2"][len(vals) + i, c["a2"][len(vals) + i]] = 1.0, v
    calls["confidences at the thresholds"] = c
    calls["one read of 4096 + T"] = _random_call(rng, [4096 + T], T)
    calls["one read of T + 1"] = _random_call(rng, [T + 1], T)
    calls["two reads"] = _random_call(rng, [T + 2, 700], T)
    calls["37 reads, one of 200 000 events"] = _random_call(rng, list(rng.integers(0, 60, 20)) + [200_000] + list(rng.integers(T, 900, 16)), T)
    c = _random_call(rng, [40, 0, 2000, T + 1], T)
    c["a1"][:], c["a2"][:] = 1, 0                                        # both '-': every window drops its base
    calls["all drop"] = c
    c = _random_call(rng, [3000], T)
    c["a1"][:], c["a2"][:] = 0, rng.integers(1, 5, len(c["a2"]))         # 'D' + a base: two characters per window
    calls["all two characters"] = c
    c = _random_call(rng, [500, 77], T)
    c["a1"][:], c["a2"][:] = rng.integers(-128, 128, len(c["a1"])), rng.integers(-128, 127, len(c["a2"]))
    calls["labels out of range (no quality)"] = c
    return calls


def _expected(c, T, fastq):
    qc = cli.phred_chars(c["p1"], c["p2"], c["a1"], c["a2"]) if fastq and len(c["a1"]) else (np.zeros(0, np.uint8) if fastq else None)
    return hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], qc, T)


def _same_merged(got, want, what):
    for j, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (what, j)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.shape, w.shape)
            bad = np.flatnonzero(g != w)
            assert not len(bad), (what, j, len(bad), bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


def _merge_alone(rv):
    """nrv_merge_calls on every synthetic call, FASTA and FASTQ -> [(name, array)]; checked against emit_calls on the way."""
    T, out = rv.T, []
    thr = cli.phred_thresholds()
    for name, c in _synthetic_calls(T).items():
        for fastq in (False, True):
            if fastq and "no quality" in name:
                continue
            want = _expected(c, T, fastq)
            got = rv.merge_calls_device(c["bases"], c["ev_len"], c["a1"], c["a2"], *((c["p1"], c["p2"], thr) if fastq else ()))
            _same_merged(got, want, (name, fastq))
            if name == "all two characters":
                assert len(got[0]) == int(c["ev_len"].sum()) + len(c["a1"])          # the capacity, exactly
            if name == "all drop":
                assert len(got[0]) == int(np.minimum(c["ev_len"], T).sum())            # what is left: the kept ends of every read
            out += [(f"{name} {fastq} {j}", x) for j, x in enumerate(got) if x is not None]
    # no window at all: the reads as they are
    b = np.frombuffer(b"ACGTAC", np.uint8)
    got = rv.merge_calls_device(b, [2, 0, 4], np.zeros(0, np.int8), np.zeros(0, np.int8), np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32), thr)
    assert got[0].tobytes() == b"ACGTAC" and got[1].tobytes() == b"######" and got[2].tolist() == [0, 2, 2, 6]
    got = rv.merge_calls_device(np.zeros(0, np.uint8), [], np.zeros(0, np.int8), np.zeros(0, np.int8))
    assert len(got[0]) == 0 and got[1] is None and got[2].tolist() == [0]
    return out


def test_merge_alone_equals_emit_calls(species_models, monkeypatch):
    T = species_models["ecoli"][0].T
    calls = _synthetic_calls(T)
    seen = set()                                           # the synthetic calls do hold what the docstring says
    for c in calls.values():
        first, _, count = hs.merge_calls(c["bases"][(T - 1) // 2:][:len(c["a1"])], c["a1"], c["a2"])
        seen |= set(count.tolist())
    assert seen == {0, 1, 2}
    from nanoreviser_amd.engine import NrvError
    rv = _engine(monkeypatch, *species_models["ecoli"])
    _merge_alone(rv)
    with pytest.raises(NrvError):                          # n_win must be sum(ev_len) - T
        rv.merge_calls_device(np.full(40, 65, np.uint8), [40], np.zeros(5, np.int8), np.zeros(5, np.int8))
    _merge_alone(rv)                                       # the handle is fine afterwards
    rv.close()


# ---- 2. end to end ---------------------------------------------------------------------------------------------------------------
def _blind(rr):
    feat = rr.feat_ev.copy()
    feat[:, 1:3] = np.nan
    return feat


def _host_revised(rv, rrs, fastq):
    """nrv_predict_reads_raw fed by the host stage + the host merge: the reference of every end-to-end form."""
    p1, p2, a1, a2 = rv.predict_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs],
                                          [r.shift for r in rrs], [r.scale for r in rrs])
    qc = cli.phred_chars(p1, p2, a1, a2) if fastq else None
    return hs.emit_calls(np.concatenate([np.asarray(r.bases, "S1") for r in rrs]).view(np.uint8), [len(r.starts) for r in rrs], a1, a2, qc, rv.T)


def _packed(rv, rrs, lds, fastq, stats):
    if stats:
        p = rv.pack_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [_blind(r) for r in rrs], [np.nan] * len(rrs), [np.nan] * len(rrs), rv.T)
        p = rv.with_device_stats(p, lds, [1] * len(rrs))
    else:
        p = rv.pack_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs], [r.shift for r in rrs], [r.scale for r in rrs], rv.T)
    return rv.with_device_merge(p, np.concatenate([np.asarray(r.bases, "S1") for r in rrs]), fastq)


def _revise(rv, fixture_reads):
    """Every end-to-end form on the fixture reads -> [(name, array)] of the NEW calls; compared with the host merge inside."""
    out = []
    rrs, lds = [r for r, _ in fixture_reads], [ld for _, ld in fixture_reads]
    for fastq in (False, True):
        ref_all = _host_revised(rv, rrs, fastq)
        ref_a, ref_b = _host_revised(rv, rrs[:3], fastq), _host_revised(rv, rrs[3:], fastq)
        for stats in (False, True):
            what = f"fastq {fastq} stats {stats}"
            got = rv.run_packed_raw(_packed(rv, rrs, lds, fastq, stats))                      # one call
            _same_merged(got, ref_all, what + " one call")
            out += [(f"{what} one {j}", x.copy()) for j, x in enumerate(got) if x is not None]
            ta = rv.begin_packed_raw(_packed(rv, rrs[:3], lds[:3], fastq, stats))             # two calls in flight
            tb = rv.begin_packed_raw(_packed(rv, rrs[3:], lds[3:], fastq, stats))
            got_a, got_b = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
            _same_merged(got_a, ref_a, what + " in flight, first")
            _same_merged(got_b, ref_b, what + " in flight, second")
            out += [(f"{what} b {j}", x.copy()) for j, x in enumerate(got_b) if x is not None]
        # a new call and an old one in flight together
        old = rv.pack_reads_raw([r.raw for r in rrs[3:]], [r.starts for r in rrs[3:]], [r.feat_ev for r in rrs[3:]],
                                [r.shift for r in rrs[3:]], [r.scale for r in rrs[3:]], rv.T)
        want_old = [x.copy() for x in rv.run_packed_raw(old)]
        tn, to = rv.begin_packed_raw(_packed(rv, rrs[:3], lds[:3], fastq, False)), rv.begin_packed_raw(old)
        _same_merged(rv.end_packed_raw(tn), ref_a, "a new call in front of an old one")
        for x, y in zip(want_old, rv.end_packed_raw(to)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # a call without a window: nothing is enqueued, the read comes back as it is
    r0 = rrs[0]
    k = rv.T
    p = rv.pack_reads_raw([r0.raw], [r0.starts[:k]], [r0.feat_ev[:k]], [r0.shift], [r0.scale], rv.T)
    seq, qual, off = rv.run_packed_raw(rv.with_device_merge(p, np.asarray(r0.bases, "S1")[:k], True))
    assert seq.tobytes() == np.asarray(r0.bases, "S1")[:k].tobytes() and qual.tobytes() == b"#" * k and off.tolist() == [0, k]
    return out


@pytest.mark.parametrize("sp", ["ecoli", "human"])
def test_revise_reads_raw_equals_the_host_merge(species_models, fixture_reads, sp, monkeypatch):
    rv = _engine(monkeypatch, *species_models[sp])
    for mode in MODES:
        rv.set_precision(mode)
        _revise(rv, fixture_reads)
        assert rv.saturated() == (0, 0), (sp, mode)
    rv.close()


@pytest.mark.parametrize("sp", ["ecoli", "human"])
def test_range_guard_rerun_runs_the_merge_again(species_models, fixture_reads, sp, monkeypatch):
    """The spiked read of test_gpu_device_stats.py: the call is re-run on the f32 kernels in nrv_reads_raw_end, and the merged
    block that comes back is the one computed behind that re-run - the records are those of the f32 mode."""
    rr, _ = fixture_reads[-1]
    N = 1500
    starts = rr.starts[:N].copy()
    raw = rr.raw[: int(starts[-1]) + 60].copy()
    rng = np.random.default_rng(11)
    pos = rng.choice(len(raw), 30, replace=False)
    raw[pos] = rng.choice(np.array([-32768, 32767], np.int16), 30)
    sh, sc, c1, c2 = hs.stats_columns(raw, starts, 3)
    assert (32767 - sh) / sc > 250
    feat = rr.feat_ev[:N].copy()
    feat[:, 1], feat[:, 2] = c1, c2
    blind = feat.copy()
    blind[:, 1:3] = np.nan
    other, other_ld = fixture_reads[0]
    bases = np.concatenate([np.asarray(other.bases, "S1"), np.asarray(rr.bases, "S1")[:N]])
    rv = _engine(monkeypatch, *species_models[sp])
    rv.set_precision("f32")
    p1, p2, a1, a2 = rv.predict_reads_raw([other.raw, raw], [other.starts, starts], [other.feat_ev, feat], [other.shift, sh], [other.scale, sc])
    want = {fq: hs.emit_calls(bases.view(np.uint8), [len(other.starts), N], a1, a2, cli.phred_chars(p1, p2, a1, a2) if fq else None, rv.T)
            for fq in (False, True)}
    assert rv.saturated()[1] == 0
    for mode in MODES:
        rv.set_precision(mode)
        for stats in (False, True):
            for fq in (False, True):
                r0 = rv.saturated()[1]
                if stats:
                    p = rv.pack_reads_raw([other.raw, raw], [other.starts, starts], [_blind(other), blind], [np.nan, np.nan], [np.nan, np.nan], rv.T)
                    p = rv.with_device_stats(p, [other_ld, 3], [1, 1])
                else:
                    p = rv.pack_reads_raw([other.raw, raw], [other.starts, starts], [other.feat_ev, feat], [other.shift, sh], [other.scale, sc], rv.T)
                got = rv.run_packed_raw(rv.with_device_merge(p, bases, fq))
                assert rv.saturated()[1] - r0 == (1 if mode == "f16x2" else 0), (mode, stats, fq)
                if mode != "bf16x3":                       # f16x2 was re-run in f32: the f32 mode's records, byte for byte
                    _same_merged(got, want[fq], (sp, mode, stats, fq))
    rv.close()


# ---- 3. poison -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_poisoned_workspace_gives_the_same_bytes(species_models, fixture_reads, mode, monkeypatch):
    """Records, tile sums, offsets and characters are written by the call's own kernels before anything reads them: a handle whose
    every buffer (the bases in the input block and the merged block with its page-locked twin included) holds a pattern gives the
    clean handle's bytes, on a first and on a second pass."""
    sp = "ecoli"
    clean = _engine(monkeypatch, *species_models[sp], precision=mode)
    ref = _merge_alone(clean) + _revise(clean, fixture_reads)
    assert clean.saturated() == (0, 0)
    clean.close()
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models[sp], poison=poison, precision=mode)
        for p in range(2):
            got = _merge_alone(rv) + _revise(rv, fixture_reads)
            assert [k for k, _ in got] == [k for k, _ in ref]
            for (k, x), (_, y) in zip(ref, got):
                assert x.dtype == y.dtype and np.array_equal(x, y), (mode, poison, p, k)
        assert rv.saturated() == (0, 0), (mode, poison)
        rv.close()


# ---- 4. command line -------------------------------------------------------------------------------------------------------------
def _inputs(tmp_path):
    big = tmp_path / "in"
    big.mkdir()
    src = sorted(glob.glob(os.path.join(FAST5, "*.fast5")) + glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))
    for i in range(15):
        shutil.copy(src[i % len(src)], big / f"s{i:02d}.fast5")
    return str(big)


def _clean_env(monkeypatch):
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NRV_CLI_GROUPS", "4")                                # a few reads per device call: several calls in flight


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_command_line_writes_the_same_bytes_with_and_without_the_switch(tmp_path, monkeypatch, fmt):
    from nanoreviser_amd.engine import Reviser
    _clean_env(monkeypatch)
    forms = []
    real = Reviser.begin_packed_raw
    monkeypatch.setattr(Reviser, "begin_packed_raw", lambda self, packed: forms.append((len(packed), len(packed) == 12 and packed[7] is not None)) or real(self, packed))
    d = _inputs(tmp_path)
    outs = {}
    for tag, extra in (("off", []), ("merge", ["--device_merge"]), ("both", ["--device_merge", "--device_stats"])):
        del forms[:]
        out = str(tmp_path / tag) + "/"
        assert cli.main(["-d", d, "-o", out, "-S", "ecoli", "-F", fmt, "--gpus", "1", "--thread", "4"] + extra) == 0
        outs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        assert outs[tag]["failed_reads.txt"] == b"" and len(outs[tag]) == 16
        assert forms and set(forms) == {"off": {(7, False)}, "merge": {(12, False)}, "both": {(12, True)}}[tag], (tag, forms)
    assert outs["merge"] == outs["off"] and outs["both"] == outs["off"]
    # the fixture directory as it is (two reads: no parser pool): the switch changes no call
    del forms[:]
    out = str(tmp_path / "small") + "/"
    assert cli.main(["-d", FAST5, "-o", out, "-S", "ecoli", "-F", fmt, "--gpus", "1", "--thread", "4", "--device_merge"]) == 0
    assert not [f for f in forms if f[0] == 12]


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_command_line_failed_read_gets_its_original_basecalls(tmp_path, monkeypatch, fmt):
    """One read of a device call cannot be written by the native finisher (its destination is sent to a directory that does not
    exist, so the C call reports that read alone): with and without the switch it goes to `fallback` - the original basecalls
    come out, it is listed in the failed-reads file, the exit code is the same - and every file holds the same bytes."""
    from nanoreviser_amd import hostlib
    _clean_env(monkeypatch)
    d = _inputs(tmp_path)
    hit = []

    def misdirect(real, at):
        def f(*a):
            a = list(a)
            a[at] = [os.path.join(os.path.dirname(x), "no_such_dir", "x") if "s07_out" in x else x for x in a[at]]
            hit.append(real.__name__)
            return real(*a)
        return f
    monkeypatch.setattr(hostlib, "finish_bundle", misdirect(hostlib.finish_bundle, 7))
    monkeypatch.setattr(hostlib, "write_records", misdirect(hostlib.write_records, 4))
    res = {}
    for tag, extra in (("off", []), ("on", ["--device_merge"])):
        del hit[:]
        out = str(tmp_path / tag) + "/"
        rc = cli.main(["-d", d, "-o", out, "-S", "ecoli", "-F", fmt, "--gpus", "1", "--thread", "4"] + extra)
        assert hit and set(hit) == {"write_records" if extra else "finish_bundle"}, (tag, hit)
        files = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        res[tag] = (rc, files)
        assert files["failed_reads.txt"].split() == [b"s07.fast5"] and len(files) == 16, tag
        code, o = hostlib.load_fast5(os.path.join(d, "s07.fast5"), "Basecall_1D_000", "BaseCalled_template", True)
        assert code == hostlib.OK
        orig = hs.trim_fastq(o["fastq"])[0].encode() if fmt == "fastq" else np.asarray(o["bases"], "S1").tobytes()
        body = files[f"s07_out.{fmt}"].split(b"\n")[1].split(b"+")[0]
        assert len(body) > 1000 and body == orig                           # the file's own basecalls, unrevised
    assert res["on"][0] == res["off"][0] and res["on"][1] == res["off"][1]
