"""Read statistics computed on the device (MI355X only, -m gpu): csrc/nrv_stats.h through nrv_read_stats,
nrv_reads_raw_stats_begin / nrv_predict_reads_raw_stats and the command line's --device_stats.

Everything is compared BIT FOR BIT - nothing here has a tolerance:
  1. the five fixture reads against the goldens the reference's own signal_segmentation produced (shift, scale, per-base mean /
     std as uint64) and feature columns 1 - 2 against hoststage.read_tensors_raw (uint32), one read per call and all in one;
  2. synthetic reads against hoststage.median_mad / hoststage.event_stats (NumPy is the definition): empty bases, every base
     length 1 - 300, 1000, 5000, 20 000 (all three branches of the pairwise summation order, several levels of halving),
     reads of 1, 2, odd and even length, a half-integer median, a constant read (scale 0), the whole int16 range in one read
     (the global-memory histogram path) and ranges either side of the LDS limit, a read of 1 M samples;
  3. p1, p2, a1, a2 of the new call against nrv_predict_reads_raw fed by the host stage: E. coli and human weights, f16x2 /
     bf16x3 / f32, one call, two calls in flight, flagged and unflagged reads mixed in one call, and a read whose spikes trip
     the f16x2 range guard (the f32 re-run reads the device-written descriptors and feature columns);
  4. 1 and 3 again on handles created under NRV_POISON (quiet NaN, FLT_MAX, -1500.0f): the same bits, the guard silent;
  5. the command line with and without --device_stats, FASTA and FASTQ: the same bytes in every file.
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


def _bits_equal(got, want, what):
    """Bit equality; NaN is compared as NaN (the host's 0 / 0 and the device's differ in the sign bit only)."""
    got, want = np.asarray(got), np.asarray(want, got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions", int((gn != wn).sum()))
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    bad = np.nonzero((got.view(u) != want.view(u)) & ~gn)
    assert not len(bad[0]), (what, len(bad[0]), [b[:5].tolist() for b in bad], got[bad][:5].tolist(), want[bad][:5].tolist())


def _fixture(reads, key):
    g, rd, _ = reads(key)
    return g, rd, hs.read_tensors_raw(rd), int(rd.length[-1])


@pytest.fixture(scope="module")
def fixture_reads(reads):
    return [_fixture(reads, k) for k in reads.keys]


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


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------
def _golden_stats(rv, fixture_reads):
    """nrv_read_stats on the fixture reads, one per call and all five in one call -> [(name, array)]; checked on the way."""
    out = []
    one = [rv.read_stats([rr.raw], [rr.starts], [ld]) for _, _, rr, ld in fixture_reads]
    allin = rv.read_stats([rr.raw for _, _, rr, _ in fixture_reads], [rr.starts for _, _, rr, _ in fixture_reads],
                          [ld for _, _, _, ld in fixture_reads])
    e0 = 0
    for i, ((g, rd, rr, ld), (sh, sc, mean, std, f12)) in enumerate(zip(fixture_reads, one)):
        n = len(rr.starts)
        for tag, (sh2, sc2, mean2, std2, f2) in (("one", (sh[0], sc[0], mean, std, f12)),
                                                 ("all", (allin[0][i], allin[1][i], allin[2][e0:e0 + n], allin[3][e0:e0 + n], allin[4][e0:e0 + n]))):
            what = f"read {i} ({tag})"
            assert sh2 == float(g["seg_shift"]) and sc2 == float(g["seg_scale"]), (what, sh2, sc2)
            _bits_equal(mean2, np.asarray(g["seg_mean"], np.float64), what + " mean")
            _bits_equal(std2, np.asarray(g["seg_std"], np.float64), what + " std")
            _bits_equal(f2, rr.feat_ev[:, 1:3], what + " feat12")
        e0 += n
    for i, o in enumerate(one):
        out += [(f"stats one {i} {j}", np.asarray(x)) for j, x in enumerate(o)]
    out += [(f"stats all {j}", np.asarray(x)) for j, x in enumerate(allin)]
    return out


def test_fixture_reads_equal_the_reference_run_goldens(species_models, fixture_reads, monkeypatch):
    lens = np.concatenate([np.diff(rr.starts) for _, _, rr, _ in fixture_reads])
    assert (lens < 8).any() and ((lens >= 8) & (lens <= 128)).any() and (lens > 128).sum() >= 30 and lens.max() > 256   # every branch
    rv = _engine(monkeypatch, *species_models["ecoli"])
    _golden_stats(rv, fixture_reads)
    rv.close()


# ---- 2. synthetic -------------------------------------------------------------------------------------------------------------
def _events(rng, lengths, tail=1):
    """starts for bases of the given lengths, and the sample count: the last base is clipped to `tail` samples."""
    starts = np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int32)
    return starts, int(starts[-1]) + tail


def _synthetic_reads():
    rng = np.random.default_rng(1606)
    reads = {}
    lengths = np.concatenate([[0], np.arange(1, 301), [1000, 5000, 20_000], [0, 7, 8, 9, 127, 128, 129, 136, 255, 256, 257, 3]])
    rng.shuffle(lengths)
    st, L = _events(rng, lengths)
    reads["every length"] = (rng.normal(480, 90, L).round().clip(-32768, 32767).astype(np.int16), st, 3)
    lengths = rng.integers(3, 30, 500)
    st, L = _events(rng, lengths, tail=5)
    reads["last base unclipped, dur 5"] = (rng.normal(600, 40, L + 40).round().astype(np.int16), st, 5)
    for name, n in (("raw_len 1", 1), ("raw_len 2", 2), ("raw_len odd", 7), ("raw_len even", 8)):
        reads[name] = (rng.integers(300, 700, n).astype(np.int16), np.array([0, max(n - 1, 0)], np.int32)[: 2 if n > 1 else 1], 3)
    reads["half-integer median"] = (np.array([1, 2, 3, 4], np.int16), np.array([0, 2], np.int32), 5)
    reads["half-integer median, even count"] = (np.array([-3, 0, 1, 4, 9, 20], np.int16), np.array([0, 1, 1, 4], np.int32), 3)
    reads["half-integer MAD"] = (np.array([1, 2, 4, 9], np.int16), np.array([0, 3], np.int32), 3)
    reads["constant"] = (np.full(333, 412, np.int16), np.arange(0, 330, 11, dtype=np.int32), 3)
    wide = rng.normal(0, 9000, 30_000).round().clip(-32768, 32767).astype(np.int16)
    wide[[17, 29_000]] = [-32768, 32767]
    reads["whole int16 range"] = (wide, np.arange(0, 29_990, 9, dtype=np.int32), 3)
    reads["two values at the limits"] = (np.array([-32768, 32767, 32767, -32768, 32767], np.int16), np.array([0, 2, 5], np.int32), 3)
    for name, span in (("range 4096 (the LDS limit)", 4096), ("range 4097 (global)", 4097), ("range 3000", 3000)):
        x = rng.integers(-1000, -1000 + span, 50_000).astype(np.int16)
        x[:2] = [-1000, -1000 + span - 1]
        reads[name] = (x, np.arange(0, 49_000, 13, dtype=np.int32), 5)
    runs = np.repeat(rng.integers(450, 460, 4000), rng.integers(1, 40, 4000)).astype(np.int16)      # long runs of equal samples
    reads["runs of equal samples"] = (runs, np.arange(0, len(runs) - 5, 8, dtype=np.int32), 3)
    big = (rng.normal(500, 70, 1_000_000) + 40 * np.sin(np.arange(1_000_000) / 5000.0)).round().astype(np.int16)
    reads["1 M samples"] = (big, np.cumsum(rng.integers(2, 20, 95_000)).astype(np.int32), 5)
    return reads


def _expected(raw, starts, last_dur):
    sh, sc = hs.median_mad(raw)
    mean, std, sh2, sc2 = hs.event_stats(raw, starts, last_dur)
    assert sh == sh2 and sc == sc2
    with np.errstate(divide="ignore", invalid="ignore"):
        f12 = np.stack([(mean / sh).astype(np.float32), (std / sc).astype(np.float32)], axis=1)
    return float(sh), float(sc), mean, std, f12


def test_synthetic_reads_equal_numpy(species_models, monkeypatch):
    reads = _synthetic_reads()
    want = {k: _expected(*v) for k, v in reads.items()}
    assert want["half-integer median"][0] == 2.5 and want["constant"][1] == 0.0 and want["half-integer MAD"][:2] == (3.0, 1.5)
    assert np.isnan(want["every length"][2]).sum() == 2                 # the two empty bases
    assert np.isinf(want["constant"][4][:, 0]).sum() == 0 and np.isnan(want["constant"][4][:, 1]).all()
    rv = _engine(monkeypatch, *species_models["ecoli"])

    def check(names, got):
        e0 = 0
        for i, k in enumerate(names):
            sh, sc, mean, std, f12 = want[k]
            n = len(reads[k][1])
            assert got[0][i] == sh and got[1][i] == sc, (k, got[0][i], got[1][i], sh, sc)
            _bits_equal(got[2][e0:e0 + n], mean, k + " mean")
            _bits_equal(got[3][e0:e0 + n], std, k + " std")
            _bits_equal(got[4][e0:e0 + n], f12, k + " feat12")
            e0 += n
    for k, (raw, st, ld) in reads.items():
        check([k], rv.read_stats([raw], [st], [ld]))
    names = list(reads)                                                 # all in ONE call: long and short reads share the launches
    check(names, rv.read_stats([reads[k][0] for k in names], [reads[k][1] for k in names], [reads[k][2] for k in names]))
    check(names[::-1], rv.read_stats([reads[k][0] for k in names[::-1]], [reads[k][1] for k in names[::-1]], [reads[k][2] for k in names[::-1]]))
    # a read without samples cannot have a median: refused, as the host's median_mad_i16 does
    from nanoreviser_amd.engine import NrvError
    with pytest.raises(NrvError):
        rv.read_stats([np.zeros(0, np.int16)], [np.zeros(2, np.int32)], [3])
    check(["constant"], rv.read_stats([reads["constant"][0]], [reads["constant"][1]], [3]))     # the handle is fine afterwards
    rv.close()


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------
def _blind(rr):
    """The read as the device-statistics loader hands it over: statistics columns and shift / scale NOT filled in (NaN here:
    whatever is there must be ignored)."""
    feat = rr.feat_ev.copy()
    feat[:, 1:3] = np.nan
    return feat


def _calls(rv, fixture_reads, with_ref=True):
    """Every end-to-end form on the fixture reads -> [(name, array)] of the NEW calls; compared with the host-fed call inside."""
    T, out = rv.T, []
    rrs = [rr for _, _, rr, _ in fixture_reads]
    lds = [ld for _, _, _, ld in fixture_reads]

    def host(idx):
        return rv.pack_reads_raw([rrs[i].raw for i in idx], [rrs[i].starts for i in idx], [rrs[i].feat_ev for i in idx],
                                 [rrs[i].shift for i in idx], [rrs[i].scale for i in idx], T)

    def dev(idx, flags):
        p = rv.pack_reads_raw([rrs[i].raw for i in idx], [rrs[i].starts for i in idx],
                              [_blind(rrs[i]) if f else rrs[i].feat_ev for i, f in zip(idx, flags)],
                              [np.nan if f else rrs[i].shift for i, f in zip(idx, flags)],
                              [np.nan if f else rrs[i].scale for i, f in zip(idx, flags)], T)
        return rv.with_device_stats(p, [lds[i] for i in idx], flags)

    def same(ref, got, what):
        for j, (x, y) in enumerate(zip(ref, got)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, j, int((x != y).sum()))

    everyone = list(range(len(rrs)))
    ref_all = [x.copy() for x in rv.run_packed_raw(host(everyone))]
    got = rv.run_packed_raw(dev(everyone, [1] * len(rrs)))                      # one call, every read flagged
    same(ref_all, got, "one call")
    out += [(f"one call {j}", x.copy()) for j, x in enumerate(got)]
    a, b = everyone[:3], everyone[3:]                                           # two calls in flight
    ref_a, ref_b = [x.copy() for x in rv.run_packed_raw(host(a))], [x.copy() for x in rv.run_packed_raw(host(b))]
    ta, tb = rv.begin_packed_raw(dev(a, [1] * len(a))), rv.begin_packed_raw(dev(b, [1] * len(b)))
    got_a, got_b = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
    same(ref_a, got_a, "in flight, first")
    same(ref_b, got_b, "in flight, second")
    out += [(f"in flight a {j}", x.copy()) for j, x in enumerate(got_a)] + [(f"in flight b {j}", x.copy()) for j, x in enumerate(got_b)]
    tm, th = rv.begin_packed_raw(dev(everyone, [1, 0, 1, 0, 1])), rv.begin_packed_raw(host(b))   # mixed flags; a new and an old call in flight
    got_m, got_h = rv.end_packed_raw(tm), rv.end_packed_raw(th)
    same(ref_all, got_m, "flagged and unflagged reads in one call")
    same(ref_b, got_h, "old call behind a new one")
    out += [(f"mixed {j}", x.copy()) for j, x in enumerate(got_m)]
    got0 = rv.run_packed_raw(dev(everyone, [0] * len(rrs)))                     # no read flagged: the old call through the new entry
    same(ref_all, got0, "no read flagged")
    return out


@pytest.mark.parametrize("sp", ["ecoli", "human"])
def test_end_to_end_bit_identical_to_the_host_fed_call(species_models, fixture_reads, sp, monkeypatch):
    rv = _engine(monkeypatch, *species_models[sp])
    for mode in MODES:
        rv.set_precision(mode)
        _calls(rv, fixture_reads)
        assert rv.saturated() == (0, 0), (sp, mode)
    rv.close()


@pytest.mark.parametrize("sp", ["ecoli", "human"])
def test_range_guard_rerun_reads_the_device_written_statistics(species_models, fixture_reads, sp, monkeypatch):
    """Spikes at the int16 limits in a fixture read (the pattern of test_gpu_range.py): (32767 - median) / MAD is far outside
    the f16x2 range, so the call is re-run on the f32 kernels in nrv_reads_raw_end - over the slot's inputs, whose
    shift / scale and feature columns the device wrote."""
    _, _, rr, _ = fixture_reads[-1]
    N = 1500
    starts = rr.starts[:N].copy()
    raw = rr.raw[: int(starts[-1]) + 60].copy()
    rng = np.random.default_rng(11)
    pos = rng.choice(len(raw), 30, replace=False)
    raw[pos] = rng.choice(np.array([-32768, 32767], np.int16), 30)
    sh, sc, c1, c2 = hs.stats_columns(raw, starts, 3)
    assert (32767 - sh) / sc > 250                                          # beyond every model's static conv1 bound (93 - 212)
    feat = rr.feat_ev[:N].copy()
    feat[:, 1], feat[:, 2] = c1, c2
    blind = feat.copy()
    blind[:, 1:3] = np.nan
    other = fixture_reads[0][2]                                             # a clean read in the same call
    rv = _engine(monkeypatch, *species_models[sp])
    for mode in MODES:
        rv.set_precision(mode)
        r0 = rv.saturated()[1]
        ref = [x.copy() for x in rv.predict_reads_raw([other.raw, raw], [other.starts, starts], [other.feat_ev, feat],
                                                      [other.shift, sh], [other.scale, sc])]
        r1 = rv.saturated()[1]
        p = rv.pack_reads_raw([other.raw, raw], [other.starts, starts], [_blind(other), blind], [np.nan, np.nan], [np.nan, np.nan], rv.T)
        got = rv.run_packed_raw(rv.with_device_stats(p, [fixture_reads[0][3], 3], [1, 1]))
        r2 = rv.saturated()[1]
        assert (r1 - r0, r2 - r1) == ((1, 1) if mode == "f16x2" else (0, 0)), (mode, r0, r1, r2)
        for j, (x, y) in enumerate(zip(ref, got)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (sp, mode, j, int((x != y).sum()))
    rv.close()


# ---- 4. poison ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", ["ecoli", "human"])
@pytest.mark.parametrize("mode", MODES)
def test_poisoned_workspace_gives_the_same_bits(species_models, fixture_reads, sp, mode, monkeypatch):
    """Histograms, min / max and counters are zeroed by the call itself, on its stream: a handle whose every buffer holds a
    pattern gives the clean handle's bits, on a first and on a second pass, and the range guard stays silent."""
    clean = _engine(monkeypatch, *species_models[sp], precision=mode)
    ref = _golden_stats(clean, fixture_reads) + _calls(clean, fixture_reads)
    assert clean.saturated() == (0, 0)
    clean.close()
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models[sp], poison=poison, precision=mode)
        for p in range(2):
            got = _golden_stats(rv, fixture_reads) + _calls(rv, fixture_reads)
            assert [k for k, _ in got] == [k for k, _ in ref]
            for (k, x), (_, y) in zip(ref, got):
                assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (sp, mode, poison, p, k)
        assert rv.saturated() == (0, 0), (sp, mode, poison)
        rv.close()


# ---- 5. command line ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_command_line_writes_the_same_bytes_with_and_without_the_switch(tmp_path, monkeypatch, fmt):
    from nanoreviser_amd.engine import Reviser
    monkeypatch.delenv("NRV_DEVICE_STATS", raising=False)
    monkeypatch.delenv("NRV_CLI_PIPELINE", raising=False)
    monkeypatch.delenv("NRV_CLI_ENGINES", raising=False)
    forms = []
    real = Reviser.begin_packed_raw
    monkeypatch.setattr(Reviser, "begin_packed_raw", lambda self, packed: forms.append(len(packed)) or real(self, packed))
    # the fixture directory as it is (two reads: no parser pool, so both runs are fed by the host), and all five fixture reads
    # several times over with a parser pool, where the switch takes the new calls
    big = tmp_path / "in"
    big.mkdir()
    src = sorted(glob.glob(os.path.join(FAST5, "*.fast5")) + glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))
    for i in range(15):
        shutil.copy(src[i % len(src)], big / f"s{i:02d}.fast5")
    monkeypatch.setenv("NRV_CLI_GROUPS", "4")                                # a few reads per device call: several calls in flight
    for tag, d, pooled in (("fixture", FAST5, False), ("pooled", str(big), True)):
        outs = {}
        for sw in ("off", "on"):
            del forms[:]
            out = str(tmp_path / f"{tag}_{sw}") + "/"
            argv = ["-d", d, "-o", out, "-S", "ecoli", "-F", fmt, "--gpus", "1", "--thread", "4"] + (["--device_stats"] if sw == "on" else [])
            assert cli.main(argv) == 0
            outs[sw] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
            assert "failed_reads.txt" in outs[sw] and outs[sw]["failed_reads.txt"] == b""
            if pooled:
                assert forms and set(forms) == ({9} if sw == "on" else {7}), (sw, forms)
            else:
                assert 9 not in forms
        assert outs["on"] == outs["off"] and len(outs["on"]) == (16 if pooled else 3)
