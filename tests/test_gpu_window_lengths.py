"""Everything behind the model graph at window lengths other than the shipped 11 (MI355X only, -m gpu): T = 1, 2, 12, 13, 32
(tests/window_cases.py says why these), weights `with_window(T)` of the shipped pairs.

Everything is compared BIT FOR BIT / BYTE FOR BYTE - nothing here has a tolerance.  The host definitions are the reference
(tests/test_window_lengths_host.py holds them to the rule text at the same T):
  3. the kernels alone on host-supplied calls, one handle per T, a FASTA and a FASTQ pass on it: nrv_merge_calls on the merge
     test's synthetic calls built at T; nrv_merge_calls_report and nrv_merge_calls_edits (with and without the report) on
     report_case(T) and the three density cases, each checked to hold what it claims (window_cases.check_case_holds); the
     caller's edit records at and beyond the total untouched; at T = 12 the call of 257 * 256 + 3 events (the tile scan's carry);
  4. raw reads end to end: ONE call of the shorter short read, slices of T - 1, T, T + 1 and 1 events, and the second short read
     - reads without a window inside a call that has windows, straddling windows at every boundary - through the full call
     (merge + report + edits + records), FASTA and FASTQ, with and without device statistics, reads handed back or not, two calls
     in flight, N = T and N = T - 1; f16x2 at every T, f32 and bf16x3 at T = 1 and 32, the human pair at T = 13; the range guard
     at T = 32 (one re-run, the f32 mode's results); NRV_POISON (quiet NaN) at T = 1 and 32: the clean handle's bytes on a first
     and on a second pass - a read of an unwritten halo row would show here;
  5. read mode across stages and launch groups at T = 1 and 32: the five fixture reads in one nrv_predict_reads_raw call (more
     than 2 x 16 384 windows) against nrv_predict_read on the device-cut events, against nrv_predict on five slices of 600
     windows, and against a handle with ragged groups of 1000 windows.
"""
import numpy as np
import pytest

from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from edits_cases import carry_case
from report_cases import TIE_EPS
from test_gpu_device_merge import _expected, _same_merged, _synthetic_calls, fixture_reads  # noqa: F401 (fixture_reads: a fixture)
from test_gpu_device_report import short_reads  # noqa: F401 (a fixture)
from window_cases import T_SET, calls_cases, check_case_holds

pytestmark = pytest.mark.gpu

QNAN = 0x7FC00000


def _make(species_models, T, sp="ecoli", poison=None, coalesce=None, **kw):
    """A handle at window length T: the shipped pair with `with_window(T)`; the environment is read by nrv_create."""
    from nanoreviser_amd.engine import Reviser
    m1, m2 = species_models[sp]
    with pytest.MonkeyPatch.context() as mp:
        for k in ("NRV_PRECISION", "NRV_COALESCE", "NRV_LANES", "NRV_POISON"):
            mp.delenv(k, raising=False)
        if poison is not None:
            mp.setenv("NRV_POISON", f"{poison:08x}")
        if coalesce is not None:
            mp.setenv("NRV_COALESCE", coalesce)
        rv = Reviser(m1.with_window(T), m2.with_window(T), **kw)
    assert rv.T == T
    return rv


@pytest.fixture(scope="module")
def engines(species_models):
    """One clean handle per (T, species), shared by the tests of this file and closed behind them."""
    made = {}

    def get(T, sp="ecoli"):
        if (T, sp) not in made:
            made[(T, sp)] = _make(species_models, T, sp)
        return made[(T, sp)]
    yield get
    for rv in made.values():
        rv.close()


# ---- 3. the kernels alone ----------------------------------------------------------------------------------------------------------
def _same_edits(got, want, what):
    assert got[0].dtype == hs.EDIT_DTYPE and np.array_equal(got[1], want[1]), (what, got[1].tolist()[:8], want[1].tolist()[:8])
    assert len(got[0]) == int(want[1][-1]) and got[0].tobytes() == want[0].tobytes(), (what, np.flatnonzero(got[0] != want[0])[:4].tolist())
    whole = got[0].base if got[0].base is not None else got[0]          # the caller's block: zeros behind the total, as handed over
    assert not whole.view(np.uint8).reshape(-1)[16 * int(want[1][-1]):].any(), what


def _kernels_on_case(rv, c, T, fastq, what):
    """nrv_merge_calls_report and nrv_merge_calls_edits (with and without the report) on one calls case against the definitions."""
    thr = cli.phred_thresholds()
    n = len(c["a1"])
    ins = (c["bases"], c["ev_len"], c["a1"], c["a2"])
    qc = cli.phred_lookup(np.minimum(c["p1"][np.arange(n), np.clip(c["a1"], 0, 5)], c["p2"][np.arange(n), np.clip(c["a2"], 0, 4)]))
    forms = {"fastq": (c["p1"], c["p2"], thr, qc)} if fastq else {"rows": (c["p1"], c["p2"], None, None), "bare": (None, None, None, None)}
    for form, (p1, p2, q, qcf) in forms.items():
        merged = hs.emit_calls(*ins, qcf, T)
        rep = hs.revision_report(*ins, p1, p2, qcf, T, TIE_EPS)
        edits = hs.revision_edits(*ins, p1, p2, qcf, T)
        got = rv.merge_calls_report_device(*ins, p1, p2, q, TIE_EPS)
        _same_merged(got[:3], merged, (what, form, "report: merged"))
        assert got[3].dtype == np.uint64 and np.array_equal(got[3], rep), (what, form, np.argwhere(got[3] != rep)[:8].tolist())
        for report in (True, False):
            got = rv.merge_calls_edits_device(*ins, p1, p2, q, TIE_EPS, report=report)
            _same_merged(got[:3], merged, (what, form, report, "edits: merged"))
            assert (got[3] is None) if not report else np.array_equal(got[3], rep), (what, form, report)
            _same_edits(got[4:], edits, (what, form, report))


@pytest.mark.parametrize("T", T_SET)
def test_kernels_alone_equal_the_definitions(engines, T):
    rv = engines(T)
    thr = cli.phred_thresholds()
    synth = _synthetic_calls(T)
    seen = set()
    for c in synth.values():
        seen |= set(hs.merge_calls(c["bases"][(T - 1) // 2:][:len(c["a1"])], c["a1"], c["a2"])[2].tolist())
    assert seen == {0, 1, 2}
    cases = dict(calls_cases(T))
    for name, c in cases.items():
        print(f"T={T} {name}: {check_case_holds(name, c, T)}")
    if T == 12:
        cases["carry"] = carry_case(False, T=T)                          # crosses the tile scan's carry once at an even T
        assert (cases["carry"]["N"] + 255) // 256 > 256
    for fastq in (False, True):                                          # two passes on the one handle
        for name, c in synth.items():
            if fastq and "no quality" in name:
                continue
            got = rv.merge_calls_device(c["bases"], c["ev_len"], c["a1"], c["a2"], *((c["p1"], c["p2"], thr) if fastq else ()))
            _same_merged(got, _expected(c, T, fastq), (T, name, fastq))
            if name == "all two characters":
                assert len(got[0]) == int(c["ev_len"].sum()) + len(c["a1"])          # the capacity N + (N - T), exactly
            if name == "all drop":
                assert len(got[0]) == int(np.minimum(c["ev_len"], T).sum())            # the kept ends of every read
        for name, c in cases.items():
            _kernels_on_case(rv, c, T, fastq, (T, name))
    assert rv.saturated() == (0, 0)


# ---- 4. end to end on raw reads ----------------------------------------------------------------------------------------------------
class _Rd:
    """One read of a raw call: samples, starts, features, bases, shift / scale, the samples of its last base and whether the
    device may compute its statistics (a slice keeps the whole read's: its own would differ)."""

    def __init__(self, rr, ld, k=None):
        self.stats = k is None
        if k is None:
            k = len(rr.starts)
        self.raw = rr.raw if self.stats else rr.raw[:int(rr.starts[k])]          # the samples up to the slice's end
        self.starts, self.feat_ev, self.bases = rr.starts[:k], rr.feat_ev[:k], np.asarray(rr.bases, "S1")[:k]
        self.shift, self.scale, self.ld = rr.shift, rr.scale, (ld if self.stats else 0)


def _call_reads(short_reads, T):
    (a, lda), (b, ldb) = short_reads
    return [_Rd(a, lda)] + [_Rd(b, ldb, k) for k in (T - 1, T, T + 1, 1)] + [_Rd(b, ldb)]


def _names(k):
    return [b"r%d|||x" % i + b"y" * i for i in range(k)]


def _args(rds, blind=False):
    feats = []
    for r in rds:
        f = r.feat_ev
        if blind and r.stats:
            f = f.copy()
            f[:, 1:3] = np.nan
        feats.append(f)
    nan = [blind and r.stats for r in rds]
    return ([r.raw for r in rds], [r.starts for r in rds], feats, [np.nan if x else r.shift for x, r in zip(nan, rds)],
            [np.nan if x else r.scale for x, r in zip(nan, rds)])


def _b8(rds):
    return np.concatenate([r.bases for r in rds] + [np.zeros(0, "S1")]).view(np.uint8)


def _definition(rv, rds, names):
    """fastq -> (report, seq, qual, off, edits, edit_off, blob, rec_off): nrv_predict_reads_raw on this handle, then the definitions."""
    p1, p2, a1, a2 = rv.predict_reads_raw(*_args(rds))
    el, b, T = [len(r.starts) for r in rds], _b8(rds), rv.T
    assert len(a1) == max(sum(el) - T, 0)
    out = {}
    for fastq in (False, True):
        qc = (cli.phred_chars(p1, p2, a1, a2) if len(a1) else np.zeros(0, np.uint8)) if fastq else None
        merged = tuple(hs.emit_calls(b, el, a1, a2, qc, T))
        out[fastq] = (hs.revision_report(b, el, a1, a2, p1, p2, qc, T, TIE_EPS),) + merged + tuple(hs.revision_edits(b, el, a1, a2, p1, p2, qc, T)) \
            + tuple(hs.pack_records(names, *merged))
    return out


def _packed(rv, rds, names, fastq, stats=False, hand_back=True):
    p = rv.pack_reads_raw(*_args(rds, blind=stats), rv.T)
    if stats:
        p = rv.with_device_stats(p, [r.ld for r in rds], [1 if r.stats else 0 for r in rds])
    p = rv.with_device_edits(rv.with_device_report(rv.with_device_merge(p, _b8(rds), fastq), TIE_EPS))
    p = rv.with_device_records(p, names, hand_back=hand_back)
    assert len(p) == 20
    p[14].view(np.uint8)[:] = 0xA5                                        # what the call does not write stays
    p[18][:] = 0xA5
    return p


def _check_call(got, want, what, packed, hand_back=True):
    seq, qual, off, rep, ed, edit_off, blob, rec_off = got
    assert np.array_equal(off, want[3]), what
    if hand_back:
        assert np.array_equal(seq, want[1]), (what, len(seq), len(want[1]))
        assert (qual is None) == (want[2] is None) and (qual is None or np.array_equal(qual, want[2])), what
    else:
        assert seq is None and qual is None, what
    assert rep.dtype == np.uint64 and np.array_equal(rep, want[0]), (what, np.argwhere(rep != want[0])[:8].tolist())
    assert np.array_equal(edit_off, want[5]) and ed.tobytes() == want[4].tobytes(), what
    assert np.array_equal(rec_off, want[7]) and blob.tobytes() == want[6].tobytes(), what
    rest = packed[14].view(np.uint8).reshape(-1, 16)[int(edit_off[-1]):]
    assert (rest == 0xA5).all() and (packed[18][int(rec_off[-1]):] == 0xA5).all(), what


def _end_to_end(rv, short_reads):
    """Every end-to-end form at the handle's T -> [(name, array)] of what came back; compared with the definition inside."""
    T, out = rv.T, []
    rds = _call_reads(short_reads, T)
    names = _names(len(rds))
    el = [len(r.starts) for r in rds]
    assert el[1:5] == [T - 1, T, T + 1, 1] and min(el[0], el[5]) > 4096
    want = _definition(rv, rds, names)
    halves = [(rds[:3], names[:3]), (rds[3:], names[3:])]
    want_half = [_definition(rv, r, n) for r, n in halves]
    n_win = sum(el) - T
    owned = sum(max(x - T, 0) for x in el)
    print(f"T={T} end to end: events {sum(el)}, windows {n_win}, straddling {n_win - owned}, edits {int(want[True][5][-1])}, "
          f"inserted {int(want[True][0][:, 6].sum())}, deleted {int(want[True][0][:, 7].sum())}, substituted {int(want[True][0][:, 5].sum())}")
    assert n_win - owned > 0 and want[True][5][-1] > 0 and want[False][5][-1] > 0     # an empty list cannot pass for a correct one
    for fastq in (False, True):
        for stats in (False, True):
            for back in (True, False):
                p = _packed(rv, rds, names, fastq, stats, back)
                got = rv.run_packed_raw(p)
                _check_call(got, want[fastq], (T, "one call", fastq, stats, back), p, back)
                out += [(f"one call {fastq} {stats} {back} {j}", x.copy()) for j, x in enumerate(got) if x is not None]
        # two calls in flight
        pa, pb = _packed(rv, *halves[0], fastq), _packed(rv, *halves[1], fastq, stats=True, hand_back=False)
        ta, tb = rv.begin_packed_raw(pa), rv.begin_packed_raw(pb)
        ga, gb = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
        _check_call(ga, want_half[0][fastq], (T, "in flight, first", fastq), pa)
        _check_call(gb, want_half[1][fastq], (T, "in flight, second", fastq), pb, False)
        out += [(f"in flight {fastq} {j}", x.copy()) for j, x in enumerate(gb) if x is not None]
        # N = T and N = T - 1: no window at all, everything is filled on the host
        (b, ldb) = short_reads[1]
        for N in sorted({T, T - 1} - {0}):
            two = [_Rd(b, ldb, N - N // 2), _Rd(b, ldb, N // 2)]
            p = _packed(rv, two, _names(2), fastq)
            p[15][:], p[19][:] = -1, -1
            seq, qual, off, rep, ed, edit_off, blob, rec_off = rv.run_packed_raw(p)
            b8, z = _b8(two), np.zeros(0, np.int8)
            assert seq.tobytes() == b8.tobytes() and off.tolist() == [0, N - N // 2, N] and (qual.tobytes() == b"#" * N if fastq else qual is None)
            assert np.array_equal(rep, hs.revision_report(b8, [N - N // 2, N // 2], z, z, None, None, np.zeros(0, np.uint8) if fastq else None, T))
            assert len(ed) == 0 and edit_off.tolist() == [0, 0, 0]
            w = hs.pack_records(_names(2), b8, np.full(N, ord("#"), np.uint8) if fastq else None, off)
            assert blob.tobytes() == w[0].tobytes() and np.array_equal(rec_off, w[1]) and (p[18][int(rec_off[-1]):] == 0xA5).all()
    return out


@pytest.mark.parametrize("T", T_SET)
def test_raw_reads_end_to_end_equal_the_definitions(engines, short_reads, T):
    rv = engines(T)
    for mode in ["f16x2"] + (["f32", "bf16x3"] if T in (1, 32) else []):
        rv.set_precision(mode)
        _end_to_end(rv, short_reads)
        assert rv.saturated() == (0, 0), (T, mode)
    rv.set_precision("f16x2")


def test_raw_reads_end_to_end_on_the_human_pair(engines, short_reads):
    rv = engines(13, "human")
    _end_to_end(rv, short_reads)
    assert rv.saturated() == (0, 0)


@pytest.mark.parametrize("T", [32, 1])
def test_poisoned_workspace_gives_the_same_bytes(engines, species_models, short_reads, T):
    """A handle whose every buffer holds quiet NaNs gives the clean handle's bytes, twice, with the range guard silent."""
    clean = engines(T)
    clean.set_precision("f16x2")
    ref = _end_to_end(clean, short_reads)
    rv = _make(species_models, T, poison=QNAN)
    for p in range(2):
        got = _end_to_end(rv, short_reads)
        assert [k for k, _ in got] == [k for k, _ in ref]
        for (k, x), (_, y) in zip(ref, got):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (T, p, k)
    assert rv.saturated() == (0, 0) and clean.saturated() == (0, 0)
    rv.close()


def test_range_guard_rerun_at_the_largest_window_length(species_models, short_reads):
    """The spiked read of test_gpu_combined_records.py::test_range_guard_rerun_gives_the_f32_records behind a clean one, at T = 32:
    exactly one re-run per call, and report, edits, blob and rec_off are the f32 mode's."""
    T = 32
    other, _ = short_reads[0]
    rr, _ = short_reads[1]
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
    bases = np.concatenate([np.asarray(other.bases, "S1"), np.asarray(rr.bases, "S1")[:N]])
    args = ([other.raw, raw], [other.starts, starts], [other.feat_ev, feat], [other.shift, sh], [other.scale, sc])
    rv = _make(species_models, T)
    rv.set_precision("f32")
    p1, p2, a1, a2 = rv.predict_reads_raw(*args)
    el, b8 = [len(other.starts), N], bases.view(np.uint8)
    want = {}
    for fq in (False, True):
        qc = cli.phred_chars(p1, p2, a1, a2) if fq else None
        merged = tuple(hs.emit_calls(b8, el, a1, a2, qc, T))
        want[fq] = (hs.revision_report(b8, el, a1, a2, p1, p2, qc, T, TIE_EPS),) + merged + tuple(hs.revision_edits(b8, el, a1, a2, p1, p2, qc, T)) \
            + tuple(hs.pack_records(_names(2), *merged))
    assert rv.saturated()[1] == 0
    rv.set_precision("f16x2")
    for fq in (False, True):
        r0 = rv.saturated()[1]
        p = rv.with_device_edits(rv.with_device_report(rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, fq), TIE_EPS))
        p = rv.with_device_records(p, _names(2))
        p[14].view(np.uint8)[:] = 0xA5
        p[18][:] = 0xA5
        got = rv.run_packed_raw(p)
        assert rv.saturated()[1] - r0 == 1, fq
        _check_call(got, want[fq], ("re-run", fq), p)
        assert got[3][:, 1].tolist() == [el[0] - T, N - T]
    rv.close()


# ---- 5. read mode across stages and launch groups ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 32])
def test_read_mode_across_stages_and_groups(engines, species_models, fixture_reads, T):
    """The five fixture reads in ONE nrv_predict_reads_raw call: three stages of 16 384 windows (each with its T - 1 event halo),
    ten launch groups.  The windows are never materialised whole on the host: five slices of 600 go through nrv_predict."""
    rrs = [r for r, _ in fixture_reads]
    args = ([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs], [r.shift for r in rrs], [r.scale for r in rrs])
    rv = engines(T)
    rv.set_precision("f16x2")
    out = [x.copy() for x in rv.predict_reads_raw(*args)]
    n = len(out[2])
    assert len(rrs) == 5 and n == sum(len(r.starts) for r in rrs) - T and n > 2 * 16384 + 600
    sig = rv.segment_reads(*args[:2], *args[3:])
    feat = np.concatenate(args[2])
    for j, (x, y) in enumerate(zip(out, rv.predict_read(sig, feat))):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (T, "nrv_predict_read", j)
    for s in (0, 4096 - 300, 16384 - 300, 32768 - 300, n - 600):
        sw, fw = hs.sliding_windows(sig[s:s + 600 + T], feat[s:s + 600 + T], T)
        assert len(fw) == 600
        for j, (x, y) in enumerate(zip(out, rv.predict_pair(np.ascontiguousarray(sw), np.ascontiguousarray(fw)))):
            assert x[s:s + 600].tobytes() == y.tobytes(), (T, "nrv_predict", s, j)
    assert rv.saturated() == (0, 0)
    ragged = _make(species_models, T, coalesce="0", batch=1000)           # groups of 1000 windows on one stream, a ragged tail
    assert ragged.batch == 1000
    for j, (x, y) in enumerate(zip(out, ragged.predict_reads_raw(*args))):
        assert x.tobytes() == y.tobytes(), (T, "batch 1000", j)
    assert ragged.saturated() == (0, 0)
    ragged.close()
