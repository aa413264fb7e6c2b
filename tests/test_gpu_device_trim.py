"""Sliding-window quality trimming and the length filter on the device (MI355X only, -m gpu): csrc/nrv_trim.h and the trimmed
records of csrc/nrv_pack.h through nrv_trim_reads, nrv_pack_records_trim, nrv_merge_calls_trim, nrv_revise_reads_raw_trim_begin /
nrv_revise_reads_raw_trim and the command line's --trim_q.

Everything is compared BIT FOR BIT - the rule is integers only, nothing here has a tolerance.  hoststage.trim_bounds and
hoststage.pack_records are the definitions (tests/test_trim_host.py holds them to the rule text).  The shipped E. coli weights:
  1. nrv_trim_reads on tests/trim_cases.py's planted qualities, W = 1, 2, 10, 64: read lengths around W and around the tile of 256,
     300 reads of 3, one read of 70 000, the only good window at 0, at L - W and across a tile edge, a window that is good only by
     reaching into the next read, sums exactly at and one below the bar, all bad, all 40; two passes over the same handle;
  2. nrv_pack_records_trim, FASTA and FASTQ: dropped reads first, last, three in a row, all of them, lo = hi, min_len 0 and 1,
     against hoststage.pack_records; trim NULL: nrv_pack_records' bytes;
  3. nrv_merge_calls_trim on profile_case and report_case(T) at T = 1, 2, 11, 32, with and without q_thr and with a q_thr that is
     not trim_thr, against cli.trim_rows; seq / qual / off are nrv_merge_calls'; the trimmed records behind the same call;
  4. nrv_revise_reads_raw_trim on the two shortest fixture reads in one call, in each precision mode, FASTA and FASTQ, with and
     without device statistics, report, edit list, records and profile, against the definition on nrv_predict_reads_raw's outputs
     in that mode; every other output is that of the same call without the trim, the blob being pack_records(..., trim); Q = 3,
     W = 4, both reads with 0 < lo < hi < L; and a min_len that drops exactly the shorter read;
  5. two calls in flight; a call that trips the f16x2 range guard (one re-run, the f32 mode's bounds); handles under NRV_POISON; a
     call with N <= T (filled on the host);
  6. the command line with --device_merge --trim_q, with and without --combined: form 27, files and --trim_log those of the host route.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from profile_cases import profile_case, window_qc
from records_cases import name_lengths_case, names_for, tiny_reads_case
from report_cases import T, report_case
from trim_cases import WINDOWS, planted_cases

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "bf16x3", "f32"]
PATTERNS = {"qnan": 0x7FC00000, "m1500": 0xC4BB8000}
FAST5 = os.path.join(GOLD, "fast5")
INNER = ["merge", "report", "edits", "records", "records_only", "profile", "all"]    # what the call carries beside the trim
Q, W = 3, 4


def _engine(monkeypatch, m1, m2, poison=None, Tw=T, **kw):
    from nanoreviser_amd.engine import Reviser
    if poison is None:
        monkeypatch.delenv("NRV_POISON", raising=False)
    else:
        monkeypatch.setenv("NRV_POISON", f"{PATTERNS[poison]:08x}")
    for k in ("NRV_PRECISION", "NRV_COALESCE", "NRV_LANES"):
        monkeypatch.delenv(k, raising=False)
    rv = Reviser(m1.with_window(Tw), m2.with_window(Tw), **kw) if Tw != T else Reviser(m1, m2, **kw)
    monkeypatch.delenv("NRV_POISON", raising=False)
    assert rv.T == Tw
    return rv


@pytest.fixture(scope="module")
def short_reads(reads):
    """The two shortest fixture reads as (RawReadTensors, samples of the last base)."""
    out = []
    for k in reads.keys:
        _, rd, _ = reads(k)
        out.append((hs.read_tensors_raw(rd), int(rd.length[-1])))
    return sorted(out, key=lambda x: len(x[0].starts))[:2]


def _same(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8].tolist(), got[got != want][:8].tolist(), want[got != want][:8].tolist())


def _eq(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


# ---- 1. the window kernel on planted qualities -------------------------------------------------------------------------------------
@pytest.mark.parametrize("Wp", WINDOWS)
def test_trim_reads_on_planted_qualities(species_models, monkeypatch, Wp):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    cases = planted_cases(Wp)
    wants = {name: hs.trim_bounds(qual, off, Qp, Wp) for name, (qual, off, Qp) in cases.items()}
    L = 2 * 256 + 77
    assert wants["only window at 0"].tolist() == [[0, 0], [0, Wp], [0, 0]]
    assert wants["only window at L - W"].tolist() == [[0, 0], [L - Wp, L], [0, 0]]
    assert wants["only window across a tile edge"].tolist() == [[0, 0], [155, 155 + Wp], [0, 0]]
    assert wants["sum exactly Q W"].tolist() == [[7, 7 + Wp], [0, 0]] and not wants["lengths, all bad"].any()
    assert wants["70000 in one read"][1, 0] > 0 and wants["70000 in one read"][1, 1] > 60000
    if Wp > 1:
        assert not wants["window reaching into the next read"].any() and not wants["window reaching into the next read over a tile edge"].any()
    for p in range(2):                                                   # a second pass over the same handle: the same bounds
        for name, (qual, off, Qp) in cases.items():
            _same(rv.trim_reads(qual, off, Qp, Wp), wants[name], (Wp, name, p))
    # every bar on one input
    qual, off, _ = cases["lengths, random"]
    for Qp in (1, 17, 40):
        _same(rv.trim_reads(qual, off, Qp, Wp), hs.trim_bounds(qual, off, Qp, Wp), (Wp, "bar", Qp))
    from nanoreviser_amd import engine as E
    for bad_q, bad_w in ((0, Wp), (41, Wp), (3, 0), (3, 65)):            # the C entry point refuses them under its own name
        with pytest.raises(E.NrvError, match="nrv_trim_reads"):
            rv._check(rv._lib.nrv_trim_reads(*E._marshal((rv._h, qual, off, off.size - 1, bad_q, bad_w, np.zeros((off.size - 1, 2), np.int64)),
                                                         E._TRIM_READS_T)))
    rv.close()


# ---- 2. the trimmed records --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fastq", [False, True])
def test_pack_records_trim_equals_the_definition(species_models, monkeypatch, fastq):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rng = np.random.default_rng(29)
    for case in (name_lengths_case(fastq), tiny_reads_case(fastq)):
        names, seq, qual, off = case["names"], case["seq"], case["qual"], case["off"]
        R, L = len(names), np.diff(case["off"])
        blob, rec_off = rv.pack_records_trim(names, seq, qual, off, None)
        plain = rv.pack_records_device(names, seq, qual, off)
        assert blob.tobytes() == plain[0].tobytes() == hs.pack_records(names, seq, qual, off)[0].tobytes() and np.array_equal(rec_off, plain[1])
        for drop in ((), (0,), (R - 1,), (3, 4, 5), (0, 1, 2, 7, 8, 9, R - 3, R - 2, R - 1), tuple(range(0, R, 2)), tuple(range(R))):
            lo = (rng.random(R) * (L + 1)).astype(np.int64)
            hi = lo + (rng.random(R) * (L - lo + 1)).astype(np.int64)
            t = np.stack([lo, hi], 1)
            t[list(drop)] = 0                                           # lo = hi = 0
            for min_len in (0, 1, 7):
                blob, rec_off = rv.pack_records_trim(names, seq, qual, off, t, min_len)
                want, want_off = hs.pack_records(names, seq, qual, off, t, min_len)
                assert np.array_equal(rec_off, want_off), (len(drop), min_len)
                assert blob.tobytes() == want.tobytes(), (len(drop), min_len)
                if min_len == 0:
                    assert (np.diff(rec_off) >= 3).all()                # lo = hi: an empty record, kept
                elif len(drop) == R:
                    assert rec_off[-1] == 0 and blob.size == 0          # all of them dropped
    rv.close()


# ---- 3. the three launches behind the merge ---------------------------------------------------------------------------------------
def _in_range(c):
    """The case with its labels clipped into range: what cli.trim_rows (phred_chars gathers the class as it is) can be given."""
    d = dict(c)
    d["a1"], d["a2"] = np.clip(c["a1"], 0, 5).astype(np.int8), np.clip(c["a2"], 0, 4).astype(np.int8)
    return d


def _merge_trim_checks(rv, c, Tw, rules):
    thr = cli.phred_thresholds()
    other = np.linspace(0.05, 0.95, 39).astype(np.float32)               # a q_thr that is not trim_thr: qual changes, the trim does not
    names = names_for(len(c["ev_len"]))
    for d, by_rows in ((c, False), (_in_range(c), True)):
        ins = (d["bases"], d["ev_len"], d["a1"], d["a2"], d["p1"], d["p2"])
        seq_w, qual_w, off_w = hs.emit_calls(d["bases"], d["ev_len"], d["a1"], d["a2"], window_qc(d), Tw)
        for Qp, Wp in rules:
            want = hs.trim_bounds(qual_w, off_w, Qp, Wp)
            if by_rows:
                _same(cli.trim_rows(Tw, *ins[:2], d["p1"], d["p2"], d["a1"], d["a2"], Qp, Wp), want, "trim_rows is the definition")
            for q_thr in (thr, None, other):
                seq, qual, off, trim = rv.merge_calls_trim(*ins, Qp, Wp, q_thr=q_thr)
                _same(trim, want, (Tw, Qp, Wp, by_rows, q_thr is None))
                m = rv.merge_calls_device(*ins, q_thr)
                assert np.array_equal(seq, m[0]) and _eq(qual, m[1]) and np.array_equal(off, m[2])
            for q_thr in (thr, None):                                    # the trimmed records behind the same call
                for min_len in (1, 40):
                    seq, qual, off, trim, blob, rec_off = rv.merge_calls_trim(*ins, Qp, Wp, q_thr=q_thr, names=names, min_len=min_len)
                    _same(trim, want, "with records")
                    wb, wo = hs.pack_records(names, seq, qual, off, want, min_len)
                    assert np.array_equal(rec_off, wo) and blob.tobytes() == wb.tobytes(), (Tw, Qp, Wp, min_len)
            yield want


def test_merge_calls_trim_equals_the_definition(species_models, monkeypatch):
    c = profile_case()
    rv = _engine(monkeypatch, *species_models["ecoli"])
    wants = list(_merge_trim_checks(rv, c, T, ((2, 4), (3, 10), (9, 2), (2, 64))))
    assert any((w[:, 1] > w[:, 0]).any() and (w[:, 1] == 0).any() for w in wants)       # kept reads and reads without a good window
    assert any(((w[:, 0] > 0) & (w[:, 1] > w[:, 0])).any() for w in wants)
    # no window at all: filled on the host, every quality 2
    z = np.zeros(0, np.int8)
    e6, e5 = np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32)
    for Qp, Wp, want in ((2, 4, [[0, 5], [0, 0], [0, 4]]), (3, 4, [[0, 0]] * 3), (2, 5, [[0, 5], [0, 0], [0, 0]]), (1, 1, [[0, 5], [0, 0], [0, 4]])):
        out = rv.merge_calls_trim(c["bases"][:9], [5, 0, 4], z, z, e6, e5, Qp, Wp, q_thr=cli.phred_thresholds(), names=[b"a", b"b", b"c"])
        assert out[3].tolist() == want == hs.trim_bounds(np.full(9, 35, np.uint8), out[2], Qp, Wp).tolist()
        wb, wo = hs.pack_records([b"a", b"b", b"c"], out[0], out[1], out[2], out[3], 1)
        assert out[4].tobytes() == wb.tobytes() and np.array_equal(out[5], wo)
    from nanoreviser_amd import engine as E
    ins = rv._merge_inputs(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], None, True)
    for bad in ((0, 4), (41, 4), (3, 0), (3, 65)):                       # the C entry point refuses them under its own name
        more = E._marshal((cli.phred_thresholds(), bad[0], bad[1], 1, np.zeros((len(c["ev_len"]), 2), np.int64), None, None, None, None),
                          E._TRIM[0] + E._RECORDS[0])
        with pytest.raises(E.NrvError, match="nrv_merge_calls_trim"):
            rv._merge_call("nrv_merge_calls_trim", *ins, *more)
    rv.close()


@pytest.mark.parametrize("Tw", [1, 2, 32])
def test_merge_calls_trim_at_other_window_lengths(species_models, monkeypatch, Tw):
    c = report_case(T=Tw)
    rv = _engine(monkeypatch, *species_models["ecoli"], Tw=Tw)
    wants = list(_merge_trim_checks(rv, c, Tw, ((2, 4), (3, 2))))
    assert any((w[:, 1] > w[:, 0]).any() for w in wants)
    rv.close()


# ---- 4, 5. end to end --------------------------------------------------------------------------------------------------------------
def _bases(rrs):
    return np.concatenate([np.asarray(r.bases, "S1") for r in rrs]).view(np.uint8)


def _definition(rv, rrs, Qp=Q, Wp=W):
    """The bounds of the host: nrv_predict_reads_raw in the engine's mode, then the host routes' function."""
    p1, p2, a1, a2 = rv.predict_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs],
                                          [r.shift for r in rrs], [r.scale for r in rrs])
    return cli.trim_rows(rv.T, _bases(rrs), [len(r.starts) for r in rrs], p1, p2, a1, a2, Qp, Wp)


NAMES = [b"read_0", b"the_second_read"]


def _packed(rv, rrs, lds, fastq, stats=False, inner="merge", trim=True, min_len=1):
    if stats:
        blind = []
        for r in rrs:
            f = r.feat_ev.copy()
            f[:, 1:3] = np.nan
            blind.append(f)
        p = rv.pack_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], blind, [np.nan] * len(rrs), [np.nan] * len(rrs), rv.T)
        p = rv.with_device_stats(p, lds, [1] * len(rrs))
    else:
        p = rv.pack_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs], [r.shift for r in rrs], [r.scale for r in rrs], rv.T)
    p = rv.with_device_merge(p, _bases(rrs), fastq)
    if inner in ("report", "edits", "records", "all"):
        p = rv.with_device_report(p)
    if inner in ("edits", "records", "all"):
        p = rv.with_device_edits(p)
    if inner in ("records", "records_only", "all"):
        p = rv.with_device_records(p, NAMES[:len(rrs)], hand_back=inner != "records_only")
    if inner in ("profile", "all"):
        p = rv.with_device_profile(p)
    return rv.with_device_trim(p, Q, W, min_len) if trim else p


def _check_call(got, plain, want, what, names, min_len, whole):
    """A form-27 result: the trim last, every other output that of the same call without the trim (None where it carries none) -
    but for the blob, which is pack_records(..., trim) of the call's reads (`whole`: their seq / qual when the call leaves them on
    the device)."""
    assert len(got) == 10 and len(plain) in (3, 4, 6, 8, 9), what
    _same(got[9], want, what)
    for k, (g, p) in enumerate(zip(got, plain)):
        if k not in (6, 7):
            assert _eq(g, p), (what, k)
    assert all(g is None for g in got[len(plain):9]), what
    L = np.diff(got[2])
    assert (got[9][:, 0] >= 0).all() and (got[9][:, 1] <= L).all()
    if len(plain) >= 8 and plain[6] is not None:
        seq, qual = (got[0], got[1]) if got[0] is not None else whole
        wb, wo = hs.pack_records(names, seq, qual, got[2], want, min_len)
        assert np.array_equal(got[7], wo) and got[6].tobytes() == wb.tobytes(), what
        assert plain[6].tobytes() == hs.pack_records(names, seq, qual, got[2])[0].tobytes(), what
    else:
        assert got[6] is None and got[7] is None, what


def _end_to_end(rv, short_reads, inners=INNER):
    """Every end-to-end form on the two reads -> [(name, trim)]; compared with the definition inside."""
    out = []
    rrs, lds = [r for r, _ in short_reads], [ld for _, ld in short_reads]
    want = _definition(rv, rrs)
    # a vacuous pass is a failure: both reads are cut at both ends and keep something
    for fastq in (False, True):
        whole = rv.run_packed_raw(_packed(rv, rrs, lds, fastq, trim=False))[:2]
        L = np.diff(rv.run_packed_raw(_packed(rv, rrs, lds, fastq, trim=False))[2])
        assert ((0 < want[:, 0]) & (want[:, 0] < want[:, 1]) & (want[:, 1] < L)).all(), (want.tolist(), L.tolist())
        assert (want[:, 0] >= 2).all()                                   # the edge characters of Phred 2 cannot open a window of mean 3
        kept = want[:, 1] - want[:, 0]
        assert kept[0] != kept[1]
        drop_len = int(kept.min()) + 1                                   # above the shorter trimmed read: exactly that read is dropped
        for stats in (False, True):
            for inner in inners:
                for min_len in (1, drop_len):
                    got = rv.run_packed_raw(_packed(rv, rrs, lds, fastq, stats, inner, min_len=min_len))
                    plain = rv.run_packed_raw(_packed(rv, rrs, lds, fastq, stats, inner, trim=False))
                    _check_call(got, plain, want, ("one call", fastq, stats, inner, min_len), NAMES, min_len, whole)
                    if got[7] is not None and min_len == drop_len:
                        assert (np.diff(got[7]) > 0).tolist() == (kept >= drop_len).tolist() and (np.diff(got[7]) > 0).sum() == 1
                    out.append((f"one call {fastq} {stats} {inner} {min_len}", got[9].copy()))
        # two calls in flight, one read each
        wa, wb = _definition(rv, rrs[:1]), _definition(rv, rrs[1:])
        ta = rv.begin_packed_raw(_packed(rv, rrs[:1], lds[:1], fastq, inner="records"))
        tb = rv.begin_packed_raw(_packed(rv, rrs[1:], lds[1:], fastq, inner="records"))
        ga, gb = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
        _same(ga[9], wa, ("in flight, first", fastq))
        _same(gb[9], wb, ("in flight, second", fastq))
        assert not np.array_equal(ga[9], gb[9])
        _same(np.concatenate([ga[9], gb[9]]), want, ("the two calls are the one call's reads", fastq))
        assert ga[6].tobytes() == hs.pack_records(NAMES[:1], ga[0], ga[1], ga[2], wa, 1)[0].tobytes()
        assert gb[6].tobytes() == hs.pack_records(NAMES[:1], gb[0], gb[1], gb[2], wb, 1)[0].tobytes()
        # no window at all (N <= T): filled on the host, every quality 2
        r0 = rrs[0]
        for k in (rv.T, 4):
            p = rv.pack_reads_raw([r0.raw, r0.raw], [r0.starts[:k - 3], r0.starts[:3]], [r0.feat_ev[:k - 3], r0.feat_ev[:3]], [r0.shift] * 2, [r0.scale] * 2, rv.T)
            b = np.concatenate([np.asarray(r0.bases, "S1")[:k - 3], np.asarray(r0.bases, "S1")[:3]])
            for Qp, Wp in ((2, 3), (3, 3), (2, 4)):
                p27 = rv.with_device_trim(rv.with_device_records(rv.with_device_merge(p, b, fastq), NAMES), Qp, Wp, 1)
                got = rv.run_packed_raw(p27)
                z = np.zeros(0, np.int8)
                wt = cli.trim_rows(rv.T, b, [k - 3, 3], np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32), z, z, Qp, Wp)
                _same(got[9], wt, ("no window", k, Qp, Wp))
                wq = np.full(k, ord("#"), np.uint8) if fastq else None
                assert got[6].tobytes() == hs.pack_records(NAMES, b.view(np.uint8), wq, got[2], wt, 1)[0].tobytes(), ("no window", k, Qp, Wp)
    return out


def test_revise_reads_raw_trim_equals_the_definition(species_models, short_reads, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for mode in MODES:
        rv.set_precision(mode)
        _end_to_end(rv, short_reads, INNER if mode == "f16x2" else ["merge", "all"])
        assert rv.saturated() == (0, 0), mode
    rv.close()


def test_trim_call_refuses_a_bad_rule_by_its_name(species_models, short_reads, monkeypatch):
    from nanoreviser_amd.engine import NrvError
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rrs, lds = [r for r, _ in short_reads][:1], [ld for _, ld in short_reads][:1]
    p = _packed(rv, rrs, lds, True)
    for k, v in ((22, None), (26, None), (23, 0), (23, 41), (24, 0), (24, 65), (25, -1)):
        with pytest.raises(NrvError, match="nrv_revise_reads_raw_trim_begin"):
            rv.run_packed_raw(p[:k] + (v,) + p[k + 1:])
    _same(rv.run_packed_raw(p)[9], _definition(rv, rrs), "the handle is usable after a refusal")
    rv.close()


def test_range_guard_rerun_gives_the_f32_bounds(species_models, short_reads, monkeypatch):
    """The spiked read of tests/test_gpu_device_report.py behind a clean one: nrv_reads_raw_end runs the whole call again on the f32
    kernels and starts the accumulators from nothing - the bounds are the f32 mode's, not the minimum over two passes."""
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
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rv.set_precision("f32")
    p1, p2, a1, a2 = rv.predict_reads_raw(*args)
    el = [len(other.starts), N]
    want = cli.trim_rows(T, bases.view(np.uint8), el, p1, p2, a1, a2, Q, W)
    assert rv.saturated()[1] == 0 and (want[:, 1] > want[:, 0]).all()
    rv.set_precision("f16x2")
    for fq in (False, True):
        r0 = rv.saturated()[1]
        p = rv.with_device_records(rv.with_device_report(rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, fq)), NAMES)
        got = rv.run_packed_raw(rv.with_device_trim(p, Q, W, 1))
        assert rv.saturated()[1] - r0 == 1, fq
        _same(got[9], want, ("re-run", fq))
        assert got[6].tobytes() == hs.pack_records(NAMES, got[0], got[1], got[2], want, 1)[0].tobytes()
        assert np.array_equal(got[3][:, 2].astype(np.int64), np.diff(got[2]))                 # the report of the same pass
    rv.close()


def test_poisoned_workspace_gives_the_same_bounds(species_models, short_reads, monkeypatch):
    clean = _engine(monkeypatch, *species_models["ecoli"])
    ref = _end_to_end(clean, short_reads, ["merge", "all"])
    clean.close()
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
        for p in range(2):
            got = _end_to_end(rv, short_reads, ["merge", "all"])
            assert [k for k, _ in got] == [k for k, _ in ref]
            for (k, x), (_, y) in zip(ref, got):
                _same(y, x, (poison, p, k))
        c = planted_cases(10)
        for name in ("lengths, random", "only window across a tile edge", "window reaching into the next read"):
            qual, off, Qp = c[name]
            _same(rv.trim_reads(qual, off, Qp, 10), hs.trim_bounds(qual, off, Qp, 10), (poison, name))
        assert rv.saturated() == (0, 0), poison
        rv.close()


# ---- 6. command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_command_line_trim_is_the_same_on_the_device_route(tmp_path, monkeypatch, fmt):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_SUMMARY",
              "NRV_TRIM_Q"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NRV_CLI_GROUPS", "4")                               # a few reads per device call: several calls in flight
    d = tmp_path / "in"
    d.mkdir()
    src = sorted(glob.glob(os.path.join(FAST5, "*.fast5")) + glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))
    for i in range(10):
        shutil.copy(src[i % len(src)], d / f"s{i:02d}.fast5")
    forms = []
    real = Reviser.begin_packed_raw
    monkeypatch.setattr(Reviser, "begin_packed_raw", lambda self, packed: forms.append(len(packed)) or real(self, packed))
    outs, logs, comb = {}, {}, {}
    trim = ["--trim_q", "3", "--trim_window", "4"]
    for tag, extra, form, min_len in (("host", [], 7, 1), ("device", ["--device_merge"], 27, 1), ("host_c", ["--combined"], 7, 1),
                                      ("device_c", ["--device_merge", "--combined"], 27, 1), ("host_drop", [], 7, None),
                                      ("device_drop", ["--device_merge"], 27, None), ("device_c_drop", ["--device_merge", "--combined"], 27, None),
                                      ("host_c_drop", ["--combined"], 7, None)):
        if min_len is None:                                                 # above the median kept length: about half of the reads are dropped
            kept = sorted(int(ln.split("\t")[4]) - int(ln.split("\t")[3]) for ln in logs["host"].decode().split("\n")[1:11])
            assert kept[0] < kept[-1]
            min_len = kept[5] if kept[5] > kept[0] else kept[-1]
        del forms[:]
        out = str(tmp_path / tag) + "/"
        argv = ["-d", str(d), "-o", out, "-S", "ecoli", "-F", fmt, "--gpus", "1", "--thread", "4"] + trim
        argv += ["--min_len", str(min_len), "--trim_log", str(tmp_path / (tag + ".tsv"))]
        argv += [x for e in extra for x in ([e, str(tmp_path / (tag + "." + fmt))] if e == "--combined" else [e])]
        assert cli.main(argv) == 0
        outs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        logs[tag] = open(str(tmp_path / (tag + ".tsv")), "rb").read()
        assert outs[tag]["failed_reads.txt"] == b"" and forms and set(forms) == {form}, (tag, forms)
        if "--combined" in extra:
            comb[tag] = (open(str(tmp_path / (tag + "." + fmt)), "rb").read(), open(str(tmp_path / (tag + "." + fmt + ".fai")), "rb").read())
            assert len(outs[tag]) == 1
        assert not glob.glob(str(tmp_path / "*.part*")) and not glob.glob(out + "*.part*")
    assert outs["device"] == outs["host"] and logs["device"] == logs["host"] and len(outs["host"]) == 11
    assert outs["device_drop"] == outs["host_drop"] and logs["device_drop"] == logs["host_drop"] and 1 < len(outs["host_drop"]) < 11
    assert logs["device_c"] == logs["host_c"] == logs["host"] and logs["device_c_drop"] == logs["host_c_drop"] == logs["host_drop"]
    for a, b in (("device_c", "host_c"), ("device_c_drop", "host_c_drop")):
        assert sorted(comb[a][0].split(b"\n")) == sorted(comb[b][0].split(b"\n"))
        assert sorted(ln.split(b"\t")[:2] for ln in comb[a][1].split(b"\n")) == sorted(ln.split(b"\t")[:2] for ln in comb[b][1].split(b"\n"))
    lines = [ln.split("\t") for ln in logs["host_drop"].decode().split("\n")[1:11]]
    assert all(c[1] == "revised" and 0 < int(c[3]) < int(c[4]) < int(c[2]) for c in lines)
    for c in lines:                                                         # a dropped read has no file, a kept one its bases [lo, hi)
        f = c[0].split(".")[0] + "_out." + fmt
        assert (f in outs["host_drop"]) == (c[5] == "1")
        body = outs["host"][f].split(b"\n")[1]
        assert len(body) - (fmt == "fastq") == int(c[4]) - int(c[3])
    assert comb["device_c_drop"][1].count(b"\n") == sum(c[5] == "1" for c in lines) == len(outs["host_drop"]) - 1
