"""The per-read revision report counted on the device (MI355X only, -m gpu): csrc/nrv_report.h through nrv_merge_calls_report,
nrv_revise_reads_raw_report_begin / nrv_revise_reads_raw_report and the command line's --report.

Everything is compared BIT FOR BIT - the counts are integers, nothing here has a tolerance.  hoststage.revision_report is the
definition (tests/test_revision_report_host.py holds it to the rule text).  T = 11, the shipped E. coli weights (the kernel and
the report call at T = 1, 2, 12, 13, 32: tests/test_gpu_window_lengths.py):
  3. nrv_merge_calls_report on the inputs of tests/report_cases.py (one call of ~2.8 k events: a read boundary on a tile edge, others
     mid-tile, a tile with five reads, a read over whole tiles, empty reads first / in the middle / last; labels out of range; ties,
     margins one ulp either side of tie_eps, NaNs), with and without q_thr; seq / qual / off are nrv_merge_calls';
  4. nrv_revise_reads_raw_report on the two shortest fixture reads in one call, in each precision mode, against the definition on
     the outputs of nrv_predict_reads_raw in that mode; seq / qual / off are nrv_revise_reads_raw's;
  5. two calls in flight: each report is its own;
  6. a call that trips the f16x2 range guard: one re-run, the report is the f32 mode's - nothing is counted twice;
  7. handles created under NRV_POISON: the reports of 4 unchanged;
  8. a call with N <= T: the report filled on the host;
  9. the command line with --report, with and without --device_merge and --device_stats: one report, the same read files.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from report_cases import T, TIE_EPS, report_case

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "bf16x3", "f32"]
PATTERNS = {"qnan": 0x7FC00000, "m1500": 0xC4BB8000}
FAST5 = os.path.join(GOLD, "fast5")


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
    assert rv.T == T
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
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8].tolist())


def _bases(rrs):
    return np.concatenate([np.asarray(r.bases, "S1") for r in rrs]).view(np.uint8)


def _definition(rv, rrs, fastq, tie_eps=TIE_EPS, feats=None, shifts=None, scales=None, raws=None, starts=None):
    """(report, seq, qual, off) of the host: nrv_predict_reads_raw in the engine's mode, then the definition and the host merge."""
    p1, p2, a1, a2 = rv.predict_reads_raw(raws or [r.raw for r in rrs], starts or [r.starts for r in rrs], feats or [r.feat_ev for r in rrs],
                                          shifts or [r.shift for r in rrs], scales or [r.scale for r in rrs])
    el = [len(s) for s in (starts or [r.starts for r in rrs])]
    b = np.concatenate([np.asarray(r.bases, "S1")[:n] for r, n in zip(rrs, el)]).view(np.uint8)
    qc = cli.phred_chars(p1, p2, a1, a2) if fastq else None
    return (hs.revision_report(b, el, a1, a2, p1, p2, qc, rv.T, tie_eps),) + tuple(hs.emit_calls(b, el, a1, a2, qc, rv.T))


def _packed(rv, rrs, lds, fastq, stats, tie_eps=None, report=True):
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
    return rv.with_device_report(p, tie_eps) if report else p


def _check_call(got, want, what):
    seq, qual, off, rep = got
    _same(rep, want[0], what)
    assert np.array_equal(seq, want[1]) and np.array_equal(off, want[3]), what
    assert (qual is None) == (want[2] is None) and (qual is None or np.array_equal(qual, want[2])), what


# ---- 3. the kernel alone ---------------------------------------------------------------------------------------------------------
def test_merge_calls_report_equals_the_definition(species_models, monkeypatch):
    c = report_case()
    thr = cli.phred_thresholds()
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for p in range(2):                                                   # a second pass on the same handle
        # FASTQ: quality from the thresholds, near-ties from the rows
        qc = cli.phred_lookup(np.minimum(c["p1"][np.arange(c["n"]), np.clip(c["a1"], 0, 5)], c["p2"][np.arange(c["n"]), np.clip(c["a2"], 0, 4)]))
        seq, qual, off, rep = rv.merge_calls_report_device(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], thr, TIE_EPS)
        _same(rep, hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], qc, T, TIE_EPS), ("fastq", p))
        assert rep[:, 21].sum() == 7 and rep[:, 22].sum() > 0
        m = rv.merge_calls_device(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], thr)
        assert np.array_equal(seq, m[0]) and np.array_equal(qual, m[1]) and np.array_equal(off, m[2])
        assert np.array_equal(rep[:, 2].astype(np.int64), np.diff(off))
        # without q_thr: the rows still give the near-ties, no quality is summed
        seq, qual, off, rep = rv.merge_calls_report_device(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], None, TIE_EPS)
        _same(rep, hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], None, T, TIE_EPS), ("fasta", p))
        m = rv.merge_calls_device(c["bases"], c["ev_len"], c["a1"], c["a2"])
        assert qual is None and np.array_equal(seq, m[0]) and np.array_equal(off, m[2])
        assert rep[:, 21].sum() == 7 and not rep[:, 22].any()
        # without the rows: no near-tie column; another margin
        rep = rv.merge_calls_report_device(c["bases"], c["ev_len"], c["a1"], c["a2"])[3]
        _same(rep, hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], None, None, None, T), ("bare", p))
        rep = rv.merge_calls_report_device(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], None, 0.05)[3]
        _same(rep, hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], None, T, 0.05), ("eps 0.05", p))
    rv.close()


# ---- 4, 5, 8. end to end ---------------------------------------------------------------------------------------------------------
def _end_to_end(rv, short_reads):
    """Every end-to-end form on the two reads -> [(name, report)]; compared with the definition inside."""
    out = []
    rrs, lds = [r for r, _ in short_reads], [ld for _, ld in short_reads]
    for fastq in (False, True):
        want = _definition(rv, rrs, fastq)
        for stats in (False, True):
            got = rv.run_packed_raw(_packed(rv, rrs, lds, fastq, stats))
            _check_call(got, want, ("one call", fastq, stats))
            plain = rv.run_packed_raw(_packed(rv, rrs, lds, fastq, stats, report=False))      # nrv_revise_reads_raw
            assert len(plain) == 3 and np.array_equal(got[0], plain[0]) and np.array_equal(got[2], plain[2])
            assert (got[1] is None and plain[1] is None) or np.array_equal(got[1], plain[1])
            assert (got[3][:, 22].sum() > 0) == fastq
            out.append((f"one call {fastq} {stats}", got[3].copy()))
        # near_tie is filled without a quality too: a margin that real calls do fall under
        got = rv.run_packed_raw(_packed(rv, rrs, lds, fastq, False, tie_eps=0.2))
        _check_call(got, _definition(rv, rrs, fastq, 0.2), ("eps 0.2", fastq))
        assert (got[3][:, 21] > 0).all()
        out.append((f"eps 0.2 {fastq}", got[3].copy()))
        # 5. two calls in flight, one read each
        wa, wb = _definition(rv, rrs[:1], fastq), _definition(rv, rrs[1:], fastq)
        ta = rv.begin_packed_raw(_packed(rv, rrs[:1], lds[:1], fastq, False))
        tb = rv.begin_packed_raw(_packed(rv, rrs[1:], lds[1:], fastq, False))
        ga, gb = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
        _check_call(ga, wa, ("in flight, first", fastq))
        _check_call(gb, wb, ("in flight, second", fastq))
        assert not np.array_equal(ga[3], gb[3])
        _same(np.concatenate([ga[3], gb[3]]), want[0], ("the two calls are the one call's reads", fastq))
        # 8. no window at all (N <= T): filled on the host
        r0 = rrs[0]
        for k in (T, 4):
            p = rv.pack_reads_raw([r0.raw, r0.raw], [r0.starts[:k - 3], r0.starts[:3]], [r0.feat_ev[:k - 3], r0.feat_ev[:3]], [r0.shift] * 2, [r0.scale] * 2, rv.T)
            b = np.concatenate([np.asarray(r0.bases, "S1")[:k - 3], np.asarray(r0.bases, "S1")[:3]])
            seq, qual, off, rep = rv.run_packed_raw(rv.with_device_report(rv.with_device_merge(p, b, fastq)))
            z = np.zeros(0, np.int8)
            _same(rep, hs.revision_report(b.view(np.uint8), [k - 3, 3], z, z, None, None, np.zeros(0, np.uint8) if fastq else None, T), ("no window", k))
            assert rep[:, 0].tolist() == rep[:, 2].tolist() == rep[:, 3].tolist() == [k - 3, 3] and not rep[:, 4:22].any()
            assert seq.tobytes() == b.tobytes() and off.tolist() == [0, k - 3, k]
    return out


def test_revise_reads_raw_report_equals_the_definition(species_models, short_reads, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for mode in MODES:
        rv.set_precision(mode)
        _end_to_end(rv, short_reads)
        assert rv.saturated() == (0, 0), mode
    rv.close()


# ---- 6. range guard --------------------------------------------------------------------------------------------------------------
def test_range_guard_rerun_counts_once(species_models, short_reads, monkeypatch):
    """The spiked read of tests/test_gpu_range.py / test_gpu_device_merge.py behind a clean one: nrv_reads_raw_end runs the whole
    call again on the f32 kernels, zeroes the report block and counts again - the report is the f32 mode's, not a sum of two."""
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
    want = {fq: (hs.revision_report(bases.view(np.uint8), el, a1, a2, p1, p2, cli.phred_chars(p1, p2, a1, a2) if fq else None, T, 0.2),)
            + tuple(hs.emit_calls(bases.view(np.uint8), el, a1, a2, cli.phred_chars(p1, p2, a1, a2) if fq else None, T)) for fq in (False, True)}
    assert rv.saturated()[1] == 0
    rv.set_precision("f16x2")
    for fq in (False, True):
        r0 = rv.saturated()[1]
        p = rv.with_device_report(rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, fq), 0.2)
        got = rv.run_packed_raw(p)
        assert rv.saturated()[1] - r0 == 1, fq
        _check_call(got, want[fq], ("re-run", fq))
        assert got[3][:, 1].tolist() == [el[0] - T, N - T]
    rv.close()


# ---- 7. poison -------------------------------------------------------------------------------------------------------------------
def test_poisoned_workspace_gives_the_same_reports(species_models, short_reads, monkeypatch):
    clean = _engine(monkeypatch, *species_models["ecoli"])
    ref = _end_to_end(clean, short_reads)
    clean.close()
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
        for p in range(2):
            got = _end_to_end(rv, short_reads)
            assert [k for k, _ in got] == [k for k, _ in ref]
            for (k, x), (_, y) in zip(ref, got):
                _same(y, x, (poison, p, k))
        assert rv.saturated() == (0, 0), poison
        rv.close()


# ---- 9. command line -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_command_line_report_is_the_same_on_every_path(tmp_path, monkeypatch, fmt):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT"):
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
    outs, reps = {}, {}
    for tag, extra in (("plain", None), ("host", []), ("host_stats", ["--device_stats"]), ("merge", ["--device_merge"]),
                       ("merge_stats", ["--device_merge", "--device_stats"])):
        del forms[:]
        out = str(tmp_path / tag) + "/"
        rep = str(tmp_path / (tag + ".tsv"))
        argv = ["-d", str(d), "-o", out, "-S", "ecoli", "-F", fmt, "--gpus", "1", "--thread", "4"]
        assert cli.main(argv + (extra + ["--report", rep] if extra is not None else [])) == 0
        outs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        assert outs[tag]["failed_reads.txt"] == b"" and len(outs[tag]) == 11
        assert forms and set(forms) == {{"plain": 7, "host": 7, "host_stats": 9, "merge": 14, "merge_stats": 14}[tag]}, (tag, forms)
        if extra is not None:
            reps[tag] = open(rep, "rb").read()
        else:
            assert not os.path.exists(rep)
        assert not glob.glob(str(tmp_path / "*.part*"))
    assert all(o == outs["plain"] for o in outs.values())
    assert all(r == reps["host"] for r in reps.values())
    lines = reps["host"].decode().split("\n")
    assert len(lines) == 1 + 10 + 1 + 1 and lines[-2].startswith("#total\t") and [ln.split("\t")[0] for ln in lines[1:11]] == sorted(os.listdir(d))
    for ln in lines[1:11]:
        c = ln.split("\t")
        v = [int(x) for x in c[2:]]
        body = outs["plain"][c[0].split(".")[0] + "_out." + fmt].split(b"\n")[1].split(b"+")[0]
        assert c[1] == "revised" and v[2] == len(body) and sum(v[4:9]) == v[1] == v[0] - T and (v[22] > 0) == (fmt == "fastq")
        assert v[20] > v[1] // 2                                             # model 2 mostly agrees with the basecaller on these reads
