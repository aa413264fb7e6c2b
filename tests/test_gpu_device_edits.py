"""The per-read edit list compacted on the device (MI355X only, -m gpu): csrc/nrv_edits.h through nrv_merge_calls_edits,
nrv_revise_reads_raw_edits_begin / nrv_revise_reads_raw_edits and the command line's --edits.

Everything is compared BIT FOR BIT - slots and positions are integers, conf is a copied f32 - the records as .tobytes().
hoststage.revision_edits is the definition (tests/test_revision_edits_host.py holds it to the rule text).  T = 11, the shipped
E. coli weights (the kernels and the edits call at T = 1, 2, 12, 13, 32: tests/test_gpu_window_lengths.py):
  1. nrv_merge_calls_edits on tests/report_cases.py (a read boundary on a tile edge, five reads in one tile, a read over whole
     tiles, empty reads first / in the middle / last), two passes on one handle: FASTQ, rows without q_thr, bare; seq / qual /
     off / report are nrv_merge_calls_report's;
  2. all-deletion, all-insertion, no-edit calls, and one call of 257 * 256 + 3 events in four reads - the tile scan carries
     across its 256-wide passes - with random and with all-deletion labels;
  3. nrv_revise_reads_raw_edits on the two shortest fixture reads in each precision mode against the definition on the outputs
     of nrv_predict_reads_raw in that mode: with and without a report, with and without device statistics, FASTA and FASTQ, two
     calls in flight, N <= T;
  4. a call that trips the f16x2 range guard: one re-run, the records are the f32 mode's;
  5. handles created under NRV_POISON: records and edit_off unchanged;
  6. the caller's records pre-filled with 0xA5: rows at and beyond edit_off[-1] untouched;
  7. the command line with --edits, with and without --device_merge / --device_stats / --report: the same edit files, and the
     read outputs and the report of a run without --edits.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from edits_cases import carry_case, density_case
from report_cases import T, TIE_EPS, report_case
from test_gpu_device_report import FAST5, MODES, PATTERNS, _bases, _engine, short_reads  # noqa: F401 (short_reads: a fixture)

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    """(edits, edit_off) against the definition's."""
    assert got[0].dtype == hs.EDIT_DTYPE and got[1].dtype == np.int64, what
    assert np.array_equal(got[1], want[1]), (what, got[1].tolist()[:8], want[1].tolist()[:8])
    assert len(got[0]) == int(want[1][-1]), (what, len(got[0]))
    if got[0].tobytes() != want[0].tobytes():
        bad = np.flatnonzero(got[0] != want[0])[:4]
        raise AssertionError((what, bad.tolist(), got[0][bad].tolist(), want[0][bad].tolist()))


def _kernel_forms(rv, c, what):
    """The three forms of nrv_merge_calls_edits on one case, each against the definition."""
    thr = cli.phred_thresholds()
    n = c["n"]
    qc = cli.phred_lookup(np.minimum(c["p1"][np.arange(n), np.clip(c["a1"], 0, 5)], c["p2"][np.arange(n), np.clip(c["a2"], 0, 4)])) \
        if n else np.zeros(0, np.uint8)
    ins = (c["bases"], c["ev_len"], c["a1"], c["a2"])
    out = {}
    for form, (p, q) in {"fastq": (True, thr), "rows": (True, None), "bare": (False, None)}.items():
        p1, p2 = (c["p1"], c["p2"]) if p else (None, None)
        got = rv.merge_calls_edits_device(*ins, p1, p2, q, TIE_EPS)
        _same(got[4:], hs.revision_edits(*ins, p1, p2, qc if q is not None else None, T), (what, form))
        out[form] = got
    return out


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------------------
def test_merge_calls_edits_equals_the_definition(species_models, monkeypatch):
    c = report_case()
    thr = cli.phred_thresholds()
    rv = _engine(monkeypatch, *species_models["ecoli"])
    ins = (c["bases"], c["ev_len"], c["a1"], c["a2"])
    for p in range(2):                                                   # a second pass on the same handle
        got = _kernel_forms(rv, c, p)
        assert len(got["fastq"][4]) > 300 and set(got["fastq"][4]["kind"].tolist()) == {1, 2, 3}
        for form, (p1, p2, q) in {"fastq": (c["p1"], c["p2"], thr), "rows": (c["p1"], c["p2"], None), "bare": (None, None, None)}.items():
            seq, qual, off, rep = rv.merge_calls_report_device(*ins, p1, p2, q, TIE_EPS)
            g = got[form]
            assert np.array_equal(g[0], seq) and np.array_equal(g[2], off) and np.array_equal(g[3], rep), (form, p)
            assert (g[1] is None and qual is None) or np.array_equal(g[1], qual), (form, p)
        # without a report (NULL): the same records
        g = rv.merge_calls_edits_device(*ins, c["p1"], c["p2"], thr, report=False)
        assert g[3] is None and np.array_equal(g[0], got["fastq"][0])
        _same(g[4:], got["fastq"][4:], ("no report", p))
    rv.close()


# ---- 2. densities, and the carry of the tile scan ----------------------------------------------------------------------------------
def test_density_and_carry_cases(species_models, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for what in ("deletion", "insertion", "none"):
        one = density_case(what, ev_len=(700,))
        got = _kernel_forms(rv, one, (what, "one read"))
        assert got["fastq"][5].tolist() == [0, 0 if what == "none" else one["n"]]         # total == n_win
        _kernel_forms(rv, density_case(what), (what, "reads"))
    for deletions in (False, True):
        c = carry_case(deletions)
        assert (c["N"] + 255) // 256 > 256
        got = _kernel_forms(rv, c, ("carry", deletions))
        assert got["bare"][5][-1] > (256 * 256 // 8 if not deletions else c["n"] - 4 * T)
    rv.close()


# ---- 3, 6. end to end --------------------------------------------------------------------------------------------------------------
def _definition(rv, rrs, fastq):
    """(report, seq, qual, off, edits, edit_off) of the host: nrv_predict_reads_raw in the engine's mode, then the definitions."""
    p1, p2, a1, a2 = rv.predict_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs],
                                          [r.shift for r in rrs], [r.scale for r in rrs])
    el = [len(r.starts) for r in rrs]
    b = _bases(rrs)
    qc = cli.phred_chars(p1, p2, a1, a2) if fastq else None
    return (hs.revision_report(b, el, a1, a2, p1, p2, qc, rv.T, TIE_EPS),) + tuple(hs.emit_calls(b, el, a1, a2, qc, rv.T)) \
        + tuple(hs.revision_edits(b, el, a1, a2, p1, p2, qc, rv.T))


def _packed(rv, rrs, lds, fastq, stats, report):
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
    p = rv.with_device_edits(rv.with_device_report(p, TIE_EPS) if report else p)
    assert len(p) == 16
    p[14].view(np.uint8)[:] = 0xA5                                         # 6. what the call does not write stays
    return p


def _check_call(got, want, what, report, packed=None):
    seq, qual, off, rep, edits, edit_off = got
    assert np.array_equal(seq, want[1]) and np.array_equal(off, want[3]), what
    assert (qual is None) == (want[2] is None) and (qual is None or np.array_equal(qual, want[2])), what
    assert (rep is None) == (not report) and (rep is None or np.array_equal(rep, want[0])), what
    _same((edits, edit_off), want[4:], what)
    if packed is not None:
        rest = packed[14].view(np.uint8).reshape(-1, 16)[int(edit_off[-1]):]
        assert len(rest) > 0 and (rest == 0xA5).all(), what


def _end_to_end(rv, short_reads):
    """Every end-to-end form on the two reads -> [(name, records, edit_off)]; compared with the definition inside."""
    out = []
    rrs, lds = [r for r, _ in short_reads], [ld for _, ld in short_reads]
    for fastq in (False, True):
        want = _definition(rv, rrs, fastq)
        assert want[5][-1] > 0                                           # an empty list cannot pass for a correct one
        for stats in (False, True):
            for report in (True, False):
                p = _packed(rv, rrs, lds, fastq, stats, report)
                got = rv.run_packed_raw(p)
                _check_call(got, want, ("one call", fastq, stats, report), report, p)
                out.append((f"one call {fastq} {stats} {report}", got[4].copy(), got[5].copy()))
        assert (want[4]["qual"] > 33).all() if fastq else not want[4]["qual"].any()
        assert (want[4]["conf"] > 0).all()                               # FASTA calls carry the confidence too
        # two calls in flight, one read each: concatenated, they are the one call's records
        wa, wb = _definition(rv, rrs[:1], fastq), _definition(rv, rrs[1:], fastq)
        pa, pb = _packed(rv, rrs[:1], lds[:1], fastq, False, True), _packed(rv, rrs[1:], lds[1:], fastq, False, False)
        ta, tb = rv.begin_packed_raw(pa), rv.begin_packed_raw(pb)
        ga, gb = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
        _check_call(ga, wa, ("in flight, first", fastq), True, pa)
        _check_call(gb, wb, ("in flight, second", fastq), False, pb)
        assert np.concatenate([ga[4], gb[4]]).tobytes() == want[4].tobytes()
        assert np.array_equal(np.concatenate([ga[5], gb[5][1:] + ga[5][-1]]), want[5])
        # no window at all (N <= T): edit_off is zeros, filled on the host
        r0 = rrs[0]
        for k in (T, 4):
            p = rv.pack_reads_raw([r0.raw, r0.raw], [r0.starts[:k - 3], r0.starts[:3]], [r0.feat_ev[:k - 3], r0.feat_ev[:3]], [r0.shift] * 2, [r0.scale] * 2, rv.T)
            b = np.concatenate([np.asarray(r0.bases, "S1")[:k - 3], np.asarray(r0.bases, "S1")[:3]])
            p = rv.with_device_edits(rv.with_device_merge(p, b, fastq))
            p[15][:] = -1
            seq, qual, off, rep, edits, edit_off = rv.run_packed_raw(p)
            assert rep is None and len(edits) == 0 and edit_off.tolist() == [0, 0, 0]
            assert seq.tobytes() == b.tobytes() and off.tolist() == [0, k - 3, k]
    return out


def test_revise_reads_raw_edits_equals_the_definition(species_models, short_reads, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for mode in MODES:
        rv.set_precision(mode)
        _end_to_end(rv, short_reads)
        assert rv.saturated() == (0, 0), mode
    rv.close()


# ---- 4. range guard ----------------------------------------------------------------------------------------------------------------
def test_range_guard_rerun_gives_the_f32_records(species_models, short_reads, monkeypatch):
    """The spiked read of tests/test_gpu_device_report.py behind a clean one: nrv_reads_raw_end runs the whole call again on the f32
    kernels and the three edit launches behind the merge - the records are the f32 mode's."""
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
    b8 = bases.view(np.uint8)
    want = {}
    for fq in (False, True):
        qc = cli.phred_chars(p1, p2, a1, a2) if fq else None
        want[fq] = (hs.revision_report(b8, el, a1, a2, p1, p2, qc, T, TIE_EPS),) + tuple(hs.emit_calls(b8, el, a1, a2, qc, T)) \
            + tuple(hs.revision_edits(b8, el, a1, a2, p1, p2, qc, T))
        assert (np.diff(want[fq][5]) > 0).all()
    assert rv.saturated()[1] == 0
    rv.set_precision("f16x2")
    for fq in (False, True):
        r0 = rv.saturated()[1]
        p = rv.with_device_edits(rv.with_device_report(rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, fq), TIE_EPS))
        p[14].view(np.uint8)[:] = 0xA5
        got = rv.run_packed_raw(p)
        assert rv.saturated()[1] - r0 == 1, fq
        _check_call(got, want[fq], ("re-run", fq), True, p)
    rv.close()


# ---- 5. poison ---------------------------------------------------------------------------------------------------------------------
def test_poisoned_workspace_gives_the_same_records(species_models, short_reads, monkeypatch):
    clean = _engine(monkeypatch, *species_models["ecoli"])
    ref = _end_to_end(clean, short_reads)
    c = report_case()
    ref_k = _kernel_forms(clean, c, "clean")
    clean.close()
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
        for p in range(2):
            got = _end_to_end(rv, short_reads)
            assert [k for k, _, _ in got] == [k for k, _, _ in ref]
            for (k, e, o), (_, e2, o2) in zip(ref, got):
                assert e.tobytes() == e2.tobytes() and np.array_equal(o, o2), (poison, p, k)
            got_k = _kernel_forms(rv, c, (poison, p))
            for form in ref_k:
                _same(got_k[form][4:], ref_k[form][4:], (poison, p, form))
        assert rv.saturated() == (0, 0), poison
        rv.close()


# ---- 7. command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_command_line_edits_are_the_same_on_every_path(tmp_path, monkeypatch, fmt):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS"):
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
    outs, eds, reps = {}, {}, {}
    runs = (("plain", None, True), ("host", [], True), ("host_stats", ["--device_stats"], False),
            ("merge", ["--device_merge"], False), ("merge_stats", ["--device_merge", "--device_stats"], True))
    for tag, extra, report in runs:
        del forms[:]
        out = str(tmp_path / tag) + "/"
        ed, rep = str(tmp_path / (tag + "_ed")), str(tmp_path / (tag + ".tsv"))
        argv = ["-d", str(d), "-o", out, "-S", "ecoli", "-F", fmt, "--gpus", "1", "--thread", "4"]
        argv += (extra + ["--edits", ed] if extra is not None else []) + (["--report", rep] if report else [])
        assert cli.main(argv) == 0
        outs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        assert outs[tag]["failed_reads.txt"] == b"" and len(outs[tag]) == 11
        want_form = 16 if extra is not None and "--device_merge" in extra else (9 if extra and "--device_stats" in extra else 7)
        assert forms and set(forms) == {want_form}, (tag, forms)
        if extra is not None:
            eds[tag] = {f: open(os.path.join(ed, f), "rb").read() for f in sorted(os.listdir(ed))}
            assert sorted(eds[tag]) == [f"s{i:02d}_edits.tsv" for i in range(10)]
        else:
            assert not os.path.exists(ed)
        if report:
            reps[tag] = open(rep, "rb").read()
    assert all(o == outs["plain"] for o in outs.values())
    assert all(e == eds["host"] for e in eds.values())
    assert len(reps) == 3 and all(r == reps["plain"] for r in reps.values())
    for f, text in eds["host"].items():
        lines = text.decode().split("\n")
        assert lines[0] == cli.EDITS_HEADER and lines[-1] == "" and len(lines) > 3
        kinds = [ln.split("\t")[2] for ln in lines[1:-1]]
        row = [ln for ln in reps["plain"].decode().split("\n") if ln.startswith(f.split("_")[0] + ".fast5\t")][0].split("\t")
        assert [kinds.count(k) for k in "SID"] == [int(v) for v in row[2 + 5:2 + 8]]
        assert all((ln.split("\t")[5] == ".") == (fmt == "fasta") for ln in lines[1:-1])
