"""The FASTA / FASTQ records laid out on the device (MI355X only, -m gpu): csrc/nrv_pack.h through nrv_pack_records,
nrv_revise_reads_raw_records_begin / nrv_revise_reads_raw_records and the command line's --combined.

Everything is compared BYTE FOR BYTE - copies and integer offsets, nothing here has a tolerance.  hoststage.pack_records is the
definition (tests/test_combined_records_host.py holds it to the rule text).  T = 11, the shipped E. coli weights (the records call
at T = 1, 2, 12, 13, 32: tests/test_gpu_window_lengths.py; nrv_pack_records itself does not depend on T):
  1. nrv_pack_records on the merged reads of tests/report_cases.py, two passes on one handle, FASTQ and FASTA; the caller's blob
     is pre-filled with 0xA5 and untouched at and beyond the total;
  2. edge shapes: no read, only empty reads, names of 1 / 3 / 4 / 5 / 15 / 16 / 17 / 255 bytes and one with `|||` (the kernel
     stores 4-byte words), a first sequence at byte 3 of the blob, 600 reads of 0 - 40 bases (the scan over the reads carries
     across its 256-wide passes), and one call of 257 * 256 + 3 events in four reads (a record that spans many workgroups);
  3. nrv_revise_reads_raw_records on the two shortest fixture reads in each precision mode against the definition on the outputs
     of nrv_predict_reads_raw in that mode: with and without a report, edits, device statistics, FASTA and FASTQ, reads handed
     back or not, two calls in flight, N <= T; off / report / edits are those of the edits call;
  4. a call that trips the f16x2 range guard: one re-run, blob and rec_off are the f32 mode's;
  5. handles created under NRV_POISON: blob and rec_off unchanged;
  6. the command line with --device_merge --combined, alone and with --device_stats / --report / --edits: the records are the
     per-read outputs of a run without --combined, they came from the device call, and the host route gives the same set.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from records_cases import EDGE_CASES, carry_records_case, fai_lines, parse_records, report_records_case
from report_cases import T, TIE_EPS
from test_gpu_device_report import FAST5, MODES, PATTERNS, _bases, _engine, short_reads  # noqa: F401 (short_reads: a fixture)

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    """(blob, rec_off) against the definition's."""
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int64, what
    assert np.array_equal(got[1], want[1]), (what, got[1].tolist()[:8], want[1].tolist()[:8])
    assert len(got[0]) == int(want[1][-1]), (what, len(got[0]))
    if got[0].tobytes() != want[0].tobytes():
        bad = np.flatnonzero(got[0] != want[0])[:8]
        raise AssertionError((what, bad.tolist(), got[0][bad].tolist(), want[0][bad].tolist()))


def _kernel(rv, c, what):
    """nrv_pack_records on one case against the definition; the caller's blob beyond the total stays as it was."""
    want = hs.pack_records(c["names"], c["seq"], c["qual"], c["off"])
    mine = np.full(len(want[0]) + 64, 0xA5, np.uint8)
    got = rv.pack_records_device(c["names"], c["seq"], c["qual"], c["off"], blob=mine)
    _same(got, want, what)
    assert (mine[len(want[0]):] == 0xA5).all(), what
    return got


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------------------
def test_pack_records_equals_the_definition(species_models, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for p in range(2):                                                   # a second pass on the same handle
        for fastq in (True, False):
            c = report_records_case(fastq)
            blob, rec_off = _kernel(rv, c, ("report case", fastq, p))
            assert (np.diff(rec_off) >= 3).all() and len(parse_records(blob, fastq)) == len(c["names"])
    rv.close()


# ---- 2. edge shapes ----------------------------------------------------------------------------------------------------------------
def test_edge_shapes(species_models, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for fastq in (False, True):
        for what, build in EDGE_CASES.items():
            c = build(fastq)
            blob, rec_off = _kernel(rv, c, (what, fastq))
            if what == "name lengths":
                assert len(c["names"][0]) == 1 and rec_off[0] == 0           # '>' + 1 byte + '\n': the first sequence starts at byte 3
                assert {len(n) for n in c["names"]} == {1, 3, 4, 5, 15, 16, 17, 255} and any(b"|||" in n for n in c["names"])
            if what == "600 tiny reads":
                assert len(c["names"]) == 600 and rec_off[-1] > 600 * 3
        c = carry_records_case(fastq)
        blob, rec_off = _kernel(rv, c, ("carry", fastq))
        assert np.diff(rec_off).max() > 256 * 256                        # one record over more than 64 workgroups of 1024 bytes
    rv.close()


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------
def _names(k):
    return [b"r%d|||x" % i + b"y" * i for i in range(k)]


def _definition(rv, rrs, fastq):
    """(report, seq, qual, off, edits, edit_off, blob, rec_off) of the host: nrv_predict_reads_raw in the engine's mode, then the definitions."""
    p1, p2, a1, a2 = rv.predict_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs],
                                          [r.shift for r in rrs], [r.scale for r in rrs])
    el = [len(r.starts) for r in rrs]
    b = _bases(rrs)
    qc = cli.phred_chars(p1, p2, a1, a2) if fastq else None
    merged = tuple(hs.emit_calls(b, el, a1, a2, qc, rv.T))
    return (hs.revision_report(b, el, a1, a2, p1, p2, qc, rv.T, TIE_EPS),) + merged + tuple(hs.revision_edits(b, el, a1, a2, p1, p2, qc, rv.T)) \
        + tuple(hs.pack_records(_names(len(rrs)), *merged))


def _packed(rv, rrs, lds, fastq, stats, report, edits, hand_back=True):
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
    if report:
        p = rv.with_device_report(p, TIE_EPS)
    if edits:
        p = rv.with_device_edits(p)
    p = rv.with_device_records(p, _names(len(rrs)), hand_back=hand_back)
    assert len(p) == 20
    p[18][:] = 0xA5                                                       # what the call does not write stays
    return p


def _check_call(got, want, what, report, edits, packed, hand_back=True):
    seq, qual, off, rep, ed, edit_off, blob, rec_off = got
    assert np.array_equal(off, want[3]), what
    if hand_back:
        assert np.array_equal(seq, want[1]), what
        assert (qual is None) == (want[2] is None) and (qual is None or np.array_equal(qual, want[2])), what
    else:
        assert seq is None and qual is None, what
    assert (rep is None) == (not report) and (rep is None or np.array_equal(rep, want[0])), what
    assert (ed is None) == (not edits) == (edit_off is None), what
    if edits:
        assert np.array_equal(edit_off, want[5]) and ed.tobytes() == want[4].tobytes(), what
    _same((blob, rec_off), want[6:], what)
    rest = packed[18][int(rec_off[-1]):]
    assert len(rest) > 0 and (rest == 0xA5).all(), what


def _end_to_end(rv, short_reads):
    """Every end-to-end form on the two reads -> [(name, blob, rec_off)]; compared with the definition inside."""
    out = []
    rrs, lds = [r for r, _ in short_reads], [ld for _, ld in short_reads]
    for fastq in (False, True):
        want = _definition(rv, rrs, fastq)
        assert want[7][-1] > sum(len(r.starts) for r in rrs) * (2 if fastq else 1)
        for stats in (False, True):
            for report in (True, False):
                for edits in (True, False):
                    back = report == edits                               # reads handed back in half of the forms
                    p = _packed(rv, rrs, lds, fastq, stats, report, edits, back)
                    got = rv.run_packed_raw(p)
                    _check_call(got, want, ("one call", fastq, stats, report, edits), report, edits, p, back)
                    out.append((f"one call {fastq} {stats} {report} {edits}", got[6].copy(), got[7].copy()))
            # off / report / edits are those of the edits call
            pe = rv.with_device_merge(rv.pack_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs],
                                                        [r.shift for r in rrs], [r.scale for r in rrs], rv.T), _bases(rrs), fastq)
            ge = rv.run_packed_raw(rv.with_device_edits(rv.with_device_report(pe, TIE_EPS)))
            gr = rv.run_packed_raw(_packed(rv, rrs, lds, fastq, stats, True, True))
            assert np.array_equal(ge[2], gr[2]) and np.array_equal(ge[3], gr[3]) and ge[4].tobytes() == gr[4].tobytes()
            assert np.array_equal(ge[5], gr[5]) and np.array_equal(ge[0], gr[0])
        # two calls in flight, one read each: concatenated, they are the one call's records but for the names
        wa, wb = _definition(rv, rrs[:1], fastq), _definition(rv, rrs[1:], fastq)
        pa, pb = _packed(rv, rrs[:1], lds[:1], fastq, False, True, False), _packed(rv, rrs[1:], lds[1:], fastq, False, False, True, False)
        ta, tb = rv.begin_packed_raw(pa), rv.begin_packed_raw(pb)
        ga, gb = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
        _check_call(ga, wa, ("in flight, first", fastq), True, False, pa)
        _check_call(gb, wb, ("in flight, second", fastq), False, True, pb, False)
        assert len(ga[6]) + len(gb[6]) + 1 == len(want[6])                # (the second read's name is one byte longer in the one call)
        # no window at all (N <= T): the records are formed on the host from the bases, every quality '#'
        r0 = rrs[0]
        for k in (T, 4):
            p = rv.pack_reads_raw([r0.raw, r0.raw], [r0.starts[:k - 3], r0.starts[:3]], [r0.feat_ev[:k - 3], r0.feat_ev[:3]], [r0.shift] * 2, [r0.scale] * 2, rv.T)
            b = np.concatenate([np.asarray(r0.bases, "S1")[:k - 3], np.asarray(r0.bases, "S1")[:3]])
            p = rv.with_device_records(rv.with_device_merge(p, b, fastq), _names(2))
            p[18][:] = 0xA5
            p[19][:] = -1
            seq, qual, off, rep, ed, edit_off, blob, rec_off = rv.run_packed_raw(p)
            assert rep is None and ed is None and seq.tobytes() == b.tobytes() and off.tolist() == [0, k - 3, k]
            b8 = b.view(np.uint8)
            _same((blob, rec_off), hs.pack_records(_names(2), b8, np.full(k, ord("#"), np.uint8) if fastq else None, off), ("no window", k, fastq))
            assert (p[18][int(rec_off[-1]):] == 0xA5).all()
    return out


def test_revise_reads_raw_records_equals_the_definition(species_models, short_reads, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for mode in MODES:
        rv.set_precision(mode)
        _end_to_end(rv, short_reads)
        assert rv.saturated() == (0, 0), mode
    rv.close()


# ---- 4. range guard ----------------------------------------------------------------------------------------------------------------
def test_range_guard_rerun_gives_the_f32_records(species_models, short_reads, monkeypatch):
    """The spiked read of tests/test_gpu_device_report.py behind a clean one: nrv_reads_raw_end runs the whole call again on the f32
    kernels, the merge and the two record launches behind it - blob and rec_off are the f32 mode's."""
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
        merged = tuple(hs.emit_calls(b8, el, a1, a2, qc, T))
        want[fq] = (hs.revision_report(b8, el, a1, a2, p1, p2, qc, T, TIE_EPS),) + merged + tuple(hs.revision_edits(b8, el, a1, a2, p1, p2, qc, T)) \
            + tuple(hs.pack_records(_names(2), *merged))
    assert rv.saturated()[1] == 0
    rv.set_precision("f16x2")
    for fq in (False, True):
        r0 = rv.saturated()[1]
        p = rv.with_device_edits(rv.with_device_report(rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, fq), TIE_EPS))
        p = rv.with_device_records(p, _names(2))
        p[18][:] = 0xA5
        got = rv.run_packed_raw(p)
        assert rv.saturated()[1] - r0 == 1, fq
        _check_call(got, want[fq], ("re-run", fq), True, True, p)
    rv.close()


# ---- 5. poison ---------------------------------------------------------------------------------------------------------------------
def test_poisoned_workspace_gives_the_same_records(species_models, short_reads, monkeypatch):
    clean = _engine(monkeypatch, *species_models["ecoli"])
    ref = _end_to_end(clean, short_reads)
    cases = {fq: report_records_case(fq) for fq in (False, True)}
    ref_k = {fq: _kernel(clean, c, "clean") for fq, c in cases.items()}
    clean.close()
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
        for p in range(2):
            got = _end_to_end(rv, short_reads)
            assert [k for k, _, _ in got] == [k for k, _, _ in ref]
            for (k, b, o), (_, b2, o2) in zip(ref, got):
                assert b.tobytes() == b2.tobytes() and np.array_equal(o, o2), (poison, p, k)
            for fq, c in cases.items():
                _same(_kernel(rv, c, (poison, p, fq)), ref_k[fq], (poison, p, fq))
        assert rv.saturated() == (0, 0), poison
        rv.close()


# ---- 6. command line ---------------------------------------------------------------------------------------------------------------
def _per_read(out, fmt):
    """{record name: (seq, qual | None)} of a run's per-read files: the second line, and the text behind `+\\n`."""
    recs = {}
    for f in sorted(os.listdir(out)):
        if "_out." not in f:
            continue
        text = open(out + f, "rb").read()
        head, rest = text.split(b"\n", 1)
        if fmt == "fastq":
            seq, qual = rest.split(b"+\n", 1)
            recs[head[1:]] = (seq, qual)
        else:
            recs[head[1:]] = (rest, None)
    return recs


def _combined(path, fmt):
    """{record name: (seq, qual | None)} of FILE, every record addressed through FILE.fai."""
    fastq = fmt == "fastq"
    blob = open(path, "rb").read()
    recs = parse_records(blob, fastq)
    names = [n for n, _, _ in recs]
    assert len(set(names)) == len(names)
    off = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in recs])])
    rec_off = np.concatenate([[0], np.cumsum([len(n) + (2 if fastq else 1) * len(s) + (6 if fastq else 3) for n, s, _ in recs])])
    assert open(path + ".fai").read().split("\n") == fai_lines(names, off, rec_off, fastq) + [""]
    for ln, (n, s, q) in zip(open(path + ".fai").read().split("\n"), recs):
        c = ln.split("\t")
        assert blob[int(c[2]):int(c[2]) + int(c[1])] == s and (not fastq or blob[int(c[5]):int(c[5]) + int(c[1])] == q)
    return {n: (s, q) for n, s, q in recs}


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_command_line_combined_records_come_from_the_device(tmp_path, monkeypatch, fmt):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NRV_CLI_GROUPS", "4")                               # a few reads per device call: several calls in flight
    d = tmp_path / "in"
    d.mkdir()
    src = sorted(glob.glob(os.path.join(FAST5, "*.fast5")) + glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))
    for i in range(10):
        shutil.copy(src[i % len(src)], d / f"s{i:02d}.fast5")
    forms, used = [], []
    real_begin, real_with = Reviser.begin_packed_raw, Reviser.with_device_records.__func__
    monkeypatch.setattr(Reviser, "begin_packed_raw", lambda self, packed: forms.append(len(packed)) or real_begin(self, packed))
    monkeypatch.setattr(Reviser, "with_device_records", classmethod(lambda cls, *a, **kw: used.append(1) or real_with(cls, *a, **kw)))
    base = ["-d", str(d), "-S", "ecoli", "-F", fmt, "--gpus", "1", "--thread", "4"]
    plain = str(tmp_path / "plain") + "/"
    assert cli.main(base + ["-o", plain, "--report", plain + "r.tsv", "--edits", plain + "ed"]) == 0
    want = _per_read(plain, fmt)
    assert len(want) == 10 and set(forms) == {7} and not used
    runs = (("merge", ["--device_merge"], 20), ("merge_stats", ["--device_merge", "--device_stats"], 20),
            ("merge_report", ["--device_merge", "--report"], 20), ("merge_edits", ["--device_merge", "--edits"], 20),
            ("merge_all", ["--device_merge", "--device_stats", "--report", "--edits"], 20), ("host", [], 7))
    for tag, extra, form in runs:
        del forms[:], used[:]
        out = str(tmp_path / tag) + "/"
        argv = base + ["-o", out, "--combined", out + "all." + fmt]
        for x in extra:
            argv += [x] + ([out + "r.tsv"] if x == "--report" else [out + "ed"] if x == "--edits" else [])
        assert cli.main(argv) == 0
        assert sorted(os.listdir(out)) == sorted(["all." + fmt, "all." + fmt + ".fai", "failed_reads.txt"] + (["r.tsv"] if "--report" in extra else [])
                                                 + (["ed"] if "--edits" in extra else [])), tag
        assert open(out + "failed_reads.txt").read() == ""
        assert forms and set(forms) == {form}, (tag, forms)
        assert (len(used) == len(forms)) if form == 20 else not used, (tag, len(used))      # the records came from the device call
        assert _combined(out + "all." + fmt, fmt) == want, tag
        if "--report" in extra:
            assert open(out + "r.tsv", "rb").read() == open(plain + "r.tsv", "rb").read()
        if "--edits" in extra:
            assert {f: open(out + "ed/" + f, "rb").read() for f in os.listdir(out + "ed")} == \
                {f: open(plain + "ed/" + f, "rb").read() for f in os.listdir(plain + "ed")}
