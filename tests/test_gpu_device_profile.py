"""The per-read quality and base profile counted on the device (MI355X only, -m gpu): csrc/nrv_profile.h through
nrv_merge_calls_profile, nrv_revise_reads_raw_profile_begin / nrv_revise_reads_raw_profile and the command line's --summary.

Everything is compared BIT FOR BIT - the counts are integers, nothing here has a tolerance.  hoststage.read_profile is the
definition (tests/test_read_profile_host.py holds it to the rule text).  The shipped E. coli weights:
  1. nrv_merge_calls_profile on tests/profile_cases.py (the tile layout of report_case, every Phred step planted one ulp either side,
     bases that are "other"), with and without q_thr, with a q_thr that is not prof_thr; seq / qual / off are nrv_merge_calls'; two
     passes; and on report_case(T) at T = 1, 2, 32;
  2. nrv_revise_reads_raw_profile on the two shortest fixture reads in one call, in each precision mode, FASTA and FASTQ, with and
     without device statistics, report, edit list and records, against the definition on nrv_predict_reads_raw's outputs in that
     mode; every other output is that of the same call without the profile;
  3. two calls in flight: each profile is its own;
  4. a call that trips the f16x2 range guard: one re-run, the profile is the f32 mode's - nothing is counted twice;
  5. handles created under NRV_POISON: the profiles unchanged;
  6. a call with N <= T: the block filled on the host;
  7. the command line with --summary on every route: one summary, the same read files, form 22 on the device-merge runs.
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
from report_cases import T, report_case

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "bf16x3", "f32"]
PATTERNS = {"qnan": 0x7FC00000, "m1500": 0xC4BB8000}
FAST5 = os.path.join(GOLD, "fast5")
INNER = ["merge", "report", "edits", "records", "records_only"]           # what the call carries beside the profile


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
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8].tolist())


def _eq(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


def _bases(rrs):
    return np.concatenate([np.asarray(r.bases, "S1") for r in rrs]).view(np.uint8)


def _definition(rv, rrs):
    """The profile of the host: nrv_predict_reads_raw in the engine's mode, then the host routes' function."""
    p1, p2, a1, a2 = rv.predict_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs],
                                          [r.shift for r in rrs], [r.scale for r in rrs])
    return cli.profile_rows(rv.T, _bases(rrs), [len(r.starts) for r in rrs], p1, p2, a1, a2)


def _packed(rv, rrs, lds, fastq, stats=False, inner="merge", profile=True):
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
    if inner in ("report", "edits", "records"):
        p = rv.with_device_report(p)
    if inner in ("edits", "records"):
        p = rv.with_device_edits(p)
    if inner in ("records", "records_only"):
        p = rv.with_device_records(p, [b"read_%d" % i for i in range(len(rrs))], hand_back=inner == "records")
    return rv.with_device_profile(p) if profile else p


def _check_call(got, plain, want, what):
    """A form-22 result: the profile last, every other output that of the same call without the profile, None where it carries none."""
    assert len(got) == 9 and len(plain) in (3, 4, 6, 8), what
    _same(got[8], want, what)
    assert all(_eq(g, p) for g, p in zip(got, plain)), what
    assert all(g is None for g in got[len(plain):8]), what
    off = got[2]
    assert np.array_equal(got[8][:, :42].sum(1).astype(np.int64), np.diff(off)), what
    assert np.array_equal(got[8][:, 42:47].sum(1).astype(np.int64), np.diff(off)) and not got[8][:, 47].any(), what


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
def test_merge_calls_profile_equals_the_definition(species_models, monkeypatch):
    c = profile_case()
    thr = cli.phred_thresholds()
    want = hs.read_profile(*hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"], T))
    assert (want[:, 1:41].sum(0) > 0).all() and want[:, 46].sum() > 0
    other = np.linspace(0.05, 0.95, 39).astype(np.float32)               # a q_thr that is not prof_thr: qual changes, the profile does not
    rv = _engine(monkeypatch, *species_models["ecoli"])
    ins = (c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"])
    for p in range(2):                                                   # a second pass on the same handle: nothing accumulates
        seq, qual, off, prof = rv.merge_calls_profile_device(*ins, thr)
        _same(prof, want, ("fastq", p))
        m = rv.merge_calls_device(*ins, thr)
        assert np.array_equal(seq, m[0]) and np.array_equal(qual, m[1]) and np.array_equal(off, m[2])
        _same(hs.read_profile(seq, qual, off), want, ("the written quality is the profile's", p))
        seq, qual, off, prof = rv.merge_calls_profile_device(*ins)        # FASTA: no quality is written, the profile is still filled
        _same(prof, want, ("fasta", p))
        m = rv.merge_calls_device(*ins[:4])
        assert qual is None and np.array_equal(seq, m[0]) and np.array_equal(off, m[2])
        seq, qual, off, prof = rv.merge_calls_profile_device(*ins, other)
        _same(prof, want, ("q_thr is not prof_thr", p))
        m = rv.merge_calls_device(*ins, other)
        assert np.array_equal(qual, m[1]) and not np.array_equal(qual, rv.merge_calls_device(*ins, thr)[1])
        seq, qual, off, prof = rv.merge_calls_profile_device(*ins, thr, other)
        _same(prof, hs.read_profile(seq, m[1], off), ("another prof_thr", p))
    # no window at all: filled on the host
    z = np.zeros(0, np.int8)
    seq, qual, off, prof = rv.merge_calls_profile_device(c["bases"][:9], [5, 0, 4], z, z, np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32), thr)
    _same(prof, hs.read_profile(seq, np.full(9, ord("#"), np.uint8), off), "no window")
    assert prof[:, 2].tolist() == [5, 0, 4] and qual.tobytes() == b"#" * 9
    rv.close()


@pytest.mark.parametrize("Tw", [1, 2, 32])
def test_merge_calls_profile_at_other_window_lengths(species_models, monkeypatch, Tw):
    c = report_case(T=Tw)
    c["qc"] = window_qc(c)
    want = hs.read_profile(*hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"], Tw))
    rv = _engine(monkeypatch, *species_models["ecoli"], Tw=Tw)
    ins = (c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"])
    for q_thr in (cli.phred_thresholds(), None):
        seq, qual, off, prof = rv.merge_calls_profile_device(*ins, q_thr)
        _same(prof, want, (Tw, q_thr is None))
        m = rv.merge_calls_device(*ins, q_thr)
        assert np.array_equal(seq, m[0]) and _eq(qual, m[1]) and np.array_equal(off, m[2])
    rv.close()


# ---- 2, 3, 6. end to end ---------------------------------------------------------------------------------------------------------
def _end_to_end(rv, short_reads, inners=INNER):
    """Every end-to-end form on the two reads -> [(name, profile)]; compared with the definition inside."""
    out = []
    rrs, lds = [r for r, _ in short_reads], [ld for _, ld in short_reads]
    want = _definition(rv, rrs)                                           # the FASTQ form's, whatever the call writes
    assert want[:, 3:41].sum() > 0
    for fastq in (False, True):
        for stats in (False, True):
            for inner in inners:
                got = rv.run_packed_raw(_packed(rv, rrs, lds, fastq, stats, inner))
                plain = rv.run_packed_raw(_packed(rv, rrs, lds, fastq, stats, inner, profile=False))
                _check_call(got, plain, want, ("one call", fastq, stats, inner))
                assert (got[1] is not None) == (fastq and inner != "records_only")
                out.append((f"one call {fastq} {stats} {inner}", got[8].copy()))
        # 3. two calls in flight, one read each
        wa, wb = _definition(rv, rrs[:1]), _definition(rv, rrs[1:])
        ta = rv.begin_packed_raw(_packed(rv, rrs[:1], lds[:1], fastq))
        tb = rv.begin_packed_raw(_packed(rv, rrs[1:], lds[1:], fastq))
        ga, gb = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
        _same(ga[8], wa, ("in flight, first", fastq))
        _same(gb[8], wb, ("in flight, second", fastq))
        assert not np.array_equal(ga[8], gb[8])
        _same(np.concatenate([ga[8], gb[8]]), want, ("the two calls are the one call's reads", fastq))
        # 6. no window at all (N <= T): filled on the host
        r0 = rrs[0]
        for k in (rv.T, 4):
            p = rv.pack_reads_raw([r0.raw, r0.raw], [r0.starts[:k - 3], r0.starts[:3]], [r0.feat_ev[:k - 3], r0.feat_ev[:3]], [r0.shift] * 2, [r0.scale] * 2, rv.T)
            b = np.concatenate([np.asarray(r0.bases, "S1")[:k - 3], np.asarray(r0.bases, "S1")[:3]])
            got = rv.run_packed_raw(rv.with_device_profile(rv.with_device_merge(p, b, fastq)))
            z = np.zeros(0, np.int8)
            _same(got[8], cli.profile_rows(rv.T, b, [k - 3, 3], np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32), z, z), ("no window", k))
            assert got[8][:, 2].tolist() == [k - 3, 3] and got[8][:, :42].sum() == k and got[0].tobytes() == b.tobytes()
    return out


def test_revise_reads_raw_profile_equals_the_definition(species_models, short_reads, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for mode in MODES:
        rv.set_precision(mode)
        _end_to_end(rv, short_reads)
        assert rv.saturated() == (0, 0), mode
    rv.close()


def test_profile_call_refuses_missing_blocks(species_models, short_reads, monkeypatch):
    from nanoreviser_amd.engine import NrvError
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rrs, lds = [r for r, _ in short_reads][:1], [ld for _, ld in short_reads][:1]
    p = _packed(rv, rrs, lds, True)
    for k in (20, 21):                                                   # prof_thr and profile are both required
        with pytest.raises(NrvError):
            rv.run_packed_raw(p[:k] + (None,) + p[k + 1:])
    _same(rv.run_packed_raw(p)[8], _definition(rv, rrs), "the handle is usable after a refusal")
    rv.close()


# ---- 4. range guard --------------------------------------------------------------------------------------------------------------
def test_range_guard_rerun_counts_once(species_models, short_reads, monkeypatch):
    """The spiked read of tests/test_gpu_device_report.py behind a clean one: nrv_reads_raw_end runs the whole call again on the f32
    kernels, zeroes the profile block and counts again - the profile is the f32 mode's, not a sum of two passes."""
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
    want = cli.profile_rows(T, bases.view(np.uint8), el, p1, p2, a1, a2)
    assert rv.saturated()[1] == 0
    rv.set_precision("f16x2")
    for fq in (False, True):
        r0 = rv.saturated()[1]
        p = rv.with_device_profile(rv.with_device_report(rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, fq)))
        got = rv.run_packed_raw(p)
        assert rv.saturated()[1] - r0 == 1, fq
        _same(got[8], want, ("re-run", fq))
        assert np.array_equal(got[8][:, :42].sum(1).astype(np.int64), np.diff(got[2]))
        assert np.array_equal(got[3][:, 2].astype(np.int64), np.diff(got[2]))                 # the report of the same pass
    rv.close()


# ---- 5. poison -------------------------------------------------------------------------------------------------------------------
def test_poisoned_workspace_gives_the_same_profiles(species_models, short_reads, monkeypatch):
    clean = _engine(monkeypatch, *species_models["ecoli"])
    ref = _end_to_end(clean, short_reads, ["merge", "records"])
    clean.close()
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
        for p in range(2):
            got = _end_to_end(rv, short_reads, ["merge", "records"])
            assert [k for k, _ in got] == [k for k, _ in ref]
            for (k, x), (_, y) in zip(ref, got):
                _same(y, x, (poison, p, k))
        assert rv.saturated() == (0, 0), poison
        rv.close()


# ---- 7. command line -------------------------------------------------------------------------------------------------------------
def _records(blob, fmt):
    """[(name, sequence, quality | None)] of a --combined file or of one per-read file."""
    lines = blob.split(b"\n")
    if fmt == "fasta":
        return [(lines[i][1:], lines[i + 1], None) for i in range(0, len(lines) - 1, 2)]
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_command_line_summary_is_the_same_on_every_path(tmp_path, monkeypatch, fmt):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_SUMMARY"):
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
    outs, sums = {}, {}
    runs = (("plain", None, 7), ("plain_combined", None, 20), ("host", [], 7), ("host_stats", ["--device_stats"], 9),
            ("merge", ["--device_merge"], 22), ("merge_stats", ["--device_merge", "--device_stats"], 22),
            ("combined", ["--device_merge", "--combined"], 22))
    for tag, extra, form in runs:
        del forms[:]
        out = str(tmp_path / tag) + "/"
        sm = str(tmp_path / (tag + ".tsv"))
        argv = ["-d", str(d), "-o", out, "-S", "ecoli", "-F", fmt, "--gpus", "1", "--thread", "4"]
        if tag == "plain_combined":
            argv += ["--device_merge", "--combined", out + "all." + fmt]
        elif extra is not None:
            argv += [x for e in extra for x in ([e, out + "all." + fmt] if e == "--combined" else [e])] + ["--summary", sm]
        assert cli.main(argv) == 0
        outs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        assert outs[tag]["failed_reads.txt"] == b"" and len(outs[tag]) == (3 if "combined" in tag else 11)
        assert forms and set(forms) == {form}, (tag, forms)
        if extra is not None:
            sums[tag] = open(sm, "rb").read()
        else:
            assert not os.path.exists(sm)
        assert not glob.glob(str(tmp_path / "*.part*")) and not glob.glob(out + "*.part*")
    assert all(outs[t] == outs["plain"] for t in ("host", "host_stats", "merge", "merge_stats"))
    assert outs["combined"] == outs["plain_combined"]
    assert all(s == sums["host"] for s in sums.values()) and len(sums) == 5
    lines = sums["host"].decode().split("\n")
    assert lines[0] == cli.SUMMARY_HEADER and len(lines) == 1 + 10 + 2 + 1
    assert lines[-3].startswith("#total\trevised\t") and [ln.split("\t")[0] for ln in lines[1:11]] == sorted(os.listdir(d))
    combined = {n.decode(): (s, q) for n, s, q in _records(outs["combined"]["all." + fmt], fmt)}
    lengths = []
    for ln in lines[1:11]:
        c = ln.split("\t")
        pl = outs["plain"][c[0].split(".")[0] + "_out." + fmt].split(b"\n")   # (the per-read FASTQ has '+' at the end of the sequence line)
        body, qual = (pl[1], None) if fmt == "fasta" else (pl[1][:-1], pl[2])
        assert combined[hs.record_name(c[0]).decode()] == (body, qual)
        assert c[1] == "revised" and int(c[2]) == len(body) == sum(int(x) for x in c[9:14])
        assert [int(x) for x in c[9:13]] == [body.count(b) for b in (b"A", b"C", b"G", b"T")]
        assert 1 <= float(c[3]) <= 40 and 1 <= int(c[4]) <= 40 and int(c[2]) >= int(c[5]) >= int(c[6]) >= int(c[7]) >= 0
        if fmt == "fastq":
            assert int(c[5]) == sum(ch >= ord("+") for ch in qual)
        lengths.append(int(c[2]))
    assert lines[-2] == f"#reads\t10\t0\t{cli.n50(lengths)}" and int(lines[-3].split("\t")[2]) == sum(lengths)
