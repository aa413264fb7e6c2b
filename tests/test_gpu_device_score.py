"""Both classifiers scored against per-base labels on the device (MI355X only, -m gpu): csrc/nrv_score.h through
nrv_merge_calls_score and nrv_revise_reads_raw_score_begin / nrv_revise_reads_raw_score.

Everything is compared BIT FOR BIT - the counts and the loss are integers, nothing here has a tolerance.  hoststage.score_calls is
the definition (tests/test_score_host.py holds it to the rule text):
  1. nrv_merge_calls_score on tests/score_cases.py against the definition, two passes over one handle, with and without p1 / p2;
     seq / qual / off are nrv_merge_calls';
  2. the same call at T = 1, 2, 12, 13, 32 through handles made with `with_window`;
  3. nrv_revise_reads_raw_score on the two shortest fixture reads in one call, in each precision mode, with and without the report
     in the same call, against the definition on that mode's nrv_predict_reads_raw outputs; the labels are seeded random valid
     bytes with 0xFF clips - the scorer does not care where labels come from;
  4. two calls in flight, one read each: each block is its own, together they are the one call's rows;
  5. a call that trips the f16x2 range guard: one re-run, the block is the f32 mode's, not a sum of two;
  6. handles created under NRV_POISON: unchanged blocks;
  7. N <= T: all zeros, filled on the host;
  8. NULL labels / score_thr / score are refused under the entry point's name and the next call on the handle succeeds;
  9. the command line: a --labels run, then --score --labels_from on the host route and with --device_merge (every call of form
     36): one score file byte for byte, the read files a plain run's; a read without a labels file, one with a stale file.  Only
     the structure of the file is asserted - no accuracy threshold has been measured."""
import glob
import os
import shutil

import numpy as np
import pytest

import score_cases
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd.engine import NrvError
from conftest import GOLD
from report_cases import T, TIE_EPS
from test_gpu_infix import mutate, random_seq, revcomp           # the regions of the command-line test: that module's own helpers
from test_score_cli_host import _check_structure

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "bf16x3", "f32"]
PATTERNS = {"qnan": 0x7FC00000, "m1500": 0xC4BB8000}


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
def short_reads(reads):
    """The two shortest fixture reads as RawReadTensors."""
    out = []
    for k in reads.keys:
        _, rd, _ = reads(k)
        out.append(hs.read_tensors_raw(rd))
    return sorted(out, key=lambda r: len(r.starts))[:2]


def _same(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8].tolist())


def _kernel_on_case(rv, T_, passes=1):
    c, with_rows, without = score_cases.cached_case(T=T_)
    ins = (c["bases"], c["ev_len"], c["a1"], c["a2"])
    thr = cli.phred_thresholds()
    for p in range(passes):
        seq, qual, off, sc = rv.merge_calls_score_device(*ins, c["labels"], c["p1"], c["p2"], thr, c["score_thr"])
        _same(sc, with_rows, ("fastq", T_, p))
        _same(sc, hs.score_calls(*ins, c["p1"], c["p2"], c["labels"], c["score_thr"], T_), ("fastq, the definition", T_, p))
        m = rv.merge_calls_device(*ins, c["p1"], c["p2"], thr)
        assert np.array_equal(seq, m[0]) and np.array_equal(qual, m[1]) and np.array_equal(off, m[2])
        seq, qual, off, sc = rv.merge_calls_score_device(*ins, c["labels"], c["p1"], c["p2"], None, c["score_thr"])
        _same(sc, with_rows, ("rows without a quality", T_, p))
        m = rv.merge_calls_device(*ins)
        assert qual is None and np.array_equal(seq, m[0]) and np.array_equal(off, m[2])
        seq, qual, off, sc = rv.merge_calls_score_device(*ins, c["labels"], score_thr=c["score_thr"])
        _same(sc, without, ("bare", T_, p))
        assert qual is None and np.array_equal(seq, m[0]) and not sc[:, 63:225].any()
        # thresholds of its own: another table moves the bins and nothing else
        other = np.linspace(0.05, 0.99, 39).astype(np.float32)
        sc2 = rv.merge_calls_score_device(*ins, c["labels"], c["p1"], c["p2"], thr, other)[3]
        _same(sc2, hs.score_calls(*ins, c["p1"], c["p2"], c["labels"], other, T_), ("another table", T_, p))
        assert np.array_equal(sc2[:, :63], with_rows[:, :63]) and np.array_equal(sc2[:, 223:], with_rows[:, 223:])


# ---- 1, 2. the kernel alone ------------------------------------------------------------------------------------------------------
def test_merge_calls_score_equals_the_definition(species_models, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    assert rv.T == T
    _kernel_on_case(rv, T, passes=2)
    rv.close()


@pytest.mark.parametrize("T_", (1, 2, 12, 13, 32))
def test_merge_calls_score_at_other_window_lengths(species_models, monkeypatch, T_):
    m1, m2 = species_models["ecoli"]
    rv = _engine(monkeypatch, m1.with_window(T_), m2.with_window(T_))
    assert rv.T == T_
    _kernel_on_case(rv, T_)
    rv.close()


# ---- 3, 4, 7. end to end ---------------------------------------------------------------------------------------------------------
def _bases(rrs):
    return np.concatenate([np.asarray(r.bases, "S1") for r in rrs]).view(np.uint8)


def _labels_for(rrs, seed=91):
    """Seeded random valid bytes, one per event, with 0xFF clips at both ends of every read and a run inside."""
    rng = np.random.default_rng(seed)
    parts = []
    for r in rrs:
        n = len(r.starts)
        lab = np.array(score_cases.VALID, np.uint8)[rng.integers(0, 20, n)]
        lab[:int(rng.integers(8, 40))] = 0xFF
        lab[n - int(rng.integers(8, 40)):] = 0xFF
        lab[n // 2:n // 2 + 25] = 0xFF
        lab[n // 3:n // 3 + 4] = [0x00, 0x06, 0x0F, 0xE3]
        parts.append(lab)
    return np.concatenate(parts)


def _packed(rv, rrs, labels, fastq, report):
    p = rv.pack_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs], [r.shift for r in rrs], [r.scale for r in rrs], rv.T)
    p = rv.with_device_merge(p, _bases(rrs), fastq)
    if report:
        p = rv.with_device_report(p, TIE_EPS)
    return rv.with_device_score(p, labels)


def _definition(rv, rrs, labels, fastq):
    """(score, report, seq, qual, off) of the host: nrv_predict_reads_raw in the engine's mode, then the definitions."""
    p1, p2, a1, a2 = rv.predict_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs], [r.shift for r in rrs],
                                          [r.scale for r in rrs])
    el, b = [len(r.starts) for r in rrs], _bases(rrs)
    qc = cli.phred_chars(p1, p2, a1, a2) if fastq else None
    return (hs.score_calls(b, el, a1, a2, p1, p2, labels, cli.phred_thresholds(), rv.T), hs.revision_report(b, el, a1, a2, p1, p2, qc, rv.T, TIE_EPS)) \
        + tuple(hs.emit_calls(b, el, a1, a2, qc, rv.T))


def _check_call(got, want, report, what):
    assert len(got) == 14, (what, len(got))
    seq, qual, off, rep = got[:4]
    assert all(x is None for x in got[4:13]), what                       # blocks the tuple does not carry
    _same(got[13], want[0], what)
    assert (rep is None) if not report else np.array_equal(rep, want[1]), what
    assert np.array_equal(seq, want[2]) and np.array_equal(off, want[4]), what
    assert (qual is None) == (want[3] is None) and (qual is None or np.array_equal(qual, want[3])), what


def _end_to_end(rv, rrs):
    """Every end-to-end form on the two reads -> [(name, score block)]; compared with the definition inside."""
    out = []
    labels = _labels_for(rrs)
    n0 = len(rrs[0].starts)
    for fastq in (False, True):
        want = _definition(rv, rrs, labels, fastq)
        assert (want[0][:, 1] > 0).all() and (want[0][:, 1] < want[0][:, 0] - 30).all()      # the clips and the run reach the windows
        for report in (False, True):
            got = rv.run_packed_raw(_packed(rv, rrs, labels, fastq, report))
            _check_call(got, want, report, ("one call", fastq, report))
            out.append((f"one call {fastq} {report}", got[13].copy()))
        # 4. two calls in flight, one read each
        ta = rv.begin_packed_raw(_packed(rv, rrs[:1], labels[:n0], fastq, True))
        tb = rv.begin_packed_raw(_packed(rv, rrs[1:], labels[n0:], fastq, False))
        ga, gb = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
        _check_call(ga, _definition(rv, rrs[:1], labels[:n0], fastq), True, ("in flight, first", fastq))
        _check_call(gb, _definition(rv, rrs[1:], labels[n0:], fastq), False, ("in flight, second", fastq))
        assert not np.array_equal(ga[13], gb[13])
        _same(np.concatenate([ga[13], gb[13]]), want[0], ("the two calls are the one call's rows", fastq))
        # 7. no window at all (N <= T): all zeros, filled on the host
        r0 = rrs[0]
        for k in (rv.T, 4):
            p = rv.pack_reads_raw([r0.raw, r0.raw], [r0.starts[:k - 3], r0.starts[:3]], [r0.feat_ev[:k - 3], r0.feat_ev[:3]], [r0.shift] * 2, [r0.scale] * 2, rv.T)
            b = np.concatenate([np.asarray(r0.bases, "S1")[:k - 3], np.asarray(r0.bases, "S1")[:3]])
            p = rv.with_device_score(rv.with_device_merge(p, b, fastq), np.full(k, 5, np.uint8))
            p[35][:] = 77                                                    # the caller's block holds something else
            got = rv.run_packed_raw(p)
            assert got[13].shape == (2, 248) and not got[13].any(), k
            z = np.zeros(0, np.int8)
            _same(got[13], hs.score_calls(b.view(np.uint8), [k - 3, 3], z, z, None, None, np.full(k, 5, np.uint8), cli.phred_thresholds(), rv.T), ("no window", k))
            assert got[0].tobytes() == b.tobytes() and got[2].tolist() == [0, k - 3, k]
    return out


def test_revise_reads_raw_score_equals_the_definition(species_models, short_reads, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for mode in MODES:
        rv.set_precision(mode)
        _end_to_end(rv, short_reads)
        assert rv.saturated() == (0, 0), mode
    rv.close()


# ---- 5. range guard --------------------------------------------------------------------------------------------------------------
def test_range_guard_rerun_counts_once(species_models, short_reads, monkeypatch):
    """The spiked read of tests/test_gpu_device_report.py behind a clean one: nrv_reads_raw_end runs the whole call again on the f32
    kernels, zeroes the score block and counts again - the block is the f32 mode's, not a sum of two."""
    other, rr = short_reads
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
    el = [len(other.starts), N]
    labels = np.array(score_cases.VALID, np.uint8)[np.random.default_rng(12).integers(0, 20, sum(el))]
    labels[:30] = 0xFF
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rv.set_precision("f32")
    p1, p2, a1, a2 = rv.predict_reads_raw(*args)
    want = hs.score_calls(bases.view(np.uint8), el, a1, a2, p1, p2, labels, cli.phred_thresholds(), T)
    assert rv.saturated()[1] == 0
    rv.set_precision("f16x2")
    for report in (False, True):
        r0 = rv.saturated()[1]
        p = rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, True)
        p = rv.with_device_score(rv.with_device_report(p, 0.2) if report else p, labels)
        got = rv.run_packed_raw(p)
        assert rv.saturated()[1] - r0 == 1, report
        _same(got[13], want, ("re-run", report))
        assert got[13][:, 0].tolist() == [el[0] - T, N - T] and got[13][:, 1].tolist() == [el[0] - T - 25, N - T]   # events 5 .. 29 of the first read have no label
    rv.close()


# ---- 6. poison -------------------------------------------------------------------------------------------------------------------
def test_poisoned_workspace_gives_the_same_blocks(species_models, short_reads, monkeypatch):
    clean = _engine(monkeypatch, *species_models["ecoli"])
    ref = _end_to_end(clean, short_reads)
    clean.close()
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
        got = _end_to_end(rv, short_reads)
        assert [k for k, _ in got] == [k for k, _ in ref]
        for (k, x), (_, y) in zip(ref, got):
            _same(y, x, (poison, k))
        _kernel_on_case(rv, T)
        assert rv.saturated() == (0, 0), poison
        rv.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_null_arguments_are_refused_by_name(species_models, short_reads, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rrs = short_reads[:1]
    labels = _labels_for(rrs)
    want = _definition(rv, rrs, labels, True)
    text = "nrv_revise_reads_raw_score_begin: null labels / score_thr / score"
    for at in (33, 34, 35):
        for begin in (False, True):
            p = _packed(rv, rrs, labels, True, False)
            p = p[:at] + (None,) + p[at + 1:]
            with pytest.raises(NrvError) as e:
                rv.begin_packed_raw(p) if begin else rv.run_packed_raw(p)
            assert e.value.code == -1 and str(e.value).endswith(": " + text), (at, begin, str(e.value))
            assert rv._lib.nrv_last_error(rv._h).decode() == text
            _check_call(rv.run_packed_raw(_packed(rv, rrs, labels, True, False)), want, False, ("after a refusal", at, begin))
    c, with_rows, _ = score_cases.cached_case()
    ins = rv._merge_inputs(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], None, True)
    blk = np.zeros((len(c["ev_len"]), 248), np.uint64)
    from nanoreviser_amd.engine import _SCORE, _marshal
    for at in range(3):
        more = [c["labels"], c["score_thr"], blk]
        more[at] = None
        with pytest.raises(NrvError) as e:
            rv._merge_call("nrv_merge_calls_score", *ins, *_marshal(more, _SCORE[0]))
        assert e.value.code == -1 and str(e.value).endswith(": nrv_merge_calls_score: null labels / score_thr / score"), (at, str(e.value))
        _same(rv.merge_calls_score_device(c["bases"], c["ev_len"], c["a1"], c["a2"], c["labels"], c["p1"], c["p2"], None, c["score_thr"])[3],
              with_rows, ("after a refusal", at))
    rv.close()


# ---- 9. command line -------------------------------------------------------------------------------------------------------------
def test_command_line_score_is_the_same_on_the_device_route(tmp_path, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_SUMMARY",
              "NRV_TRIM_Q", "NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES", "NRV_INFIX", "NRV_LABELS", "NRV_LABELS_BUDGET", "NRV_SCORE",
              "NRV_LABELS_FROM"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                               # several device calls, one in flight behind the other
    d = tmp_path / "in"
    d.mkdir()
    src = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")) + glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))
    n = 4
    for i in range(n):
        shutil.copy(src[i % len(src)], d / f"s{i:02d}.fast5")
    names = [f"s{i:02d}.fast5" for i in range(n)]
    forms = []
    real_begin = Reviser.begin_packed_raw
    monkeypatch.setattr(Reviser, "begin_packed_raw", lambda self, packed: forms.append(len(packed)) or real_begin(self, packed))
    fa, ldir = str(tmp_path / "regions.fa"), str(tmp_path / "labels")
    outs, scores = {}, {}
    for tag, extra in (("plain", []), ("A", ["--device_merge", "--truth", fa, "--infix", str(tmp_path / "A.inf"), "--labels", ldir]),
                       ("B", ["--score", str(tmp_path / "B.tsv"), "--labels_from", ldir]),
                       ("C", ["--device_merge", "--score", str(tmp_path / "C.tsv"), "--labels_from", ldir]),
                       ("D", ["--device_merge", "--report", str(tmp_path / "D.rep"), "--score", str(tmp_path / "D.tsv"), "--labels_from", ldir])):
        del forms[:]
        out = str(tmp_path / tag) + "/"
        assert cli.main(["-d", str(d), "-o", out, "-S", "ecoli", "--gpus", "1", "--thread", "4"] + extra) == 0
        outs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        assert outs[tag]["failed_reads.txt"] == b"" and outs[tag] == outs["plain"], tag
        assert forms and set(forms) == {{"plain": 7, "A": 33, "B": 7, "C": 36, "D": 36}[tag]}, (tag, forms)
        if tag in "BCD":
            scores[tag] = open(str(tmp_path / (tag + ".tsv")), "rb").read()
            assert not glob.glob(str(tmp_path / "*.part*"))
        if tag == "plain":                          # the regions: a seeded 5 % mutation of what the plain run wrote, between flanks
            rng = np.random.default_rng(8)
            with open(fa, "w") as fp:
                for i in range(n):
                    if i != 2:                                              # one read left out; every second region on the other strand
                        t = random_seq(rng, 64 + i) + mutate(rng, outs[tag][f"s{i:02d}_out.fasta"].split(b"\n")[1], 0.05) + random_seq(rng, 80)
                        t = (revcomp(t) if i % 2 else t).decode()
                        fp.write(f">s{i:02d}{'.fast5' if i % 2 else ''}\n" + "".join(t[k:k + 70] + "\n" for k in range(0, len(t), 70)))
        if tag == "A":                              # s02 has no file; the file of s03 gets another base at one place
            assert sorted(os.listdir(ldir)) == ["labels.tsv"] + [f"s{i:02d}_labels.txt" for i in range(n) if i != 2]
            f3 = os.path.join(ldir, "s03_labels.txt")
            lines = open(f3).read().split("\n")
            lines[1] = lines[1][:50] + ("A" if lines[1][50] != "A" else "C") + lines[1][51:]
            open(f3, "w").write("\n".join(lines))
    assert scores["C"] == scores["B"] and scores["D"] == scores["B"]
    status = {"s00.fast5": "scored", "s01.fast5": "scored", "s02.fast5": "no_labels", "s03.fast5": "stale_labels"}
    _check_structure(scores["B"], names, status, ldir)
