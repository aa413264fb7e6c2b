"""Substitution / insertion / deletion counts against a truth set on the device (MI355X only, -m gpu): csrc/nrv_errclass.h through
nrv_edit_classes, nrv_merge_calls_errclass, nrv_revise_reads_raw_errclass_begin / nrv_revise_reads_raw_errclass and the command
line's --error_classes.

Everything is compared BIT FOR BIT - (d, M) is a unique pair of integers, nothing here has a tolerance.
hoststage.edit_classes and hoststage.read_error_classes are the definitions (tests/test_errclass_host.py holds them to three
references that share no code with them); the planted pairs are compared with those references directly.  The shipped E. coli
weights:
  1. nrv_edit_classes on tests/errclass_cases.py's planted pairs - truth lengths on both sides of a lane's strip and of a stripe,
     one stripe and a strip, two stripes and a character, reads on both sides of lane 0's feed chunks, 3 characters against more
     than one stripe, AC / CA and 400 pairs of 3 to 5 characters, Ns, runs across the boundaries, empty truths first, in the
     middle and last - in one call, two passes over one handle; offsets that do not ascend from 0 are refused under the entry
     point's name and the handle stays usable;
  2. nrv_merge_calls_errclass on profile_case and report_case(T) at T = 1, 2, 11, 32; N <= T on the host;
  3. nrv_revise_reads_raw_errclass on the two shortest fixture reads in one call, in each precision mode, alone and behind report +
     edits + records + profile + trim, against the definition on nrv_predict_reads_raw's outputs in that mode; the dist columns
     are those of the accuracy block of the same call, every other output that of the form 30 call;
  4. a bad truth_off is refused by name; 5. a call that trips the f16x2 range guard (one re-run, the f32 mode's classes);
  6. handles under NRV_POISON, both patterns, two passes, the planted pairs of more than one stripe (they read the carry words)
     included; 7. the command line: form 31 with --device_merge, the host route's file byte for byte.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from accuracy_cases import mutate, truth_for_reads
from conftest import GOLD
from errclass_cases import planted_cases, reference, strip
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from profile_cases import profile_case
from report_cases import T, report_case
from test_gpu_device_accuracy import (FAST5, PATTERNS, _bases, _engine, _eq, _merged, _packed, _same, _truths_for_case,  # noqa: F401
                                      short_reads, truth_of_short_reads)

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "bf16x3", "f32"]


@pytest.fixture(scope="module")
def planted():
    """(names, truths, reads, the references' (d, M) as int64[n][2] with -1 / -1 for an empty truth): computed once."""
    cases, _ = planted_cases()
    ref = reference()
    names = list(cases)
    truths, rds = [cases[k][0] for k in names], [cases[k][1] for k in names]
    want = np.array([ref[k] if cases[k][0] else (-1, -1) for k in names], np.int64)
    return names, truths, rds, want


# ---- 1. the kernel on planted pairs -------------------------------------------------------------------------------------------------
def test_edit_classes_on_planted_pairs(species_models, planted, monkeypatch):
    from nanoreviser_amd import engine as E
    names, truths, rds, want = planted
    S = 64 * strip()
    assert (want[:, 0] == -1).sum() >= 3 and want[0, 0] == -1 and want[-1, 0] == -1 and len(want) > 450
    assert want[names.index("AC / CA")].tolist() == [2, 1]
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for p in range(2):                                                   # a second pass over the same handle: the same pairs
        d, M = rv.edit_classes_device(truths, rds)
        got = np.stack([d, M], 1)
        bad = [(names[i], got[i].tolist(), want[i].tolist()) for i in np.flatnonzero((got != want).any(1))]
        assert not bad and d.dtype == M.dtype == np.int64, (p, bad[:8])
    # one pair at a time: a grid of one wave
    for k in (names.index(f"m={S + 1} mutated 10 %*"), names.index("m=64 one character*"), names.index("m=1 empty*"), names.index("AC / CA")):
        d, M = rv.edit_classes_device(truths[k:k + 1], rds[k:k + 1])
        assert [d.tolist(), M.tolist()] == [[int(want[k, 0])], [int(want[k, 1])]], names[k]
    assert rv.edit_classes_device([], [])[0].size == 0
    a = np.frombuffer(b"ACGTACGT", np.uint8)
    for bad_a, bad_b in (([1, 4, 8], [0, 4, 8]), ([0, 5, 4], [0, 4, 8]), ([0, 4, 8], [0, 9, 8]), ([0, 4, 8], [2, 4, 8])):
        with pytest.raises(E.NrvError, match="nrv_edit_classes"):       # refused under the entry point's name
            rv.edit_classes_offsets(a, bad_a, a, bad_b)
    d, M = rv.edit_classes_offsets(a, [0, 4, 8], a, [0, 3, 8])          # the handle is usable afterwards
    assert d.tolist() == [1, 1] and M.tolist() == [3, 4]
    rv.close()


# ---- 2. behind the merge --------------------------------------------------------------------------------------------------------------
def _merge_errclass_checks(rv, c, Tw):
    truth, toff, e = _truths_for_case(c, Tw, 100 + Tw)
    thr = cli.phred_thresholds()
    ins = (c["bases"], c["ev_len"], c["a1"], c["a2"])
    seq_w, _, off_w = hs.emit_calls(*ins, None, Tw)
    want = hs.read_error_classes(c["bases"], c["ev_len"], seq_w, off_w, truth, toff)
    assert want[e].tolist() == [8, 8, 0, 8, 0, 0] and (want[:, 0] == 0).sum() >= 4
    assert ((want[:, 1] != want[:, 3]) | (want[:, 2] != want[:, 4])).sum() >= (3 if Tw > 2 else 1)
    for q_thr in (None, thr):
        seq, qual, off, ec = rv.merge_calls_errclass_device(*ins, truth, toff, c["p1"], c["p2"], q_thr)
        _same(ec, want, (Tw, q_thr is None))
        m = rv.merge_calls_device(*ins, c["p1"], c["p2"], q_thr)
        assert np.array_equal(seq, m[0]) and _eq(qual, m[1]) and np.array_equal(off, m[2])
    _same(rv.merge_calls_errclass_device(*ins, b"", np.zeros(len(c["ev_len"]) + 1, np.int64))[3], np.zeros_like(want), (Tw, "no truth"))
    return want


def test_merge_calls_errclass_equals_the_definition(species_models, monkeypatch):
    from nanoreviser_amd import engine as E
    c = profile_case()
    rv = _engine(monkeypatch, *species_models["ecoli"])
    _merge_errclass_checks(rv, c, T)
    # no window at all (N <= T): filled on the host, out = in
    z = np.zeros(0, np.int8)
    b = np.frombuffer(b"ACGTANNCA", np.uint8)
    truth, toff = np.frombuffer(b"ACTTAGGNNCA", np.uint8), np.array([0, 6, 8, 11], np.int64)
    seq, qual, off, ec = rv.merge_calls_errclass_device(b, [5, 0, 4], z, z, truth, toff)
    assert seq.tobytes() == b.tobytes() and off.tolist() == [0, 5, 5, 9]
    _same(ec, hs.read_error_classes(b, [5, 0, 4], seq, off, truth, toff), "no window")
    assert ec.tolist() == [[6, 2, 4, 2, 4, 0], [2, 2, 0, 2, 0, 0], [3, 2, 2, 2, 2, 0]]
    ins = rv._merge_inputs(c["bases"], c["ev_len"], c["a1"], c["a2"], None, None, None, False)
    R = len(c["ev_len"])
    for bad in (np.arange(1, R + 2), np.arange(R, -1, -1)):              # the C entry point refuses them under its own name
        more = E._marshal((np.zeros(R + 2, np.uint8), bad.astype(np.int64), np.zeros((R, 6), np.uint64)), E._TRUTH[0])
        with pytest.raises(E.NrvError, match="nrv_merge_calls_errclass"):
            rv._merge_call("nrv_merge_calls_errclass", *ins, *more)
    rv.close()


@pytest.mark.parametrize("Tw", [1, 2, 32])
def test_merge_calls_errclass_at_other_window_lengths(species_models, monkeypatch, Tw):
    rv = _engine(monkeypatch, *species_models["ecoli"], Tw=Tw)
    _merge_errclass_checks(rv, report_case(T=Tw), Tw)
    rv.close()


# ---- 3 - 6. end to end ----------------------------------------------------------------------------------------------------------------
def _definition(rv, rrs, truth, toff):
    seq, off = _merged(rv, rrs)
    return hs.read_error_classes(_bases(rrs), [len(r.starts) for r in rrs], seq, off, truth, toff)


def _packed31(rv, rrs, fastq, inner, truth):
    return rv.with_device_error_classes(_packed(rv, rrs, fastq, inner, truth))


def _check_call(got, plain, want, what):
    """A form-31 result: the error classes last, every other output that of the form 30 call, the dist columns the accuracy's."""
    assert len(got) == 12 and len(plain) == 11, what
    _same(got[11], want, what)
    for k, (g, p) in enumerate(zip(got, plain)):
        assert _eq(g, p), (what, k)
    assert np.array_equal(got[11][:, [0, 1, 3]], got[10][:, :3]) and not got[11][:, 5].any(), what


def _end_to_end(rv, short_reads, truth, toff):
    """The end-to-end forms on the two reads -> [(name, error classes)]; compared with the definition inside."""
    out = []
    rrs = [r for r, _ in short_reads]
    want = _definition(rv, rrs, truth, toff)
    # a vacuous pass is a failure: the revision moved the classes of both reads, and neither onto its truth
    assert (want[:, 0] == np.diff(toff)).all() and (want[:, 3] > 0).all(), want.tolist()
    assert (want[:, 1] != want[:, 3]).all(), want.tolist()
    for fastq, inner in ((False, "alone"), (True, "all")):
        got = rv.run_packed_raw(_packed31(rv, rrs, fastq, inner, (truth, toff)))
        plain = rv.run_packed_raw(_packed(rv, rrs, fastq, inner, (truth, toff)))
        _check_call(got, plain, want, ("one call", fastq, inner))
        out.append((f"one call {fastq} {inner}", got[11].copy()))
    # two calls in flight, one read each
    ta = rv.begin_packed_raw(_packed31(rv, rrs[:1], True, "all", (truth[:toff[1]], toff[:2])))
    tb = rv.begin_packed_raw(_packed31(rv, rrs[1:], False, "alone", (truth[toff[1]:], toff[1:] - toff[1])))
    ga, gb = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
    _same(np.concatenate([ga[11], gb[11]]), want, "the two calls are the one call's reads")
    # one read without a truth
    got = rv.run_packed_raw(_packed31(rv, rrs, False, "alone", (truth[toff[1]:], np.array([0, 0, toff[2] - toff[1]], np.int64))))
    _same(got[11], np.stack([np.zeros(6, np.uint64), want[1]]), "no truth for the first read")
    # no window at all (N <= T): filled on the host
    r0 = rrs[0]
    p = rv.pack_reads_raw([r0.raw, r0.raw], [r0.starts[:rv.T - 3], r0.starts[:3]], [r0.feat_ev[:rv.T - 3], r0.feat_ev[:3]], [r0.shift] * 2, [r0.scale] * 2, rv.T)
    b = np.concatenate([np.asarray(r0.bases, "S1")[:rv.T - 3], np.asarray(r0.bases, "S1")[:3]]).view(np.uint8)
    t2, o2 = np.frombuffer(b"ACGTACGTAC", np.uint8), np.array([0, 10, 10], np.int64)
    got = rv.run_packed_raw(rv.with_device_error_classes(rv.with_device_accuracy(rv.with_device_merge(p, b, True), t2, o2)))
    _same(got[11], hs.read_error_classes(b, [rv.T - 3, 3], got[0], got[2], t2, o2), "no window")
    assert got[11][0, 1] == got[11][0, 3] > 0 and got[11][0, 2] == got[11][0, 4] and not got[11][1].any()
    return out


def test_revise_reads_raw_errclass_equals_the_definition(species_models, short_reads, truth_of_short_reads, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for mode in MODES:
        rv.set_precision(mode)
        _end_to_end(rv, short_reads, *truth_of_short_reads)
        assert rv.saturated() == (0, 0), mode
    rv.close()


def test_errclass_call_refuses_a_bad_truth_by_its_name(species_models, short_reads, truth_of_short_reads, monkeypatch):
    from nanoreviser_amd.engine import NrvError
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rrs = [r for r, _ in short_reads]
    truth, toff = truth_of_short_reads
    p = _packed31(rv, rrs, True, "alone", (truth, toff))
    for k, v in ((28, None), (30, None), (28, toff + 1), (28, toff[::-1].copy()), (26, np.zeros((2, 2), np.int64))):   # ... and a trim without trim_thr
        with pytest.raises(NrvError, match="nrv_revise_reads_raw_errclass_begin"):
            rv.run_packed_raw(p[:k] + (v,) + p[k + 1:])
    _same(rv.run_packed_raw(p)[11], _definition(rv, rrs, truth, toff), "the handle is usable after a refusal")
    rv.close()


def test_range_guard_rerun_gives_the_f32_classes(species_models, short_reads, monkeypatch):
    """The spiked read of tests/test_gpu_device_accuracy.py behind a clean one: nrv_reads_raw_end runs the whole call again on the
    f32 kernels; the kernel runs again on the re-merged reads and stores every word again - the "out" columns are the f32
    mode's, the "in" columns what they were."""
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
    bases = np.concatenate([np.asarray(other.bases, "S1"), np.asarray(rr.bases, "S1")[:N]]).view(np.uint8)
    args = ([other.raw, raw], [other.starts, starts], [other.feat_ev, feat], [other.shift, sh], [other.scale, sc])
    el = [len(other.starts), N]
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rv.set_precision("f32")
    _, _, a1, a2 = rv.predict_reads_raw(*args)
    seq, _, off = hs.emit_calls(bases, el, a1, a2, None, T)
    truth, toff = truth_for_reads(np.random.default_rng(12), seq, off, 0.05)
    want = hs.read_error_classes(bases, el, seq, off, truth, toff)
    assert rv.saturated()[1] == 0 and (want[:, 3] > 0).all() and (want[:, 1] != want[:, 3]).all()
    rv.set_precision("f16x2")
    r0 = rv.saturated()[1]
    p = rv.with_device_report(rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, True))
    got = rv.run_packed_raw(rv.with_device_error_classes(rv.with_device_accuracy(p, truth, toff)))
    assert rv.saturated()[1] - r0 == 1
    _same(got[11], want, "re-run")
    assert np.array_equal(got[11][:, [0, 1, 3]], got[10][:, :3])
    rv.close()


def test_poisoned_workspace_gives_the_same_classes(species_models, short_reads, truth_of_short_reads, planted, monkeypatch):
    clean = _engine(monkeypatch, *species_models["ecoli"])
    ref = _end_to_end(clean, short_reads, *truth_of_short_reads)
    clean.close()
    names, truths, rds, want = planted
    S = 64 * strip()
    carry = [k for k, t in enumerate(truths) if len(t) > S]              # more than one stripe: they read the carry words
    assert len(carry) >= 10
    c = profile_case()
    truth, toff, _ = _truths_for_case(c, T, 100 + T)
    seq_w, _, off_w = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], None, T)
    want_c = hs.read_error_classes(c["bases"], c["ev_len"], seq_w, off_w, truth, toff)
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
        for p in range(2):
            got = _end_to_end(rv, short_reads, *truth_of_short_reads)
            assert [k for k, _ in got] == [k for k, _ in ref]
            for (k, x), (_, y) in zip(ref, got):
                _same(y, x, (poison, p, k))
            d, M = rv.edit_classes_device([truths[k] for k in carry], [rds[k] for k in carry])
            _same(np.stack([d, M], 1), want[carry], (poison, p, "carry"))
            _same(rv.merge_calls_errclass_device(c["bases"], c["ev_len"], c["a1"], c["a2"], truth, toff)[3], want_c, (poison, p, "merge"))
        assert rv.saturated() == (0, 0), poison
        rv.close()


# ---- 7. command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_error_classes_are_the_same_on_the_device_route(tmp_path, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_SUMMARY",
              "NRV_TRIM_Q", "NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                               # two reads per device call: several calls in flight
    d = tmp_path / "in"
    d.mkdir()
    src = sorted(glob.glob(os.path.join(FAST5, "*.fast5")) + glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))
    n = 4
    for i in range(n):
        shutil.copy(src[i % len(src)], d / f"s{i:02d}.fast5")
    forms = []
    real = Reviser.begin_packed_raw
    monkeypatch.setattr(Reviser, "begin_packed_raw", lambda self, packed: forms.append(len(packed)) or real(self, packed))
    fa = str(tmp_path / "truth.fa")
    outs, ecls, accs = {}, {}, {}
    for tag, extra, form in (("plain", [], 7), ("host", ["truth"], 7), ("device", ["--device_merge", "truth"], 31),
                             ("trim", ["--device_merge", "--trim_q", "3", "truth"], 31)):
        del forms[:]
        out = str(tmp_path / tag) + "/"
        argv = ["-d", str(d), "-o", out, "-S", "ecoli", "--gpus", "1", "--thread", "4"]
        argv += [x for e in extra for x in (["--truth", fa, "--accuracy", str(tmp_path / (tag + ".acc")),
                                             "--error_classes", str(tmp_path / (tag + ".ecl"))] if e == "truth" else [e])]
        assert cli.main(argv) == 0
        outs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        assert outs[tag]["failed_reads.txt"] == b"" and forms and set(forms) == {form}, (tag, forms)
        assert not glob.glob(str(tmp_path / "*.part*")) and not glob.glob(out + "*.part*")
        if "truth" in extra:
            ecls[tag], accs[tag] = (open(str(tmp_path / (tag + e)), "rb").read() for e in (".ecl", ".acc"))
        if tag == "plain":                                                  # the truth: a seeded 5 % mutation of what the plain run wrote
            rng = np.random.default_rng(8)
            with open(fa, "w") as fp:
                for i in range(n):
                    if i != 2:                                              # one read left out
                        t = mutate(rng, outs[tag][f"s{i:02d}_out.fasta"].split(b"\n")[1], 0.05).decode()
                        fp.write(f">s{i:02d}{'.fast5' if i % 2 else ''}\n" + "".join(t[k:k + 70] + "\n" for k in range(0, len(t), 70)))
    assert ecls["device"] == ecls["host"] == ecls["trim"] and accs["device"] == accs["host"] == accs["trim"]
    assert outs["host"] == outs["device"] == outs["plain"] and len(outs["plain"]) == n + 1
    lines = [ln.split("\t") for ln in ecls["host"].decode().split("\n")]
    acc = [ln.split("\t") for ln in accs["host"].decode().split("\n")]
    assert lines[0] == cli.ERRCLASS_HEADER.split("\t") and lines[-2] == ["#reads", str(n - 1), "1", "0"] and lines[-3][:2] == ["#total", "with_truth"]
    for i, (c, a) in enumerate(zip(lines[1:n + 1], acc[1:n + 1])):
        assert c[0] == f"s{i:02d}.fast5" and c[1] == "revised"
        if i == 2:
            assert c[2:] == ["0"] + ["."] * 10
            continue
        m, (n_in, M_in, S_in, I_in, D_in), (n_out, M_out, S_out, I_out, D_out) = int(c[2]), map(int, c[3:8]), map(int, c[8:13])
        # the identities, and the --accuracy file's distances and lengths
        assert M_in + S_in + I_in == n_in and M_in + S_in + D_in == m and M_out + S_out + I_out == n_out and M_out + S_out + D_out == m
        assert [str(m), str(n_in), str(S_in + I_in + D_in), str(n_out), str(S_out + I_out + D_out)] == a[2:7]
        assert min(S_in, I_in, D_in, S_out, I_out, D_out) >= 0 and 0 < S_out + I_out + D_out < S_in + I_in + D_in
    tot = [int(x) for x in lines[-3][2:13]]
    assert tot == [sum(int(c[k]) for c in lines[1:n + 1] if c[3] != ".") for k in range(2, 13)]
    assert lines[-3][13:] == [f"{tot[k] / tot[0]:.6f}" for k in (3, 4, 5, 8, 9, 10)]
