"""Edit distance to a truth set on the device (MI355X only, -m gpu): csrc/nrv_align.h through nrv_edit_distance,
nrv_merge_calls_accuracy, nrv_revise_reads_raw_accuracy_begin / nrv_revise_reads_raw_accuracy and the command line's
--truth / --accuracy.

Everything is compared BIT FOR BIT - the distance is an integer and unique, nothing here has a tolerance.
hoststage.edit_distance and hoststage.read_accuracy are the definitions (tests/test_accuracy_host.py holds them to two references
that share no code with them).  The shipped E. coli weights:
  1. nrv_edit_distance on tests/accuracy_cases.py's planted pairs - truth lengths on both sides of every block (32 / 64 / 128) and
     stripe (2048 / 4096) boundary, 4160, 8193, reads shorter than the number of blocks, chunks removed and inserted, a match run
     through every block, Ns, 300 pairs of 3, empty truths first, in the middle and last - in one call, two passes over one
     handle; a truth_off that does not ascend from 0 is refused under the entry point's name and the handle stays usable;
  2. nrv_merge_calls_accuracy on profile_case and report_case(T) at T = 1, 2, 11, 32: truths are seeded mutations of the
     host-merged reads for some reads, an empty read among them; seq / qual / off are nrv_merge_calls'; N <= T on the host;
  3. nrv_revise_reads_raw_accuracy on the two shortest fixture reads in one call, in each precision mode, FASTA and FASTQ, alone
     and behind report + edits + records + profile + trim, against the definition on nrv_predict_reads_raw's outputs in that
     mode; every other output is that of the same call without the accuracy; 0 < dist_out and dist_in != dist_out;
  4. two calls in flight; 5. a call that trips the f16x2 range guard (one re-run, the f32 mode's dist_out, dist_in unchanged);
  6. handles under NRV_POISON, both patterns, two passes, the planted pairs of 4097 and 8193 (they read the carry bytes) included;
  7. the command line with --truth / --accuracy: form 30 with --device_merge, the host route's file byte for byte.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from accuracy_cases import mutate, planted_cases, truth_for_reads
from conftest import GOLD
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from profile_cases import profile_case
from report_cases import T, report_case

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "bf16x3", "f32"]
PATTERNS = {"qnan": 0x7FC00000, "m1500": 0xC4BB8000}
FAST5 = os.path.join(GOLD, "fast5")
NAMES = [b"read_0", b"the_second_read"]


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


@pytest.fixture(scope="module")
def planted():
    """(names, truths, reads, the definition's distances with -1 for an empty truth): computed once."""
    cases, _ = planted_cases()
    names = list(cases)
    truths, rds = [cases[k][0] for k in names], [cases[k][1] for k in names]
    want = np.array([hs.edit_distance(t, s) if t else -1 for t, s in zip(truths, rds)], np.int64)
    return names, truths, rds, want


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (what, bad[:8].tolist(), got[got != want][:8].tolist(), want[got != want][:8].tolist())


def _eq(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


# ---- 1. the kernel on planted pairs -------------------------------------------------------------------------------------------------
def test_edit_distance_on_planted_pairs(species_models, planted, monkeypatch):
    from nanoreviser_amd import engine as E
    names, truths, rds, want = planted
    assert (want == -1).sum() >= 3 and want[0] == -1 and want[-1] == -1 and len(want) > 400
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for p in range(2):                                                   # a second pass over the same handle: the same distances
        got = rv.edit_distance_device(truths, rds)
        bad = [(names[i], int(got[i]), int(want[i])) for i in np.flatnonzero(got != want)]
        assert not bad and got.dtype == np.int64, (p, bad[:8])
    # one pair at a time: a grid of one wave
    for k in (names.index("m=4097 mutated 10 %*"), names.index("m=64 3 characters"), names.index("m=1 empty*")):
        assert rv.edit_distance_device(truths[k:k + 1], rds[k:k + 1]).tolist() == [int(want[k])], names[k]
    assert rv.edit_distance_device([], []).size == 0
    a = np.frombuffer(b"ACGTACGT", np.uint8)
    for bad_a, bad_b in (([1, 4, 8], [0, 4, 8]), ([0, 5, 4], [0, 4, 8]), ([0, 4, 8], [0, 9, 8]), ([0, 4, 8], [2, 4, 8])):
        with pytest.raises(E.NrvError, match="nrv_edit_distance"):      # refused under the entry point's name
            rv.edit_distance_offsets(a, bad_a, a, bad_b)
    assert rv.edit_distance_offsets(a, [0, 4, 8], a, [0, 3, 8]).tolist() == [1, 1]      # the handle is usable afterwards
    rv.close()


# ---- 2. behind the merge --------------------------------------------------------------------------------------------------------------
def _truths_for_case(c, Tw, seed):
    """Seeded mutations of the host-merged reads for about two reads in three; an empty read with a truth among them."""
    seq, _, off = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], None, Tw)
    R = len(c["ev_len"])
    rng = np.random.default_rng(seed)
    without = tuple(r for r in range(R) if r % 3 == 1)
    truth, toff = truth_for_reads(rng, seq, off, 0.1, without)
    parts = [truth[toff[r]:toff[r + 1]].tobytes() for r in range(R)]
    empty = [r for r in range(R) if c["ev_len"][r] == 0 and r not in without]
    assert empty
    parts[empty[0]] = b"ACGTTGCA"                                         # d = m for both kinds
    toff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), toff, empty[0]


def _merge_accuracy_checks(rv, c, Tw):
    truth, toff, e = _truths_for_case(c, Tw, 100 + Tw)
    thr = cli.phred_thresholds()
    ins = (c["bases"], c["ev_len"], c["a1"], c["a2"])
    seq_w, _, off_w = hs.emit_calls(*ins, None, Tw)
    want = hs.read_accuracy(c["bases"], c["ev_len"], seq_w, off_w, truth, toff)
    assert want[e].tolist() == [8, 8, 8, 0] and (want[:, 0] == 0).sum() >= 4 and (want[:, 1] != want[:, 2]).sum() >= (3 if Tw > 2 else 1)
    for q_thr in (None, thr):
        seq, qual, off, acc = rv.merge_calls_accuracy_device(*ins, truth, toff, c["p1"], c["p2"], q_thr)
        _same(acc, want, (Tw, q_thr is None))
        m = rv.merge_calls_device(*ins, c["p1"], c["p2"], q_thr)
        assert np.array_equal(seq, m[0]) and _eq(qual, m[1]) and np.array_equal(off, m[2])
    # no truth at all: zeros
    _same(rv.merge_calls_accuracy_device(*ins, b"", np.zeros(len(c["ev_len"]) + 1, np.int64))[3], np.zeros_like(want), (Tw, "no truth"))
    return want


def test_merge_calls_accuracy_equals_the_definition(species_models, monkeypatch):
    from nanoreviser_amd import engine as E
    c = profile_case()
    rv = _engine(monkeypatch, *species_models["ecoli"])
    _merge_accuracy_checks(rv, c, T)
    # no window at all (N <= T): filled on the host, dist_out = dist_in
    z = np.zeros(0, np.int8)
    b = np.frombuffer(b"ACGTANNCA", np.uint8)
    truth, toff = np.frombuffer(b"ACTTAGGNNCA", np.uint8), np.array([0, 6, 8, 11], np.int64)
    seq, qual, off, acc = rv.merge_calls_accuracy_device(b, [5, 0, 4], z, z, truth, toff)
    assert seq.tobytes() == b.tobytes() and off.tolist() == [0, 5, 5, 9]
    _same(acc, hs.read_accuracy(b, [5, 0, 4], seq, off, truth, toff), "no window")
    assert acc.tolist() == [[6, 2, 2, 0], [2, 2, 2, 0], [3, 2, 2, 0]]
    ins = rv._merge_inputs(c["bases"], c["ev_len"], c["a1"], c["a2"], None, None, None, False)
    R = len(c["ev_len"])
    for bad in (np.arange(1, R + 2), np.arange(R, -1, -1)):              # the C entry point refuses them under its own name
        more = E._marshal((np.zeros(R + 2, np.uint8), bad.astype(np.int64), np.zeros((R, 4), np.uint64)), E._TRUTH[0])
        with pytest.raises(E.NrvError, match="nrv_merge_calls_accuracy"):
            rv._merge_call("nrv_merge_calls_accuracy", *ins, *more)
    rv.close()


@pytest.mark.parametrize("Tw", [1, 2, 32])
def test_merge_calls_accuracy_at_other_window_lengths(species_models, monkeypatch, Tw):
    rv = _engine(monkeypatch, *species_models["ecoli"], Tw=Tw)
    _merge_accuracy_checks(rv, report_case(T=Tw), Tw)
    rv.close()


# ---- 3 - 6. end to end ----------------------------------------------------------------------------------------------------------------
def _bases(rrs):
    return np.concatenate([np.asarray(r.bases, "S1") for r in rrs]).view(np.uint8)


def _calls(rv, rrs):
    return rv.predict_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs],
                                [r.shift for r in rrs], [r.scale for r in rrs])


def _merged(rv, rrs):
    """The host-merged reads of nrv_predict_reads_raw's calls in the engine's mode: (seq, off)."""
    _, _, a1, a2 = _calls(rv, rrs)
    seq, _, off = hs.emit_calls(_bases(rrs), [len(r.starts) for r in rrs], a1, a2, None, rv.T)
    return seq, off


@pytest.fixture(scope="module")
def truth_of_short_reads(species_models, short_reads):
    """A 5 % mutation of the host-merged form (default mode) of the two reads: (truth, truth_off)."""
    from nanoreviser_amd.engine import Reviser
    rv = Reviser(*species_models["ecoli"])
    seq, off = _merged(rv, [r for r, _ in short_reads])
    rv.close()
    return truth_for_reads(np.random.default_rng(41), seq, off, 0.05)


def _definition(rv, rrs, truth, toff):
    seq, off = _merged(rv, rrs)
    return hs.read_accuracy(_bases(rrs), [len(r.starts) for r in rrs], seq, off, truth, toff)


def _packed(rv, rrs, fastq, inner="alone", truth=None):
    p = rv.pack_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs], [r.shift for r in rrs], [r.scale for r in rrs], rv.T)
    p = rv.with_device_merge(p, _bases(rrs), fastq)
    if inner == "all":                                                   # report + edits + records + profile + trim
        p = rv.with_device_trim(rv.with_device_profile(rv.with_device_records(rv.with_device_edits(rv.with_device_report(p)), NAMES[:len(rrs)])), 3, 4, 1)
    return p if truth is None else rv.with_device_accuracy(p, *truth)


def _check_call(got, plain, want, what):
    """A form-30 result: the accuracy last, every other output that of the same call without it (None where it carries none)."""
    assert len(got) == 11 and len(plain) in (3, 10), what
    _same(got[10], want, what)
    for k, (g, p) in enumerate(zip(got, plain)):
        assert _eq(g, p), (what, k)
    assert all(g is None for g in got[len(plain):10]), what


def _end_to_end(rv, short_reads, truth, toff):
    """Every end-to-end form on the two reads -> [(name, accuracy)]; compared with the definition inside."""
    out = []
    rrs = [r for r, _ in short_reads]
    want = _definition(rv, rrs, truth, toff)
    # a vacuous pass is a failure: the revision moved both reads, and neither onto its truth
    assert (want[:, 0] == np.diff(toff)).all() and (want[:, 2] > 0).all() and (want[:, 1] != want[:, 2]).all(), want.tolist()
    for fastq in (False, True):
        for inner in ("alone", "all"):
            got = rv.run_packed_raw(_packed(rv, rrs, fastq, inner, (truth, toff)))
            plain = rv.run_packed_raw(_packed(rv, rrs, fastq, inner))
            _check_call(got, plain, want, ("one call", fastq, inner))
            out.append((f"one call {fastq} {inner}", got[10].copy()))
        # two calls in flight, one read each
        ta = rv.begin_packed_raw(_packed(rv, rrs[:1], fastq, "all", (truth[:toff[1]], toff[:2])))
        tb = rv.begin_packed_raw(_packed(rv, rrs[1:], fastq, "alone", (truth[toff[1]:], toff[1:] - toff[1])))
        ga, gb = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
        _same(np.concatenate([ga[10], gb[10]]), want, ("the two calls are the one call's reads", fastq))
        # one read without a truth, and none at all
        got = rv.run_packed_raw(_packed(rv, rrs, fastq, "alone", (truth[toff[1]:], np.array([0, 0, toff[2] - toff[1]], np.int64))))
        _same(got[10], np.stack([np.zeros(4, np.uint64), want[1]]), ("no truth for the first read", fastq))
        # no window at all (N <= T): filled on the host
        r0 = rrs[0]
        p = rv.pack_reads_raw([r0.raw, r0.raw], [r0.starts[:rv.T - 3], r0.starts[:3]], [r0.feat_ev[:rv.T - 3], r0.feat_ev[:3]], [r0.shift] * 2, [r0.scale] * 2, rv.T)
        b = np.concatenate([np.asarray(r0.bases, "S1")[:rv.T - 3], np.asarray(r0.bases, "S1")[:3]]).view(np.uint8)
        t2, o2 = np.frombuffer(b"ACGTACGTAC", np.uint8), np.array([0, 10, 10], np.int64)
        got = rv.run_packed_raw(rv.with_device_accuracy(rv.with_device_merge(p, b, fastq), t2, o2))
        _same(got[10], hs.read_accuracy(b, [rv.T - 3, 3], got[0], got[2], t2, o2), ("no window", fastq))
        assert got[10][0, 1] == got[10][0, 2] > 0 and not got[10][1].any()
    return out


def test_revise_reads_raw_accuracy_equals_the_definition(species_models, short_reads, truth_of_short_reads, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for mode in MODES:
        rv.set_precision(mode)
        _end_to_end(rv, short_reads, *truth_of_short_reads)
        assert rv.saturated() == (0, 0), mode
    rv.close()


def test_accuracy_call_refuses_a_bad_truth_by_its_name(species_models, short_reads, truth_of_short_reads, monkeypatch):
    from nanoreviser_amd.engine import NrvError
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rrs = [r for r, _ in short_reads]
    truth, toff = truth_of_short_reads
    p = _packed(rv, rrs, True, "alone", (truth, toff))
    for k, v in ((28, None), (29, None), (28, toff + 1), (28, toff[::-1].copy()), (26, np.zeros((2, 2), np.int64))):   # ... and a trim without trim_thr
        with pytest.raises(NrvError, match="nrv_revise_reads_raw_accuracy_begin"):
            rv.run_packed_raw(p[:k] + (v,) + p[k + 1:])
    _same(rv.run_packed_raw(p)[10], _definition(rv, rrs, truth, toff), "the handle is usable after a refusal")
    rv.close()


def test_range_guard_rerun_gives_the_f32_distance(species_models, short_reads, monkeypatch):
    """The spiked read of tests/test_gpu_device_trim.py behind a clean one: nrv_reads_raw_end runs the whole call again on the f32
    kernels; the alignment runs again on the re-merged reads and stores every word again - dist_out is the f32 mode's, dist_in
    is what it was."""
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
    want = hs.read_accuracy(bases, el, seq, off, truth, toff)
    assert rv.saturated()[1] == 0 and (want[:, 2] > 0).all() and (want[:, 1] != want[:, 2]).all()
    rv.set_precision("f16x2")
    for fq in (False, True):
        r0 = rv.saturated()[1]
        p = rv.with_device_report(rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, fq))
        got = rv.run_packed_raw(rv.with_device_accuracy(p, truth, toff))
        assert rv.saturated()[1] - r0 == 1, fq
        _same(got[10], want, ("re-run", fq))
        assert np.array_equal(got[3][:, 2].astype(np.int64), np.diff(got[2]))                 # the report of the same pass
    rv.close()


def test_poisoned_workspace_gives_the_same_distances(species_models, short_reads, truth_of_short_reads, planted, monkeypatch):
    clean = _engine(monkeypatch, *species_models["ecoli"])
    ref = _end_to_end(clean, short_reads, *truth_of_short_reads)
    clean.close()
    names, truths, rds, want = planted
    carry = [k for k, n in enumerate(names) if n.startswith(("m=4097", "m=8193", "m=4160"))]    # more than one stripe: they read the carry bytes
    assert len(carry) >= 10
    c = profile_case()
    truth, toff, _ = _truths_for_case(c, T, 100 + T)
    seq_w, _, off_w = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], None, T)
    want_c = hs.read_accuracy(c["bases"], c["ev_len"], seq_w, off_w, truth, toff)
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
        for p in range(2):
            got = _end_to_end(rv, short_reads, *truth_of_short_reads)
            assert [k for k, _ in got] == [k for k, _ in ref]
            for (k, x), (_, y) in zip(ref, got):
                _same(y, x, (poison, p, k))
            _same(rv.edit_distance_device([truths[k] for k in carry], [rds[k] for k in carry]), want[carry], (poison, p, "carry"))
            _same(rv.merge_calls_accuracy_device(c["bases"], c["ev_len"], c["a1"], c["a2"], truth, toff)[3], want_c, (poison, p, "merge"))
        assert rv.saturated() == (0, 0), poison
        rv.close()


# ---- 7. command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_accuracy_is_the_same_on_the_device_route(tmp_path, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_SUMMARY",
              "NRV_TRIM_Q", "NRV_TRUTH", "NRV_ACCURACY"):
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
    fa = str(tmp_path / "truth.fa")
    outs, accs = {}, {}
    for tag, extra, form in (("plain", [], 7), ("host", ["truth"], 7), ("device", ["--device_merge", "truth"], 30),
                             ("trim_plain", ["--device_merge", "--trim_q", "3"], 27), ("trim", ["--device_merge", "--trim_q", "3", "truth"], 30)):
        del forms[:]
        out = str(tmp_path / tag) + "/"
        argv = ["-d", str(d), "-o", out, "-S", "ecoli", "--gpus", "1", "--thread", "4"]
        argv += [x for e in extra for x in (["--truth", fa, "--accuracy", str(tmp_path / (tag + ".tsv"))] if e == "truth" else [e])]
        assert cli.main(argv) == 0
        outs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        assert outs[tag]["failed_reads.txt"] == b"" and forms and set(forms) == {form}, (tag, forms)
        assert not glob.glob(str(tmp_path / "*.part*")) and not glob.glob(out + "*.part*")
        if "truth" in extra:
            accs[tag] = open(str(tmp_path / (tag + ".tsv")), "rb").read()
        if tag == "plain":                                                  # the truth: a seeded 5 % mutation of what the plain run wrote
            rng = np.random.default_rng(8)
            with open(fa, "w") as fp:
                for i in range(10):
                    if i not in (3, 8):                                     # two reads left out
                        t = mutate(rng, outs[tag][f"s{i:02d}_out.fasta"].split(b"\n")[1], 0.05).decode()
                        fp.write(f">s{i:02d}{'.fast5' if i % 2 else ''}\n" + "".join(t[k:k + 70] + "\n" for k in range(0, len(t), 70)))
    assert accs["device"] == accs["host"] == accs["trim"]
    assert outs["host"] == outs["device"] == outs["plain"] and outs["trim"] == outs["trim_plain"] and len(outs["plain"]) == 11
    lines = [ln.split("\t") for ln in accs["host"].decode().split("\n")]
    assert lines[0] == cli.ACCURACY_HEADER.split("\t") and lines[-2] == ["#reads", "8", "2", "0"] and lines[-3][:2] == ["#total", "with_truth"]
    for i, c in enumerate(lines[1:11]):
        assert c[0] == f"s{i:02d}.fast5" and c[1] == "revised"
        if i in (3, 8):
            assert c[2:] == ["0"] + ["."] * 6
        else:                                                               # the truth lies near the revised read, further from the original
            assert 0 < int(c[6]) < int(c[4]) and int(c[5]) == len(outs["plain"][f"s{i:02d}_out.fasta"].split(b"\n")[1])
            assert c[7] == cli.identity_field(int(c[4]), max(int(c[3]), int(c[2]))) and c[8] == cli.identity_field(int(c[6]), max(int(c[5]), int(c[2])))
    assert [int(x) for x in lines[-3][2:7]] == [sum(int(c[k]) for c in lines[1:11] if c[3] != ".") for k in range(2, 7)]
