"""--score on the CPU: hoststage.nll16 / score_calls / score_labels_from_text are the DEFINITION of what score_kernel computes on
the device (csrc/nrv_score.h).  They are held to `score_cases.loop_score`, the rule text of include/nanorev.h restated per read
and per window in plain Python, bit for bit; the integer logarithm to float64 log2; the label bytes read back from the text of a
labels file to `align_labels`' own."""
import numpy as np
import pytest

import labels_cases
import report_cases
import score_cases
from nanoreviser_amd import cli, engine
from nanoreviser_amd import hoststage as hs

WINDOWS = (1, 2, 12, 13, 32)


def _definition(c, T, rows=True):
    return hs.score_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"] if rows else None, c["p2"] if rows else None,
                          c["labels"], c["score_thr"], T)


def test_constants_and_forms():
    assert hs.SCORE_COLS == engine.SCORE_COLS == 248
    assert set(engine._RAW_FORMS_SCORE) == {36} and 36 not in engine._RAW_FORMS and 36 not in engine._RAW_FORMS_TRUTH and 36 not in engine._RAW_FORMS_INFIX
    assert {"nrv_revise_reads_raw_score_begin", "nrv_revise_reads_raw_score", "nrv_merge_calls_score"} <= set(engine.SYMBOLS)
    assert (hs.SC_CONF1, hs.SC_CONF2, hs.SC_CAL1_N, hs.SC_CAL1_OK, hs.SC_CAL2_N, hs.SC_CAL2_OK, hs.SC_NLL1, hs.SC_NLL2, hs.SC_DEC_KIND,
            hs.SC_SUB_RIGHT) == (2, 38, 63, 103, 143, 183, 223, 224, 225, 245)


def test_nll16_exact_points():
    f = lambda v: int(hs.nll16(np.array([v], np.float32))[0])
    assert f(0.5) == 65536 and f(1.0) == 0 and f(0.0) == f(np.nan) == 8323072 == 127 << 16
    assert f(np.inf) == f(-np.inf) == f(-0.0) == f(-0.5) == f(1e-40) == 8323072      # Inf, negatives, a denormal
    assert f(2.0) == f(1.5) == 0 and f(0.25) == 2 * 65536 and f(2.0 ** -126) == 126 * 65536
    assert f(np.nextafter(np.float32(1), np.float32(0))) in (0, 1)                  # -log2(1 - 2^-24) = 8.6e-8 bit: below one unit
    vals = np.array([0.5, 1.0, 0.0, np.nan, 1e-40, 0.3, 0.999, 2.0 ** -126, 7e-30], np.float32)
    assert hs.nll16(vals).dtype == np.uint64
    assert [int(x) for x in hs.nll16(vals)] == [score_cases.loop_nll16(int(b)) for b in vals.view(np.uint32)]


def test_nll16_against_float64_log2():
    """|nll16 / 65536 + log2 p| <= 2^-15 on seeded f32 values of [2^-126, 1): the truncation to sixteen bits (2^-16) plus the
    error of the sixteen truncated squarings.  Uniform bit patterns (log-uniform values) and uniform values near 1."""
    rng = np.random.default_rng(511)
    bits = rng.integers(0x00800000, 0x3F800000, 200000, dtype=np.int64).astype(np.uint32)
    near_one = (1.0 - rng.random(100000) * 0.75).astype(np.float32)
    near_one = near_one[near_one < 1]
    p = np.concatenate([bits.view(np.float32), near_one, np.array([2.0 ** -126, np.nextafter(np.float32(1), np.float32(0)), 0.5], np.float32)])
    assert p.size >= 100000 and p.min() >= np.float32(2.0 ** -126) and p.max() < 1
    err = hs.nll16(p).astype(np.float64) / 65536 + np.log2(p.astype(np.float64))
    print(f"nll16 / 65536 + log2 p in [{err.min():.3e}, {err.max():.3e}] over {p.size} values")
    assert np.abs(err).max() <= 2.0 ** -15


@pytest.mark.parametrize("T", (report_cases.T,) + WINDOWS)
def test_score_calls_is_the_loop(T):
    c, with_rows, without = score_cases.cached_case(T=T)
    got = _definition(c, T)
    assert got.dtype == np.uint64 and got.shape == (len(c["ev_len"]), 248)
    assert np.array_equal(got, with_rows), np.argwhere(got != with_rows)[:10]
    got0 = _definition(c, T, rows=False)
    assert np.array_equal(got0, without) and not got0[:, 63:225].any()
    assert np.array_equal(got0[:, :63], got[:, :63]) and np.array_equal(got0[:, 225:], got[:, 225:])


def test_the_case_plants_what_it_says():
    c, ref, _ = score_cases.cached_case()
    lab, el = c["labels"], c["ev_len"]
    assert set(score_cases.VALID) <= set(lab.tolist()) and len(score_cases.VALID) == 20
    assert ref[9, 0] == el[9] - 11 and ref[9, 1] == 0 and not ref[9, 2:].any()       # the unlabelled read: windows, nothing else
    assert (ref[:, 1] < ref[:, 0])[[8, 10, 11, 13]].all()                              # clips reach into the windows
    assert (ref[:, 225:245].sum(0) > 0).sum() >= 18                                    # nearly every decision x kind occurs
    assert ref[13, 63] > 0 and ref[13, 63 + 39] > 0 and ref[13, 143] > 0               # bin 0 (0, NaN, negatives) and bin 39 (1.0, Inf)
    assert ref[:, 245].sum() > 0 and not ref[:, 246:].any()
    never = set(score_cases.NEVER)
    assert all((b & 7) in (0, 6, 7) for b in never) and all(1 <= (b & 7) <= 5 and b != 0xFF for b in score_cases.HIGH_BITS)


@pytest.mark.parametrize("T", (report_cases.T, 1, 32))
def test_identities(T):
    c, _, _ = score_cases.cached_case(T=T)
    sc = _definition(c, T).astype(np.int64)
    labelled = sc[:, 1]
    assert (labelled <= sc[:, 0]).all() and np.array_equal(sc[:, 0], np.maximum(c["ev_len"] - T, 0))
    for lo, hi in ((2, 38), (38, 63), (63, 103), (143, 183), (225, 245)):
        assert np.array_equal(sc[:, lo:hi].sum(1), labelled), (lo, hi)
    assert np.array_equal(sc[:, 103:143].sum(1), sc[:, 2:38].reshape(-1, 6, 6).trace(axis1=1, axis2=2))
    assert np.array_equal(sc[:, 183:223].sum(1), sc[:, 38:63].reshape(-1, 5, 5).trace(axis1=1, axis2=2))
    assert (sc[:, 103:143] <= sc[:, 63:103]).all() and (sc[:, 183:223] <= sc[:, 143:183]).all()
    assert (sc[:, 245] <= sc[:, 229:233].sum(1)).all()
    # every window labelled: the decision sums are the report's columns 4 .. 8
    full = np.array(score_cases.VALID, np.uint8)[np.arange(c["N"]) % 20]
    sc = hs.score_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], full, c["score_thr"], T).astype(np.int64)
    rep = hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], None, T).astype(np.int64)
    assert np.array_equal(sc[:, 1], sc[:, 0]) and np.array_equal(sc[:, 0], rep[:, 1])
    assert np.array_equal(sc[:, 225:245].reshape(-1, 5, 4).sum(2), rep[:, 4:9])
    assert np.array_equal(sc[:, 2:38].reshape(-1, 6, 6).sum(1), rep[:, 9:15]) and np.array_equal(sc[:, 38:63].reshape(-1, 5, 5).sum(1), rep[:, 15:20])


def test_score_calls_refuses_what_does_not_fit():
    c, _, _ = score_cases.cached_case()
    with pytest.raises(ValueError):
        hs.score_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], None, None, c["labels"][:-1], c["score_thr"], 11)
    with pytest.raises(ValueError):
        hs.score_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], None, None, c["labels"], c["score_thr"][:-1], 11)


def test_labels_come_back_from_their_text():
    cases, defs = labels_cases.planted_cases(), labels_cases.definition()
    seen = compared = 0
    for name, (t, s, rev, st, en) in cases.items():
        lab, summ, _ = defs[name]
        if len(t) == 0:
            continue
        lab = np.frombuffer(lab, np.uint8)
        mp, l1, l2 = hs.label_strings(lab)
        head = "\t".join(["#" + name.replace("\t", " "), "-" if rev else "+", str(st), str(en), str(len(s))] + [str(x) for x in summ])
        got = hs.score_labels_from_text(head + "\n", bytes(s).decode("ascii", "replace"), mp, l1, l2)
        assert got.dtype == np.uint8 and got.size == len(s), name
        n, cs, ce = len(s), summ[4], summ[5]
        keep = np.ones(n, bool)
        keep[:cs] = False
        keep[n - ce:] = False
        keep &= (lab & 7) != 0
        assert np.array_equal(got[keep], lab[keep]), name
        assert (got[~keep] == 0xFF).all(), name
        seen, compared = seen + 1, compared + int(keep.sum())
    assert seen > 100 and compared > 10000
    with pytest.raises(ValueError):
        hs.score_labels_from_text("#r\t+\t0\t4\t4\t4\t0\t0\t0\t0\t0\t0", "ACGT", "MMM", "555", "555")
    with pytest.raises(ValueError):
        hs.score_labels_from_text("#r\t+\t0\t4", "ACGT", "MMMM", "5432", "5432")
    assert hs.score_labels_from_text("#r\t+\t0\t4\t4\t2\t1\t1\t0\t1\t0\t0", "AATT", "IMXD", "1540", "1543").tolist() == [0xFF, 5, 4 | 8, 3 | 16]


def test_with_device_score_pads_every_form():
    from nanoreviser_amd.engine import Reviser
    rng = np.random.default_rng(5)
    el = [40, 30]
    raws = [rng.integers(200, 900, 20 * n).astype(np.int16) for n in el]
    starts = [np.arange(n, dtype=np.int32) * 20 for n in el]
    feats = [rng.random((n, 6)).astype(np.float32) for n in el]
    packed = Reviser.pack_reads_raw(raws, starts, feats, [1.0, 2.0], [3.0, 4.0], 11)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 70)]
    labels = np.full(70, 0xFF, np.uint8)
    m12 = Reviser.with_device_merge(packed, bases, True)
    forms = [m12, Reviser.with_device_report(m12), Reviser.with_device_edits(m12), Reviser.with_device_profile(m12),
             Reviser.with_device_trim(m12, 7), Reviser.with_device_accuracy(m12, b"ACGT" * 4, [0, 8, 16])]
    forms.append(Reviser.with_device_infix(forms[-1]))
    for p in forms:
        s = Reviser.with_device_score(p, labels)
        assert len(s) == 36 and s[:len(p)] == tuple(p)
        assert s[33].dtype == np.uint8 and s[33].size == 70 and s[34].dtype == np.float32 and s[34].size == 39
        assert s[35].shape == (2, 248) and s[35].dtype == np.uint64 and np.array_equal(s[34], cli.phred_thresholds())
    s = Reviser.with_device_score(m12, labels, np.linspace(0.1, 0.9, 39))
    assert s[12:33] == (0.0, None, None, None, None, None, None, None, None, None, None, 0, 0, 0, None, None, None, None, None, 2, None)
    assert np.array_equal(s[34], np.linspace(0.1, 0.9, 39).astype(np.float32))
    for bad in (lambda: Reviser.with_device_score(packed, labels), lambda: Reviser.with_device_score(m12, labels[:-1]),
                lambda: Reviser.with_device_score(m12, labels, np.zeros(38))):
        with pytest.raises(ValueError):
            bad()


def test_score_flag_parsing(monkeypatch, capsys):
    for k in ("NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES", "NRV_INFIX", "NRV_LABELS", "NRV_TRIM_Q", "NRV_SCORE", "NRV_LABELS_FROM"):
        monkeypatch.delenv(k, raising=False)
    base = ["-d", "x", "-o", "y"]
    a = cli.get_args(base)
    assert a.score is None and a.labels_from is None
    a = cli.get_args(base + ["--score", "s.tsv", "--labels_from", "lab"])
    assert (a.score, a.labels_from, a.truth, a.infix) == ("s.tsv", "lab", None, None)      # neither --truth nor --infix is needed
    monkeypatch.setenv("NRV_SCORE", "env.tsv")
    monkeypatch.setenv("NRV_LABELS_FROM", "envdir")
    a = cli.get_args(base)
    assert (a.score, a.labels_from) == ("env.tsv", "envdir")
    monkeypatch.delenv("NRV_LABELS_FROM")
    with pytest.raises(SystemExit) as e:
        cli.get_args(base)
    assert e.value.code == 2 and "--score goes with --labels_from" in capsys.readouterr().err
    monkeypatch.delenv("NRV_SCORE")
    for bad, msg in ((["--score", "s.tsv"], "--score goes with --labels_from"),
                     (["--labels_from", "lab"], "--score goes with --labels_from"),
                     (["--score", "s.tsv", "--labels_from", "lab", "--truth", "t.fa", "--infix", "i.tsv", "--labels", "lab"],
                      "--labels_from cannot be the directory this run's --labels writes"),
                     (["--score", "s.tsv", "--labels_from", "./lab/", "--truth", "t.fa", "--infix", "i.tsv", "--labels", "lab"],
                      "--labels_from cannot be the directory this run's --labels writes"),
                     (["--score", "s.tsv", "--labels_from", "lab", "--resume"], "--resume cannot be used with --score")):
        with pytest.raises(SystemExit) as e:
            cli.get_args(base + bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err, bad
