"""Truth regions: infix alignment on both strands on the device (MI355X only, -m gpu): csrc/nrv_infix.h through nrv_infix_classes,
nrv_merge_calls_infix, nrv_revise_reads_raw_infix_begin / nrv_revise_reads_raw_infix and the command line's --infix.

Everything is compared BIT FOR BIT - (d, M, start, end) is a unique tuple of integers, nothing here has a tolerance.
hoststage.infix_classes and hoststage.read_infix are the definitions (tests/test_infix_host.py holds them to three references that
share no code with them); the planted pairs are compared with those references directly.  The shipped E. coli weights:
  1. nrv_infix_classes on tests/infix_cases.py's planted pairs, both strands - region lengths on both sides of a lane's strip and
     of a stripe, up to three stripes and a character, reads cut out of the region with their ends on both sides of the strip and
     stripe boundaries, from stripe 0 into stripe 1, ending in stripe 0 of three and ending exactly at m, the same
     reverse-complemented and mutated, Ns, a read that occurs twice, AC / CA and 800 pairs of 3 to 6 characters, reads on both
     sides of lane 0's feed chunks, empty regions first, in the middle and last - one call per strand, two passes over one
     handle; single-pair grids of one stripe, two stripes and n = 0; offsets that do not ascend from 0, reverse = 2 and a region
     above the limit are refused under the entry point's name and the handle stays usable;
  2. nrv_merge_calls_infix on profile_case and report_case(T) at T = 1, 2, 11, 32, with one strand and with both; N <= T on the
     host;
  3. nrv_revise_reads_raw_infix on the two shortest fixture reads in one call, in each precision mode, alone and behind every
     other block, against the definition on nrv_predict_reads_raw's outputs in that mode; the regions are the seeded 5 % mutation
     of the merged reads between random flanks of 64 characters and more, the second one reverse-complemented; every other
     output is that of the form 31 call; two calls in flight; one read without truth;
  4. a bad truth_off, strands outside {1, 2} and a region above the limit are refused by name; 5. a call that trips the f16x2
     range guard (one re-run, the f32 mode's block);
  6. handles under NRV_POISON, both patterns, two passes, the planted pairs of more than one stripe (they read the carry words)
     included; 7. the command line: form 33 with --device_merge, with and without --trim_q, the host route's file byte for byte;
     --infix_strand forward.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from accuracy_cases import mutate, random_seq, truth_for_reads
from conftest import GOLD
from infix_cases import by_strand, revcomp, strip
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from profile_cases import profile_case
from report_cases import T, report_case
from test_gpu_device_accuracy import (FAST5, PATTERNS, _bases, _engine, _eq, _merged, _packed, _same,  # noqa: F401
                                      short_reads, truth_of_short_reads)

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "bf16x3", "f32"]
_TABLE = {}


def _infix(t, s, rev=False):
    """hoststage.infix_classes behind a table: the modes and the passes below ask for the same few long pairs again and again."""
    key = (bytes(hs._as_u8(t)), bytes(hs._as_u8(s)), bool(rev))
    if key not in _TABLE:
        _TABLE[key] = _REAL(t, s, rev)
    return _TABLE[key]


_REAL = hs.infix_classes


@pytest.fixture(autouse=True)
def _memoised(monkeypatch):
    monkeypatch.setattr(hs, "infix_classes", _infix)


@pytest.fixture(scope="module")
def planted():
    """{reverse: (names, regions, reads, the references' tuples as int64[n][4], -1 in all four for an empty region)}: computed once."""
    return by_strand()


def _classes(rv, regions, rds, rev):
    return np.stack(rv.infix_classes_device(regions, rds, reverse=rev), 1)


# ---- 1. the kernel on planted pairs -------------------------------------------------------------------------------------------------
def test_infix_classes_on_planted_pairs(species_models, planted, monkeypatch):
    from nanoreviser_amd import engine as E
    S = 64 * strip()
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for rev in (0, 1):
        names, regions, rds, want = planted[rev]
        assert (want[:, 0] == -1).sum() >= 3 and want[0, 0] == -1 and want[-1, 0] == -1 and len(want) > 600
        for p in range(2):                                               # a second pass over the same handle: the same pairs
            got = _classes(rv, regions, rds, rev)
            bad = [(names[i], got[i].tolist(), want[i].tolist()) for i in np.flatnonzero((got != want).any(1))]
            assert not bad and got.dtype == np.int64, (rev, p, bad[:8])
    names, regions, rds, want = planted[0]
    assert want[names.index("AC / CA")].tolist() == [1, 1, 1, 2]
    assert want[names.index(f"m={3 * S + 1} cut 100:140 +")].tolist() == [0, 40, 100, 140]
    # one pair at a time: a grid of one wave - one stripe, two stripes, n = 0
    for k in (names.index("m=65 cut 1:64 +"), names.index(f"m={S + 1} cut {S - 20}:{S + 1} +"), names.index(f"m={3 * S + 1} cut 100:140 +"),
              names.index("m=64 empty read +"), names.index(f"m={2 * S + 1} empty read +")):
        got = _classes(rv, regions[k:k + 1], rds[k:k + 1], 0)
        assert got.tolist() == [want[k].tolist()], names[k]
    names1, regions1, rds1, want1 = planted[1]
    k = names1.index(f"m={2 * S + 1} cut {S - 20}:{S + 20} -")
    assert _classes(rv, regions1[k:k + 1], rds1[k:k + 1], 1).tolist() == [[0, 40, S + 1 - 20, S + 1 + 20]]
    assert rv.infix_classes_device([], [])[0].size == 0
    a = np.frombuffer(b"ACGTACGT", np.uint8)
    for bad_a, bad_b in (([1, 4, 8], [0, 4, 8]), ([0, 5, 4], [0, 4, 8]), ([0, 4, 8], [0, 9, 8]), ([0, 4, 8], [2, 4, 8])):
        with pytest.raises(E.NrvError, match="nrv_infix_classes"):      # refused under the entry point's name
            rv.infix_classes_offsets(a, bad_a, a, bad_b)
    with pytest.raises(E.NrvError, match="nrv_infix_classes: reverse"):
        rv.infix_classes_offsets(a, [0, 4, 8], a, [0, 4, 8], reverse=2)
    big = np.full(E.INFIX_MAX_LEN + 1, ord("A"), np.uint8)
    with pytest.raises(E.NrvError, match="nrv_infix_classes.*NRV_INFIX_MAX_LEN"):
        rv.infix_classes_offsets(big, [0, big.size], a, [0, 8])
    with pytest.raises(E.NrvError, match="nrv_infix_classes.*NRV_INFIX_MAX_LEN"):
        rv.infix_classes_offsets(a, [0, 8], big, [0, big.size])
    got = rv.infix_classes_offsets(a, [0, 4, 8], a, [0, 3, 8])          # the handle is usable afterwards
    assert np.stack(got, 1).tolist() == [[0, 3, 0, 3], [1, 4, 0, 4]]
    rv.close()


# ---- 2. behind the merge --------------------------------------------------------------------------------------------------------------
def _regions_for_case(c, Tw, seed):
    """Truth regions of the host-merged reads for about two reads in three: a seeded 10 % mutation between random flanks, every
    other one reverse-complemented; an empty read with a region among them."""
    seq, _, off = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], None, Tw)
    R = len(c["ev_len"])
    rng = np.random.default_rng(seed)
    parts = []
    for r in range(R):
        t = random_seq(rng, 5 + r) + mutate(rng, np.asarray(seq, np.uint8)[int(off[r]):int(off[r + 1])].tobytes(), 0.1) + random_seq(rng, 9)
        parts.append(b"" if r % 3 == 1 else (revcomp(t) if r % 2 else t))
    empty = [r for r in range(R) if c["ev_len"][r] == 0 and r % 3 != 1]
    assert empty
    parts[empty[0]] = b"ACGTTGCA"
    toff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), toff, empty[0]


def _merge_infix_checks(rv, c, Tw):
    truth, toff, e = _regions_for_case(c, Tw, 200 + Tw)
    thr = cli.phred_thresholds()
    ins = (c["bases"], c["ev_len"], c["a1"], c["a2"])
    seq_w, _, off_w = hs.emit_calls(*ins, None, Tw)
    for strands in (2, 1):
        want = hs.read_infix(c["bases"], c["ev_len"], seq_w, off_w, truth, toff, strands)
        assert want[e].tolist() == [8, strands] + [0, 0, 8, 8] * strands + [0] * (4 * (2 - strands)) + [0, 0, 8, 8] * strands + [0] * (4 * (2 - strands))
        assert (want[:, 0] == 0).sum() >= 4 and (want[:, 2:6] != want[:, 10:14]).any(1).sum() >= (3 if Tw > 2 else 1)
        if strands == 2:
            assert {hs.pick_strand(w) for w in want if w[0] > 20} == {"+", "-"}
        for q_thr in (None, thr):
            seq, qual, off, blk = rv.merge_calls_infix_device(*ins, truth, toff, strands, c["p1"], c["p2"], q_thr)
            _same(blk, want, (Tw, strands, q_thr is None))
            m = rv.merge_calls_device(*ins, c["p1"], c["p2"], q_thr)
            assert np.array_equal(seq, m[0]) and _eq(qual, m[1]) and np.array_equal(off, m[2])
    _same(rv.merge_calls_infix_device(*ins, b"", np.zeros(len(c["ev_len"]) + 1, np.int64))[3], np.zeros_like(want), (Tw, "no truth"))


def test_merge_calls_infix_equals_the_definition(species_models, monkeypatch):
    from nanoreviser_amd import engine as E
    c = profile_case()
    rv = _engine(monkeypatch, *species_models["ecoli"])
    _merge_infix_checks(rv, c, T)
    # no window at all (N <= T): filled on the host, out = in
    z = np.zeros(0, np.int8)
    b = np.frombuffer(b"ACGTANNCA", np.uint8)
    truth, toff = np.frombuffer(b"TTACTTAGGNNTGCC", np.uint8), np.array([0, 8, 10, 15], np.int64)
    for strands in (2, 1):
        seq, qual, off, blk = rv.merge_calls_infix_device(b, [5, 0, 4], z, z, truth, toff, strands)
        assert seq.tobytes() == b.tobytes() and off.tolist() == [0, 5, 5, 9]
        _same(blk, hs.read_infix(b, [5, 0, 4], seq, off, truth, toff, strands), ("no window", strands))
        assert blk[:, :2].tolist() == [[8, strands], [2, strands], [5, strands]] and np.array_equal(blk[:, 2:10], blk[:, 10:18])
        assert blk[0, 2:6].tolist() == [1, 4, 2, 7] and blk[1, 2:6].tolist() == [0, 0, 2, 2]
    ins = rv._merge_inputs(c["bases"], c["ev_len"], c["a1"], c["a2"], None, None, None, False)
    R = len(c["ev_len"])
    types = E._TRUTH[0][:2] + E._INFIX[0]
    for bad in (np.arange(1, R + 2), np.arange(R, -1, -1)):              # the C entry point refuses them under its own name
        more = E._marshal((np.zeros(R + 2, np.uint8), bad.astype(np.int64), 2, np.zeros((R, 18), np.uint64)), types)
        with pytest.raises(E.NrvError, match="nrv_merge_calls_infix"):
            rv._merge_call("nrv_merge_calls_infix", *ins, *more)
    for strands in (0, 3):
        more = E._marshal((np.zeros(1, np.uint8), np.zeros(R + 1, np.int64), strands, np.zeros((R, 18), np.uint64)), types)
        with pytest.raises(E.NrvError, match="nrv_merge_calls_infix.*strands"):
            rv._merge_call("nrv_merge_calls_infix", *ins, *more)
    rv.close()


@pytest.mark.parametrize("Tw", [1, 2, 32])
def test_merge_calls_infix_at_other_window_lengths(species_models, monkeypatch, Tw):
    rv = _engine(monkeypatch, *species_models["ecoli"], Tw=Tw)
    _merge_infix_checks(rv, report_case(T=Tw), Tw)
    rv.close()


# ---- 3 - 6. end to end ----------------------------------------------------------------------------------------------------------------
FLANKS = ((64, 90), (77, 64))                                            # characters before and behind each read's truth in its region


def _regions(truth, toff, rng):
    """Truth regions from exact truths: random flanks of 64 characters and more, every second region reverse-complemented."""
    parts = []
    for r in range(len(toff) - 1):
        t = random_seq(rng, FLANKS[r % 2][0]) + np.asarray(truth, np.uint8)[int(toff[r]):int(toff[r + 1])].tobytes() + random_seq(rng, FLANKS[r % 2][1])
        parts.append(revcomp(t) if r % 2 else t)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), off


@pytest.fixture(scope="module")
def regions_of_short_reads(truth_of_short_reads):
    """The 5 % mutation of the merged form of the two reads between random flanks, the second region reverse-complemented."""
    return _regions(*truth_of_short_reads, np.random.default_rng(43))


def _definition(rv, rrs, truth, toff, strands=2):
    seq, off = _merged(rv, rrs)
    return hs.read_infix(_bases(rrs), [len(r.starts) for r in rrs], seq, off, truth, toff, strands)


def _packed33(rv, rrs, fastq, inner, truth, strands=2, classes=True):
    p = _packed(rv, rrs, fastq, inner, truth)
    return rv.with_device_infix(rv.with_device_error_classes(p) if classes else p, strands)


def _check_call(got, plain, want, what):
    """A form-33 result: the infix block last, every other output that of the form 31 call."""
    assert len(got) == 13 and len(plain) == 12, what
    _same(got[12], want, what)
    for k, (g, p) in enumerate(zip(got, plain)):
        assert _eq(g, p), (what, k)


def _non_vacuous(want, toff):
    """On the DEFINITION's values: both reads lie strictly inside their regions, the second on the reverse strand, and the
    revision moved both closer to their truth."""
    assert (want[:, 0] == np.diff(toff)).all() and (want[:, 1] == 2).all(), want.tolist()
    assert [hs.pick_strand(w) for w in want] == ["+", "-"], want.tolist()
    for w, g in zip(want.tolist(), (2, 6)):
        d_in, _, st_in, en_in = w[g:g + 4]
        d_out, _, st_out, en_out = w[g + 8:g + 12]
        assert 0 < st_in and en_in < w[0] and 0 < st_out and en_out < w[0] and 0 < d_out < d_in, w


def _end_to_end(rv, short_reads, truth, toff):
    """The end-to-end forms on the two reads -> [(name, infix block)]; compared with the definition inside."""
    out = []
    rrs = [r for r, _ in short_reads]
    want = _definition(rv, rrs, truth, toff)
    _non_vacuous(want, toff)
    for fastq, inner in ((False, "alone"), (True, "all")):
        got = rv.run_packed_raw(_packed33(rv, rrs, fastq, inner, (truth, toff)))
        plain = rv.run_packed_raw(rv.with_device_error_classes(_packed(rv, rrs, fastq, inner, (truth, toff))))
        _check_call(got, plain, want, ("one call", fastq, inner))
        out.append((f"one call {fastq} {inner}", got[12].copy()))
    # without the error classes: their place is None; one strand: the reverse groups are zeros
    got = rv.run_packed_raw(_packed33(rv, rrs, False, "alone", (truth, toff), 1, classes=False))
    one = want.copy()
    one[:, 1], one[:, 6:10], one[:, 14:18] = 1, 0, 0
    assert len(got) == 13 and got[11] is None
    _same(got[12], one, "forward alone, no error classes")
    out.append(("forward", got[12].copy()))
    # two calls in flight, one read each
    ta = rv.begin_packed_raw(_packed33(rv, rrs[:1], True, "all", (truth[:toff[1]], toff[:2])))
    tb = rv.begin_packed_raw(_packed33(rv, rrs[1:], False, "alone", (truth[toff[1]:], toff[1:] - toff[1])))
    ga, gb = rv.end_packed_raw(ta), rv.end_packed_raw(tb)
    _same(np.concatenate([ga[12], gb[12]]), want, "the two calls are the one call's reads")
    # one read without a truth
    got = rv.run_packed_raw(_packed33(rv, rrs, False, "alone", (truth[toff[1]:], np.array([0, 0, toff[2] - toff[1]], np.int64))))
    _same(got[12], np.stack([np.zeros(18, np.uint64), want[1]]), "no truth for the first read")
    # no window at all (N <= T): filled on the host
    r0 = rrs[0]
    p = rv.pack_reads_raw([r0.raw, r0.raw], [r0.starts[:rv.T - 3], r0.starts[:3]], [r0.feat_ev[:rv.T - 3], r0.feat_ev[:3]], [r0.shift] * 2, [r0.scale] * 2, rv.T)
    b = np.concatenate([np.asarray(r0.bases, "S1")[:rv.T - 3], np.asarray(r0.bases, "S1")[:3]]).view(np.uint8)
    t2, o2 = np.frombuffer(b"ACGTACGTAC", np.uint8), np.array([0, 10, 10], np.int64)
    got = rv.run_packed_raw(rv.with_device_infix(rv.with_device_accuracy(rv.with_device_merge(p, b, True), t2, o2)))
    _same(got[12], hs.read_infix(b, [rv.T - 3, 3], got[0], got[2], t2, o2), "no window")
    assert got[12][0, 0] == 10 and np.array_equal(got[12][0, 2:10], got[12][0, 10:18]) and not got[12][1].any()
    return out


def test_revise_reads_raw_infix_equals_the_definition(species_models, short_reads, regions_of_short_reads, monkeypatch):
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for mode in MODES:
        rv.set_precision(mode)
        _end_to_end(rv, short_reads, *regions_of_short_reads)
        assert rv.saturated() == (0, 0), mode
    rv.close()


def test_infix_call_refuses_bad_input_by_its_name(species_models, short_reads, regions_of_short_reads, monkeypatch):
    from nanoreviser_amd.engine import INFIX_MAX_LEN, NrvError
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rrs = [r for r, _ in short_reads]
    truth, toff = regions_of_short_reads
    p = _packed33(rv, rrs, True, "alone", (truth, toff))
    big = np.full(INFIX_MAX_LEN + 1, ord("A"), np.uint8)
    for k, v in ((28, None), (32, None), (28, toff + 1), (28, toff[::-1].copy()), (26, np.zeros((2, 2), np.int64)), (31, 0), (31, 3)):
        with pytest.raises(NrvError, match="nrv_revise_reads_raw_infix_begin"):
            rv.run_packed_raw(p[:k] + (v,) + p[k + 1:])
    with pytest.raises(NrvError, match="nrv_revise_reads_raw_infix_begin.*NRV_INFIX_MAX_LEN"):
        rv.run_packed_raw(p[:27] + (big, np.array([0, 0, big.size], np.int64)) + p[29:])
    _same(rv.run_packed_raw(p)[12], _definition(rv, rrs, truth, toff), "the handle is usable after a refusal")
    rv.close()


def test_range_guard_rerun_gives_the_f32_block(species_models, short_reads, monkeypatch):
    """The spiked read of tests/test_gpu_device_accuracy.py behind a clean one: nrv_reads_raw_end runs the whole call again on the
    f32 kernels; the kernel runs again on the re-merged reads and stores every word again - the "out" groups are the f32
    mode's, the "in" groups what they were."""
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
    truth, toff = _regions(*truth_for_reads(np.random.default_rng(12), seq, off, 0.05), np.random.default_rng(13))
    want = hs.read_infix(bases, el, seq, off, truth, toff)
    assert rv.saturated()[1] == 0 and (want[:, 2:6] != want[:, 10:14]).any(1).all() and [hs.pick_strand(w) for w in want] == ["+", "-"]
    rv.set_precision("f16x2")
    r0 = rv.saturated()[1]
    p = rv.with_device_report(rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, True))
    got = rv.run_packed_raw(rv.with_device_infix(rv.with_device_error_classes(rv.with_device_accuracy(p, truth, toff))))
    assert rv.saturated()[1] - r0 == 1
    _same(got[12], want, "re-run")
    rv.close()


def test_poisoned_workspace_gives_the_same_block(species_models, short_reads, regions_of_short_reads, planted, monkeypatch):
    clean = _engine(monkeypatch, *species_models["ecoli"])
    ref = _end_to_end(clean, short_reads, *regions_of_short_reads)
    clean.close()
    S = 64 * strip()
    carry = {rev: [k for k, t in enumerate(planted[rev][1]) if len(t) > S] for rev in (0, 1)}    # more than one stripe: they read the carry words
    assert min(len(v) for v in carry.values()) >= 40
    c = profile_case()
    truth, toff, _ = _regions_for_case(c, T, 200 + T)
    seq_w, _, off_w = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], None, T)
    want_c = hs.read_infix(c["bases"], c["ev_len"], seq_w, off_w, truth, toff)
    for poison in PATTERNS:
        rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
        for p in range(2):
            got = _end_to_end(rv, short_reads, *regions_of_short_reads)
            assert [k for k, _ in got] == [k for k, _ in ref]
            for (k, x), (_, y) in zip(ref, got):
                _same(y, x, (poison, p, k))
            for rev in (0, 1):
                names, regions, rds, want = planted[rev]
                _same(_classes(rv, [regions[k] for k in carry[rev]], [rds[k] for k in carry[rev]], rev), want[carry[rev]], (poison, p, rev, "carry"))
            _same(rv.merge_calls_infix_device(c["bases"], c["ev_len"], c["a1"], c["a2"], truth, toff)[3], want_c, (poison, p, "merge"))
        assert rv.saturated() == (0, 0), poison
        rv.close()


# ---- 7. command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_infix_is_the_same_on_the_device_route(tmp_path, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_SUMMARY",
              "NRV_TRIM_Q", "NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES", "NRV_INFIX"):
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
    fa = str(tmp_path / "regions.fa")
    outs, infs = {}, {}
    for tag, extra, form in (("plain", [], 7), ("host", ["truth"], 7), ("device", ["--device_merge", "truth"], 33),
                             ("trim_plain", ["--device_merge", "--trim_q", "3"], 27), ("trim", ["--device_merge", "--trim_q", "3", "truth"], 33),
                             ("forward", ["--device_merge", "--infix_strand", "forward", "truth"], 33)):
        del forms[:]
        out = str(tmp_path / tag) + "/"
        argv = ["-d", str(d), "-o", out, "-S", "ecoli", "--gpus", "1", "--thread", "4"]
        argv += [x for e in extra for x in (["--truth", fa, "--infix", str(tmp_path / (tag + ".inf"))] if e == "truth" else [e])]
        assert cli.main(argv) == 0
        outs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        assert outs[tag]["failed_reads.txt"] == b"" and forms and set(forms) == {form}, (tag, forms)
        assert not glob.glob(str(tmp_path / "*.part*")) and not glob.glob(out + "*.part*")
        if "truth" in extra:
            infs[tag] = open(str(tmp_path / (tag + ".inf")), "rb").read()
        if tag == "plain":                          # the regions: a seeded 5 % mutation of what the plain run wrote, between flanks
            rng = np.random.default_rng(8)
            with open(fa, "w") as fp:
                for i in range(n):
                    if i != 2:                                              # one read left out; every second region on the other strand
                        t = random_seq(rng, 64 + i) + mutate(rng, outs[tag][f"s{i:02d}_out.fasta"].split(b"\n")[1], 0.05) + random_seq(rng, 80)
                        t = (revcomp(t) if i % 2 else t).decode()
                        fp.write(f">s{i:02d}{'.fast5' if i % 2 else ''}\n" + "".join(t[k:k + 70] + "\n" for k in range(0, len(t), 70)))
    assert infs["device"] == infs["host"] == infs["trim"]
    assert outs["host"] == outs["device"] == outs["forward"] == outs["plain"] and outs["trim"] == outs["trim_plain"] and len(outs["plain"]) == n + 1
    lines = [ln.split("\t") for ln in infs["host"].decode().split("\n")]
    assert lines[0] == cli.INFIX_HEADER.split("\t") and lines[-2] == ["#reads", str(n - 1), "1", "0"] and lines[-3][:2] == ["#total", "with_truth"]
    fwd = [ln.split("\t") for ln in infs["forward"].decode().split("\n")]
    for i, (c, f) in enumerate(zip(lines[1:n + 1], fwd[1:n + 1])):
        assert c[0] == f"s{i:02d}.fast5" and c[1] == "revised"
        if i == 2:
            assert c[2:] == f[2:] == ["0"] + ["."] * 13
            continue
        m, strand = int(c[2]), c[3]
        (n_in, d_in, M_in, st_in, en_in), (n_out, d_out, M_out, st_out, en_out) = map(int, c[4:9]), map(int, c[10:15])
        assert strand == "+-"[i % 2] and f[3] == "+"
        # the read lies inside the flanks, on the region as given, and the revision moved it closer
        lo, hi = (80, 64 + i) if i % 2 else (64 + i, 80)
        assert abs(st_out - lo) <= 20 and abs((m - en_out) - hi) <= 20 and 0 < st_in and en_in < m and 0 < d_out < d_in
        assert c[9] == f"{M_in / (M_in + d_in):.6f}" and c[15] == f"{M_out / (M_out + d_out):.6f}"
        assert (f[4:] == c[4:]) == (strand == "+") and int(f[5]) >= d_in
    tot = lines[-3]
    assert [tot[k] for k in (3, 7, 8, 13, 14)] == ["."] * 5
    assert [int(tot[k]) for k in (2, 4, 5, 6, 10, 11, 12)] == [sum(int(c[k]) for c in lines[1:n + 1] if c[3] != ".") for k in (2, 4, 5, 6, 10, 11, 12)]
    assert tot[9] == f"{int(tot[6]) / (int(tot[6]) + int(tot[5])):.6f}" and tot[15] == f"{int(tot[12]) / (int(tot[12]) + int(tot[11])):.6f}"
