"""Truth regions, infix alignment on both strands, on the host (no GPU): hoststage.infix_classes against three references that
share no code with it, hoststage.read_infix, hoststage.pick_strand, the length limit, the packed form 33, the routing table,
--infix / --infix_strand and their refusals, the line and #total formats, and the command line on stand-in engines on every host
route.  Integers and bytes only: nothing here has a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

from accuracy_cases import mutate, random_seq
from conftest import load_read
from echo_engine import EchoEngine, HashEngine, hash_factory
from infix_cases import SMALL, TINY, diagonal_infix, lengths, loop_infix, planted_cases, reference, revcomp, strip, substring_infix
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from report_cases import report_case
from test_accuracy_host import FAST5, _Recorder, _clean_env, _expected, _files, _many, _packed12
from test_errclass_host import ClassesHash

T = 11


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def test_infix_classes_equals_the_references_on_every_planted_pair():
    cases, known = planted_cases()
    ref = reference()
    R = strip()
    S = 64 * R
    assert {0, 1, 2, R - 1, R, R + 1, 63, 64, 65, S - 1, S, S + 1, S + R, 2 * S + 1, 3 * S + 1} == set(lengths())
    assert len(cases) > 1200 and len(known) > 250
    tiny = small = 0
    for name, (t, s, rev) in cases.items():
        got = hs.infix_classes(t, s, bool(rev))
        assert got == ref[name], name
        if len(t) <= SMALL and len(s) <= SMALL:
            assert got == loop_infix(t, s, rev), name
            small += 1
        if len(t) <= TINY and len(s) <= TINY:
            assert got == substring_infix(t, s, rev), name
            tiny += 1
        if name in known:
            assert got == known[name], name
        d, M, start, end = got
        assert 0 <= start <= end <= len(t) and 0 <= M <= min(end - start, len(s)) and 0 <= d <= len(s), name
        # swapping `reverse` on the reverse-complemented region gives the same answer
        assert hs.infix_classes(revcomp(t), s, not rev) == got, name
    assert tiny >= 800 and small >= 1000
    # the shapes the wave can go wrong at are there, with known answers: a cut from stripe 0 into stripe 1, one that ends in stripe
    # 0 of three, one that ends exactly at m, on both strands
    m3 = 3 * S + 1
    for name, want in ((f"m={2 * S + 1} cut {S - 20}:{S + 20} +", (0, 40, S - 20, S + 20)), (f"m={m3} cut 100:140 +", (0, 40, 100, 140)),
                       (f"m={m3} cut 100:140 -", (0, 40, m3 - 140, m3 - 100)), (f"m={m3} cut {m3 - 30}:{m3} +", (0, 30, m3 - 30, m3)),
                       (f"m={S + 200} twice +", (0, 20, S - 10, S + 10)), ("AC / CA", (1, 1, 1, 2))):
        assert known[name] == want, name
    assert hs.infix_classes(b"TTTTACGTACGTTTTT", b"ACGTACG") == (0, 7, 4, 11)
    assert hs.infix_classes(b"ACGT", b"") == (0, 0, 4, 4) and hs.infix_classes(b"", b"ACG") == (3, 0, 0, 0) and hs.infix_classes(b"", b"") == (0, 0, 0, 0)
    assert hs.infix_classes("ACGTTT", np.frombuffer(b"AACG", np.uint8), reverse=True) == (0, 4, 1, 5)
    assert hs.infix_classes(b"NNNN", b"NNNN") == (4, 0, 4, 4) and hs.infix_classes(b"nnAC", b"GT", True) == (0, 2, 0, 2)


def test_infix_classes_on_random_pairs():
    rng = np.random.default_rng(16)
    alphabet = np.frombuffer(b"ACGTNa", np.uint8)
    for k in range(300):
        m, n = int(rng.integers(0, 120)), int(rng.integers(0, 90))
        t = alphabet[rng.integers(0, 6, m)].tobytes()
        a = int(rng.integers(0, m + 1))
        s = mutate(rng, t[a:a + n], 0.2) if k % 2 else alphabet[rng.integers(0, 6, n)].tobytes()
        rev = bool(k % 3 == 0)
        s = revcomp(s) if rev and k % 2 else s
        assert hs.infix_classes(t, s, rev) == loop_infix(t, s, rev) == diagonal_infix(t, s, rev), (t, s, rev)


def test_the_length_limit():
    assert hs.INFIX_MAX_LEN == (1 << 21) - 1
    big = np.full(hs.INFIX_MAX_LEN + 1, ord("A"), np.uint8)
    with pytest.raises(ValueError):
        hs.infix_classes(big, b"ACGT")
    with pytest.raises(ValueError):
        hs.infix_classes(b"ACGT", big)
    assert hs.infix_classes(big[:-1], b"") == (0, 0, hs.INFIX_MAX_LEN, hs.INFIX_MAX_LEN)


def _regions(rng, seq, off, without=(), flank=20):
    """Truth regions of merged reads: a seeded 10 % mutation between random flanks, every other one reverse-complemented."""
    parts = []
    for r in range(len(off) - 1):
        t = random_seq(rng, flank + r) + mutate(rng, np.asarray(seq, np.uint8)[int(off[r]):int(off[r + 1])].tobytes(), 0.1) + random_seq(rng, flank)
        parts.append(b"" if r in without else (revcomp(t) if r % 2 else t))
    toff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), toff


@pytest.mark.parametrize("T_", [1, 2, 11, 32])
def test_read_infix_on_report_case_inputs(T_):
    c = report_case(T=T_)
    seq, _, off = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], None, T_)
    R = len(c["ev_len"])
    without = (1, R - 2)
    truth, toff = _regions(np.random.default_rng(T_), seq, off, without)
    blk = hs.read_infix(c["bases"], c["ev_len"], seq, off, truth, toff)
    one = hs.read_infix(c["bases"], c["ev_len"], seq, off, truth, toff, strands=1)
    assert blk.dtype == np.uint64 and blk.shape == (R, 18) == (R, hs.INFIX_COLS)
    ev_off = np.cumsum(c["ev_len"]) - c["ev_len"]
    strands = set()
    for r in range(R):
        t = truth[toff[r]:toff[r + 1]].tobytes()
        if not t:
            assert not blk[r].any() and not one[r].any()
            continue
        b, s = c["bases"][ev_off[r]:ev_off[r] + c["ev_len"][r]].tobytes(), seq[off[r]:off[r + 1]].tobytes()
        assert blk[r].tolist() == [len(t), 2, *diagonal_infix(t, b), *diagonal_infix(t, b, True), *diagonal_infix(t, s), *diagonal_infix(t, s, True)], r
        assert one[r].tolist() == [len(t), 1, *diagonal_infix(t, b), 0, 0, 0, 0, *diagonal_infix(t, s), 0, 0, 0, 0], r
        assert hs.pick_strand(one[r]) == "+"
        if len(s) >= 12:
            assert hs.pick_strand(blk[r]) == "+-"[r % 2], r
        strands.add(hs.pick_strand(blk[r]))
    assert not blk[list(without)].any() and strands == {"+", "-"}
    for bad in (dict(strands=0), dict(strands=3)):
        with pytest.raises(ValueError):
            hs.read_infix(c["bases"], c["ev_len"], seq, off, truth, toff, **bad)
    with pytest.raises(ValueError):
        hs.read_infix(c["bases"], c["ev_len"], seq, off[:-1], truth, toff)


def test_pick_strand():
    row = lambda fwd, rev, strands=2: [100, strands, *fwd, *rev] + [0] * 8
    assert hs.pick_strand(row((5, 90, 1, 96), (5, 90, 3, 98))) == "+"          # equal: the forward strand
    assert hs.pick_strand(row((5, 90, 1, 96), (4, 80, 3, 98))) == "-"          # fewer edits
    assert hs.pick_strand(row((5, 90, 1, 96), (5, 91, 3, 98))) == "-"          # as many edits, more matches
    assert hs.pick_strand(row((5, 90, 1, 96), (5, 89, 3, 98))) == "+" and hs.pick_strand(row((5, 90, 1, 96), (6, 99, 3, 98))) == "+"
    assert hs.pick_strand(row((5, 90, 1, 96), (0, 0, 0, 0), 1)) == "+"         # one strand run: its zeros are not a result
    assert hs.pick_strand(np.array(row((5, 90, 1, 96), (4, 80, 3, 98)), np.uint64)) == "-"
    assert hs.pick_strand([0] * 18) == "+"
    # only the ORIGINAL read's groups decide
    assert hs.pick_strand([100, 2, 5, 90, 1, 96, 5, 90, 3, 98, 9, 9, 9, 9, 0, 50, 0, 50]) == "+"


# ---- form 33 ----------------------------------------------------------------------------------------------------------------------
def test_form_33_marshals_strands_and_the_block_last():
    from nanoreviser_amd import engine
    from nanoreviser_amd.engine import Reviser
    assert set(engine._RAW_FORMS_INFIX) == {33} and 33 not in engine._RAW_FORMS and 33 not in engine._RAW_FORMS_TRUTH
    assert engine.INFIX_COLS == hs.INFIX_COLS == 18 and engine.INFIX_R >= 1 and engine.INFIX_MAX_LEN == hs.INFIX_MAX_LEN
    assert {"nrv_revise_reads_raw_infix_begin", "nrv_revise_reads_raw_infix", "nrv_merge_calls_infix", "nrv_infix_classes"} <= set(engine.SYMBOLS)
    p12 = _packed12()
    truth, toff = np.frombuffer(b"ACGTAC", np.uint8), np.array([0, 4, 6], np.int64)
    rv = Reviser.__new__(Reviser)
    rv._lib, rv._h = _Recorder(), C.c_void_p(0)
    addr = lambda x: C.cast(x, C.c_void_p).value
    p30 = Reviser.with_device_accuracy(p12, truth, toff)
    p31 = Reviser.with_device_error_classes(p30)
    for base, strands in ((p30, 2), (p31, 1)):
        p = Reviser.with_device_infix(base, strands)
        assert len(p) == 33 and all(p[k] is base[k] for k in range(len(base))) and p[31] == strands
        assert (p[30] is None) == (len(base) == 30) and p[32].shape == (2, 18) and p[32].dtype == np.uint64
        del rv._lib.calls[:]
        t = rv.begin_packed_raw(p)
        (name, args), = rv._lib.calls
        assert name == "nrv_revise_reads_raw_infix_begin" and len(args) == 33 + 3 + 1
        assert addr(args[32]) == p[29].ctypes.data and addr(args[35]) == p[32].ctypes.data and args[34] == strands
        assert (addr(args[33]) is None) == (len(base) == 30)
        assert len(t) == 3 and len(t[1]) == 13 and t[1][12] is p[32] and t[1][11] is p[30] and t[1][10] is p[29]
        out = rv.run_packed_raw(p)
        assert rv._lib.calls[-1][0] == "nrv_revise_reads_raw_infix" and len(rv._lib.calls[-1][1]) == 36
        assert len(out) == 13 and out[12] is p[32] and out[11] is p[30] and out[10] is p[29] and out[9] is None
        assert len(cli._host_merge_form(p)) == 7
    assert Reviser.with_device_infix(p30)[31] == 2
    for bad in (p12, p30[:27], p):
        with pytest.raises(ValueError):
            Reviser.with_device_infix(bad)
    with pytest.raises(ValueError):
        Reviser.with_device_infix(p30, 3)
    # a library without the entry points: found by presence
    rv._lib = _Recorder(without=("infix",))
    with pytest.raises(engine.NrvError, match="has no nrv_revise_reads_raw_infix_begin"):
        rv.begin_packed_raw(p)
    rv.begin_packed_raw(p31)                                             # ... and the form 31 call still goes through
    assert rv._lib.calls[-1][0] == "nrv_revise_reads_raw_errclass_begin"
    for call in (lambda: rv.infix_classes_device([b"A"], [b"A"]), lambda: rv.infix_classes_offsets(b"A", [0, 1], b"A", [0, 1]),
                 lambda: rv.merge_calls_infix_device(np.frombuffer(b"ACGT", np.uint8), [4], [], [], b"", [0, 0])):
        with pytest.raises(engine.NrvError, match="this build of libnanorev_hip.so has no nrv_"):
            call()
    rv._lib = _Recorder()
    got = rv.infix_classes_device([b"ACG", b""], [b"A", b"CC"], reverse=True)
    (name, args), = rv._lib.calls
    assert name == "nrv_infix_classes" and len(args) == 11 and args[5] == 2 and args[6] == 1 and [g.shape for g in got] == [(2,)] * 4
    with pytest.raises(ValueError):
        rv.infix_classes_device([b"A"], [])
    rv._h = None


def test_route_batch_with_infix():
    class Full:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = with_device_trim = with_device_accuracy = with_device_error_classes = None
        with_device_infix = None

    class NoInfix:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = with_device_trim = with_device_accuracy = with_device_error_classes = None

    class NoAccuracy:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = with_device_trim = with_device_infix = None
    bundle = {"bases": np.zeros(5, "S1"), "meta": np.array([[0, 5, 0, 0]])}
    route = lambda rv, dm, **kw: cli._route_batch(rv, bundle, 1, True, True, dm, False, **kw)
    assert route(Full, True, infix=True) == (33, "pipelined")                  # without --accuracy too
    assert route(Full, True, accuracy=True, infix=True) == (33, "pipelined")
    assert route(Full, True, accuracy=True, error_classes=True, infix=True, trim=True, combined=True, summary=True, edits=True) == (33, "pipelined")
    assert cli._route_batch(Full, bundle, 1, False, True, True, True, infix=True) == (33, "packed+finish_bundle")
    assert route(NoInfix, True, infix=True) == ("host-merge", "pipelined") and route(NoAccuracy, True, infix=True) == ("host-merge", "pipelined")
    assert route(NoInfix, True, accuracy=True, error_classes=True, infix=True) == ("host-merge", "pipelined")
    # the switch off: the existing answers
    assert route(Full, True, accuracy=True) == (30, "pipelined") and route(Full, True, accuracy=True, error_classes=True) == (31, "pipelined")
    assert route(Full, True) == (12, "pipelined") and route(Full, False, infix=True) == (7, "pipelined")
    doc = cli._route_batch.__doc__
    assert "33 [11]" in doc and "[11] " in doc


# ---- the switch --------------------------------------------------------------------------------------------------------------------
def test_infix_flag_parsing(monkeypatch, capsys):
    for k in ("NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES", "NRV_INFIX", "NRV_TRIM_Q"):
        monkeypatch.delenv(k, raising=False)
    base = ["-d", "x", "-o", "y"]
    assert cli.get_args(base).infix is None and cli.get_args(base).infix_strand == "both"
    a = cli.get_args(base + ["--truth", "t.fa", "--infix", "i.tsv"])                       # --accuracy is not needed
    assert (a.truth, a.accuracy, a.infix, a.infix_strand, a.accuracy_max_len) == ("t.fa", None, "i.tsv", "both", 65536)
    a = cli.get_args(base + ["--truth", "t.fa", "--accuracy", "a.tsv", "--infix", "i.tsv", "--infix_strand", "forward", "--accuracy_max_len", "9000"])
    assert (a.accuracy, a.infix, a.infix_strand, a.accuracy_max_len) == ("a.tsv", "i.tsv", "forward", 9000)
    # --accuracy_max_len is capped at the packed cell's limit next to --infix, and only there
    assert cli.get_args(base + ["--truth", "t.fa", "--infix", "i.tsv", "--accuracy_max_len", "5000000"]).accuracy_max_len == hs.INFIX_MAX_LEN
    assert cli.get_args(base + ["--truth", "t.fa", "--accuracy", "a.tsv", "--accuracy_max_len", "5000000"]).accuracy_max_len == 5000000
    monkeypatch.setenv("NRV_INFIX", "env.tsv")
    assert cli.get_args(base + ["--truth", "t.fa"]).infix == "env.tsv"
    with pytest.raises(SystemExit) as e:                                  # the environment's switch is refused alone as well
        cli.get_args(base)
    assert e.value.code == 2 and "--infix goes with --truth" in capsys.readouterr().err
    monkeypatch.delenv("NRV_INFIX")
    for bad, msg in ((["--infix", "i.tsv"], "--infix goes with --truth"),
                     (["--infix", "i.tsv", "--accuracy", "a.tsv"], "--infix goes with --truth"),
                     (["--truth", "t.fa", "--infix", "i.tsv", "--resume"], "--resume cannot be used with --infix"),
                     (["--truth", "t.fa", "--infix", "i.tsv", "--accuracy_max_len", "-1"], "--accuracy_max_len must be 0 or more"),
                     (["--truth", "t.fa"], "--truth and --accuracy go together")):
        with pytest.raises(SystemExit) as e:
            cli.get_args(base + bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        cli.get_args(base + ["--truth", "t.fa", "--infix", "i.tsv", "--infix_strand", "reverse"])


def test_line_and_total_format():
    assert cli.INFIX_HEADER.split("\t") == ["name", "status", "truth_len", "strand", "len_in", "dist_in", "match_in", "start_in", "end_in", "id_in",
                                           "len_out", "dist_out", "match_out", "start_out", "end_out", "id_out"]
    W = cli.ACC_WITH_TRUTH
    # region 100; the original (97 long) fits the forward strand better
    fwd = [100, 2, 97, 95, 12, 85, 2, 99, 60, 30, 0, 90, 3, 92, 1, 96, 50, 40, 5, 95, W]
    assert len(fwd) == cli.INFIX_PART_COLS == 21
    assert cli.infix_fields(fwd) == ["100", "+", "97", "12", "85", "2", "99", f"{85 / 97:.6f}", "95", "3", "92", "1", "96", f"{92 / 95:.6f}"]
    # ... the reverse strand: both forms are reported on it, start / end on the region as given: m - end, m - start
    rev = [100, 2, 97, 95, 60, 30, 0, 90, 12, 85, 2, 99, 50, 40, 5, 95, 3, 92, 1, 96, W]
    assert cli.infix_fields(rev) == ["100", "-", "97", "12", "85", "1", "98", f"{85 / 97:.6f}", "95", "3", "92", "4", "99", f"{92 / 95:.6f}"]
    # the ORIGINAL decides: a revised read that fits the other strand better is still reported on the original's
    odd = [100, 2, 97, 95, 12, 85, 2, 99, 60, 30, 0, 90, 50, 40, 5, 95, 3, 92, 1, 96, W]
    assert cli.infix_fields(odd)[1] == "+" and cli.infix_fields(odd)[8:10] == ["95", "50"]
    one = [100, 1, 97, 95, 12, 85, 2, 99, 0, 0, 0, 0, 3, 92, 1, 96, 0, 0, 0, 0, W]
    assert cli.infix_fields(one)[1] == "+" and cli.infix_fields(one)[3] == "12"
    for flag in (cli.ACC_NO_TRUTH, cli.ACC_TOO_LONG):
        assert cli.infix_fields([0, 0, 97, 101] + [0] * 16 + [flag]) == ["0"] + ["."] * 13
    assert cli.infix_identity(0, 0) == "." and cli.infix_identity(3, 1) == "0.750000" and cli.infix_identity(0, 4) == "0.000000"
    assert cli.infix_fields([5, 2, 0, 0, 0, 0, 5, 5, 0, 0, 5, 5, 0, 0, 5, 5, 0, 0, 5, 5, W])[7] == "."      # an empty read: no column
    assert cli.infix_sums(rev) == [100, 97, 12, 85, 95, 3, 92]
    blk = np.array([[100, 2, 12, 85, 2, 99, 60, 30, 0, 90, 3, 92, 1, 96, 50, 40, 5, 95], [0] * 18, [5, 2] + [1] * 16], np.uint64)
    rows = cli.InfixPart.rows(blk, [97, 8, 5], [95, 9, 5], [W, cli.ACC_NO_TRUTH, cli.ACC_TOO_LONG])
    assert rows == [fwd, [0, 0, 8, 9] + [0] * 16 + [cli.ACC_NO_TRUTH], [0, 0, 5, 5] + [0] * 16 + [cli.ACC_TOO_LONG]]


# ---- the command line on stand-in engines ----------------------------------------------------------------------------------------
class InfixHash(ClassesHash):
    """ClassesHash with form 33: the infix block by the host definition from the same calls."""
    with_device_infix = staticmethod(lambda *a, **k: ClassesHash._cls().with_device_infix(*a, **k))

    def begin_packed_raw(self, packed):
        if len(packed) != 33:
            return super().begin_packed_raw(packed)
        t, outs, merged = super().begin_packed_raw(tuple(packed[:30 if packed[30] is None else 31]))
        self.forms[-1] = 33
        _, _, a1, a2 = HashEngine.predict_read(self, None, packed[2])
        el = [int(d.ev_len) for d in packed[3]]
        seq, _, off = hs.emit_calls(packed[9], el, a1, a2, None, self.T)
        none = (None,) if packed[30] is None else ()
        return t, outs + none + (hs.read_infix(packed[9], el, seq, off, packed[27], packed[28], packed[31]),), merged


FLANKS = (70, 45)                                                        # characters before and behind the truth in its region
_REGIONS = {}


def _expected_regions():
    """Per fixture read (A, B) of the hash engine: (original, revised, the region - `test_accuracy_host._expected`'s truth between
    random flanks, B's reverse-complemented -, then the reference's tuple of (original | revised) x (forward | reverse)), once
    per process."""
    if not _REGIONS:
        rng = np.random.default_rng(78)
        for k, (orig, seq, truth, _, _) in _expected().items():
            region = random_seq(rng, FLANKS[0]) + truth + random_seq(rng, FLANKS[1])
            region = revcomp(region) if k else region
            _REGIONS[k] = (orig, seq, region, [diagonal_infix(region, s, rev) for s in (orig, seq) for rev in (0, 1)])
    return _REGIONS


def _write_regions(path, names, leave_out=()):
    exp = _expected_regions()
    with open(path, "w") as fp:
        for i, fn in enumerate(names):
            if fn in leave_out:
                continue
            t = exp[i % 2][2].decode()
            t = t.lower() if i % 3 == 0 else t
            fp.write(f">{fn if i % 2 else fn[:-6]} region of read {i}\n" + "".join(t[k:k + 60] + "\n" for k in range(0, len(t), 60)))
    return path


def _want_tsv(names, leave_out=(), too_long=(), unrevised=(), forward=False):
    exp = _expected_regions()
    lines, tot, n_reads = [cli.INFIX_HEADER], [0] * 7, [0, 0, 0]
    ident = lambda M, d: f"{M / (M + d):.6f}" if M + d else "."
    for i, fn in enumerate(sorted(names)):
        orig, seq, region, g = exp[i % 2]
        status = "unrevised" if fn in unrevised else "revised"
        if fn in leave_out or fn in too_long:
            lines.append(f"{fn}\t{status}\t0" + "\t." * 13)
            n_reads[2 if fn in too_long else 1] += 1
            continue
        m = len(region)
        minus = not forward and (g[1][0], -g[1][1]) < (g[0][0], -g[0][1])
        assert minus == (i % 2 == 1 and not forward)                     # B's region lies on the other strand
        v = [m]
        for n, (fw, rv) in ((len(orig), g[:2]), (len(orig), g[:2]) if fn in unrevised else (len(seq), g[2:])):
            d, M, st, en = rv if minus else fw
            st, en = (m - en, m - st) if minus else (st, en)
            v += [n, d, M, st, en]
        lines.append(f"{fn}\t{status}\t{m}\t{'-' if minus else '+'}\t" + "\t".join(str(x) for x in v[1:6]) + "\t" + ident(v[3], v[2])
                     + "\t" + "\t".join(str(x) for x in v[6:11]) + "\t" + ident(v[8], v[7]))
        tot = [a + b for a, b in zip(tot, [v[0], v[1], v[2], v[3], v[6], v[7], v[8]])]
        n_reads[0] += 1
    lines.append("\t".join(["#total", "with_truth", str(tot[0]), ".", str(tot[1]), str(tot[2]), str(tot[3]), ".", ".", ident(tot[3], tot[2]),
                            str(tot[4]), str(tot[5]), str(tot[6]), ".", ".", ident(tot[6], tot[5])]))
    lines.append("#reads\t" + "\t".join(str(x) for x in n_reads))
    return ("\n".join(lines) + "\n").encode()


def _memoised(monkeypatch):
    """hoststage.infix_classes behind a table keyed by the triple: the routes below ask for the same few long pairs again and again."""
    real, table = hs.infix_classes, {}

    def infix_classes(truth, seq, reverse=False):
        key = (bytes(hs._as_u8(truth)), bytes(hs._as_u8(seq)), bool(reverse))
        if key not in table:
            table[key] = real(truth, seq, reverse)
        return table[key]
    monkeypatch.setattr(hs, "infix_classes", infix_classes)
    return table


def test_infix_file_is_the_same_on_every_route(tmp_path, monkeypatch, capsys):
    import __graft_entry__ as g
    from nanoreviser_amd import hostlib
    g.build_host()
    _clean_env(monkeypatch)
    for k in ("NRV_ERROR_CLASSES", "NRV_INFIX"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib, "_lib", None)
    assert hostlib.load() is not None
    table = _memoised(monkeypatch)
    exp = _expected_regions()
    for k, (orig, seq, region, g4) in exp.items():
        # not vacuous: the read lies strictly inside its region, B's on the other strand, and the revision moved it closer
        best = 1 if k else 0
        assert g4[best][2] > 0 and g4[best][3] < len(region) and g4[2 + best][0] < g4[best][0] < g4[1 - best][0], (k, g4)
    src = _many(tmp_path, 6)
    names = sorted(os.listdir(src))
    leave_out = (names[1], names[4])
    fa = _write_regions(str(tmp_path / "regions.fa"), names, leave_out)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                           # several device calls for these reads
    want = _want_tsv(names, leave_out)
    assert b"\t-\t" in want and b"\t+\t" in want

    def run(tag, extra=(), infix=True, classes=False, **kw):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "--batch", "1024"] + list(extra)
        if infix:
            argv += ["--truth", fa, "--infix", out + "inf.tsv"]
        if classes:
            argv += ["--truth", fa, "--accuracy", out + "acc.tsv", "--error_classes", out + "ecl.tsv"]
        assert cli.main(argv, **kw) == 0
        assert not [f for f in os.listdir(out) if ".part" in f or ".tmp" in f]
        return out

    eng_0 = InfixHash()
    plain = _files(run("plain", ["--device_merge"], infix=False, reviser_factory=lambda a, dev: eng_0))
    assert "inf.tsv" not in plain and set(eng_0.forms) == {12} and not table            # the switch off: as it was
    eng_p = InfixHash()
    capsys.readouterr()
    piped = run("piped", reviser_factory=lambda a, dev: eng_p)
    assert capsys.readouterr().out.count("--infix: the reads are placed in their truth regions by the host stage") == 1
    eng_m = InfixHash()
    merged = run("merged", ["--device_merge"], reviser_factory=lambda a, dev: eng_m)
    assert "--infix: the reads are placed" not in capsys.readouterr().out
    assert set(eng_p.forms) == {7} and set(eng_m.forms) == {33} and len(eng_m.forms) >= 2
    seq_run = run("seq", ["--thread", "1"], reviser_factory=lambda a, dev: HashEngine())
    for o in (piped, merged, seq_run):
        f = _files(o)
        assert f.pop("inf.tsv") == want, o
        assert f == plain, o                                            # every other output is that of a run without it
    # next to --accuracy and --error_classes (form 33 on a form 31 tuple), trimmed: the same file, and theirs as without --infix
    eng_t, eng_c = InfixHash(), InfixHash()
    more = ["--device_merge", "--trim_q", "3"]
    both = _files(run("all", more, classes=True, reviser_factory=lambda a, dev: eng_t))
    ref = _files(run("ref", more, infix=False, classes=True, reviser_factory=lambda a, dev: eng_c))
    assert set(eng_t.forms) == {33} and set(eng_c.forms) == {31} and both.pop("inf.tsv") == want
    assert both["acc.tsv"] and both["ecl.tsv"] and both == ref
    # an engine with the error classes and without this call: the host merge, the same file
    eng_o = ClassesHash()
    old = run("old", ["--device_merge"], reviser_factory=lambda a, dev: eng_o)
    assert set(eng_o.forms) == {7} and _files(old)["inf.tsv"] == want
    # --infix_strand forward: every strand +, on both routes
    want_f = _want_tsv(names, leave_out, forward=True)
    assert b"\t-\t" not in want_f
    for tag, extra in (("fwd_host", []), ("fwd_dev", ["--device_merge"])):
        assert _files(run(tag, extra + ["--infix_strand", "forward"], reviser_factory=lambda a, dev: InfixHash()))["inf.tsv"] == want_f, tag
    # --accuracy_max_len applies: the longer kind has no truth and is counted as too long
    lens = [max(len(exp[k][0]), len(exp[k][2])) for k in (0, 1)]
    long_kind = int(np.argmax(lens))
    too_long = [fn for i, fn in enumerate(names) if i % 2 == long_kind and fn not in leave_out]
    want_cut = _want_tsv(names, leave_out, too_long)
    for tag, extra in (("cut_host", []), ("cut_dev", ["--device_merge"])):
        f = _files(run(tag, extra + ["--accuracy_max_len", str(min(lens))], reviser_factory=lambda a, dev: InfixHash()))
        assert f["inf.tsv"] == want_cut, tag
    assert want_cut.decode().split("\n")[-2] == f"#reads\t{6 - 2 - len(too_long)}\t2\t{len(too_long)}"


def test_infix_file_is_the_same_for_1_2_and_3_workers_and_split_reads(tmp_path, monkeypatch):
    _clean_env(monkeypatch)
    monkeypatch.delenv("NRV_INFIX", raising=False)
    _memoised(monkeypatch)                                               # (the parent's share: the split reads of the third run)
    src = _many(tmp_path, 4)
    names = sorted(os.listdir(src))
    fa = _write_regions(str(tmp_path / "regions.fa"), names, (names[2],))
    outs = {}
    for world, extra in ((1, []), (2, []), (3, ["--split_reads_above", "0.2"])):   # ... the last one: reads split over the workers, merged in the parent
        out = str(tmp_path / f"w{world}") + "/"
        assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "--truth", fa, "--infix", out + "inf.tsv"] + extra,
                        worker_factory=hash_factory, world=world) == 0
        outs[world] = _files(out)
    assert outs[1]["inf.tsv"] == _want_tsv(names, (names[2],)) and outs[2] == outs[1] and outs[3] == outs[1]


def test_an_unrevised_read_has_the_figures_of_what_was_written(tmp_path, monkeypatch):
    _clean_env(monkeypatch)
    monkeypatch.delenv("NRV_INFIX", raising=False)
    _memoised(monkeypatch)
    src = _many(tmp_path, 4)
    names = sorted(os.listdir(src))
    _, rdA, rtA = load_read("_".join(os.path.basename(FAST5[0]).split("_")[-3:-1]))
    fa = _write_regions(str(tmp_path / "regions.fa"), names)
    out = str(tmp_path / "o") + "/"
    eng = EchoEngine(fail_marker=rtA.feat_ev[0])                        # every call that STARTS with a read A fails
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "-e", "bad.txt", "--truth", fa, "--infix", out + "inf.tsv"],
                    reviser_factory=lambda a, dev: eng) == 0
    failed = set(open(out + "bad.txt").read().split())
    assert failed and "r00_A.fast5" in failed
    # the echo engine writes the original read back: revised or not, out = in
    want = _want_tsv(names, unrevised=names).decode().split("\n")
    got = open(out + "inf.tsv").read().split("\n")
    assert [ln.split("\t")[1] for ln in got[1:5]] == ["unrevised" if fn in failed else "revised" for fn in names]
    assert [ln.split("\t")[:1] + ln.split("\t")[2:] for ln in got[1:5]] == [ln.split("\t")[:1] + ln.split("\t")[2:] for ln in want[1:5]]
    assert got[5:] == want[5:] and got[0] == want[0]
    for ln in got[1:5]:
        c = ln.split("\t")
        assert c[4:10] == c[10:16]
