"""Substitution / insertion / deletion counts against a truth set on the host (no GPU): hoststage.edit_classes against three
references that share no code with it, hoststage.read_error_classes, the packed form 31, the routing table, --error_classes
and its refusals, the line and #total formats, and the command line on stand-in engines on every host route.  Integers and
bytes only: nothing here has a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

from accuracy_cases import loop_distance, mutate, truth_for_reads
from conftest import load_read
from echo_engine import EchoEngine, HashEngine, hash_factory
from errclass_cases import SMALL, TINY, all_alignments, counts, diagonal_classes, lengths, loop_classes, planted_cases, reference, strip
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from report_cases import report_case
from test_accuracy_host import FAST5, AccuracyHash, _Recorder, _clean_env, _expected, _files, _many, _packed12, _write_truth

T = 11


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def test_edit_classes_equals_the_references_on_every_planted_pair():
    cases, known = planted_cases()
    ref = reference()
    R = strip()
    assert len(cases) > 450 and sum(len(t) >= 64 * R - 1 for t, _ in cases.values()) <= 32
    assert {R - 1, R, R + 1, 64 * R - 1, 64 * R, 64 * R + 1, 64 * R + R, 128 * R + 1, 0, 1, 2, 63, 64, 65} == set(lengths())
    tiny = small = 0
    for name, (t, s) in cases.items():
        d, M = got = hs.edit_classes(t, s)
        assert got == ref[name], name
        if len(t) <= SMALL and len(s) <= SMALL:
            assert got == loop_classes(t, s), name
            small += 1
        if len(t) <= TINY and len(s) <= TINY:
            assert got == all_alignments(t, s), name
            tiny += 1
        if name in known:
            assert got == known[name], name
        # d is the d of edit_distance; the identities; all three counts are >= 0
        m, n = len(t), len(s)
        assert d == hs.edit_distance(t, s), name
        S, I, D = counts(m, n, d, M)
        assert M + S + I == n and M + S + D == m and S + I + D == d and min(S, I, D, M) >= 0, name
        # swapping truth and read swaps insertions and deletions
        d2, M2 = hs.edit_classes(s, t)
        assert (d2, M2) == (d, M) and counts(n, m, d2, M2) == (S, D, I), name
    assert tiny >= 400 and small >= 450
    assert known["AC / CA"] == (2, 1) and counts(2, 2, 2, 1) == (0, 1, 1)          # not two substitutions
    assert hs.edit_classes(b"", b"ACGT") == (4, 0) and hs.edit_classes(b"ACGT", b"") == (4, 0) and hs.edit_classes(b"", b"") == (0, 0)
    assert hs.edit_classes("ACGT", np.frombuffer(b"AGT", np.uint8)) == (1, 3)
    assert hs.edit_classes(b"NNNN", b"NNNN") == (4, 0) and hs.edit_classes(b"acgt", b"acgt") == (4, 0)


def test_edit_classes_on_random_pairs():
    rng = np.random.default_rng(6)
    alphabet = np.frombuffer(b"ACGTNa", np.uint8)
    for k in range(300):
        m, n = int(rng.integers(0, 120)), int(rng.integers(0, 120))
        t = alphabet[rng.integers(0, 6, m)].tobytes()
        s = mutate(rng, t, 0.2) if k % 2 else alphabet[rng.integers(0, 6, n)].tobytes()
        got = hs.edit_classes(t, s)
        assert got == loop_classes(t, s) == diagonal_classes(t, s) and got[0] == loop_distance(t, s), (t, s)


@pytest.mark.parametrize("T_", [1, 2, 11, 32])
def test_read_error_classes_on_report_case_inputs(T_):
    c = report_case(T=T_)
    seq, _, off = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], None, T_)
    rng = np.random.default_rng(T_)
    R = len(c["ev_len"])
    without = (1, R - 2)
    truth, toff = truth_for_reads(rng, seq, off, 0.1, without)
    ec = hs.read_error_classes(c["bases"], c["ev_len"], seq, off, truth, toff)
    acc = hs.read_accuracy(c["bases"], c["ev_len"], seq, off, truth, toff)
    assert ec.dtype == np.uint64 and ec.shape == (R, 6) == (R, hs.ERRCLASS_COLS)
    assert np.array_equal(ec[:, [0, 1, 3]], acc[:, :3]) and not ec[:, 5].any()
    ev_off = np.cumsum(c["ev_len"]) - c["ev_len"]
    some = 0
    for r in range(R):
        t = truth[toff[r]:toff[r + 1]].tobytes()
        if not t:
            assert not ec[r].any()
            continue
        b, s = c["bases"][ev_off[r]:ev_off[r] + c["ev_len"][r]].tobytes(), seq[off[r]:off[r + 1]].tobytes()
        assert ec[r].tolist() == [len(t), *diagonal_classes(t, b), *diagonal_classes(t, s), 0], r
        some += ec[r, 2] != ec[r, 4]
    assert not ec[list(without)].any() and (T_ > 2 or some >= 3)
    with pytest.raises(ValueError):
        hs.read_error_classes(c["bases"], c["ev_len"], seq, off[:-1], truth, toff)


# ---- form 31 ----------------------------------------------------------------------------------------------------------------------
def test_form_31_marshals_the_block_last():
    from nanoreviser_amd import engine
    from nanoreviser_amd.engine import Reviser
    assert 31 not in engine._RAW_FORMS and max(engine._RAW_FORMS) == 27 and set(engine._RAW_FORMS_TRUTH) == {30, 31}
    assert engine.ERRCLASS_COLS == hs.ERRCLASS_COLS == 6 and engine.ERRCLASS_R >= 1
    assert {"nrv_revise_reads_raw_errclass_begin", "nrv_revise_reads_raw_errclass", "nrv_merge_calls_errclass",
            "nrv_edit_classes"} <= set(engine.SYMBOLS)
    p12 = _packed12()
    truth, toff = np.frombuffer(b"ACGTAC", np.uint8), np.array([0, 4, 6], np.int64)
    rv = Reviser.__new__(Reviser)
    rv._lib, rv._h = _Recorder(), C.c_void_p(0)
    addr = lambda x: C.cast(x, C.c_void_p).value
    for base in (p12, Reviser.with_device_trim(Reviser.with_device_profile(Reviser.with_device_records(
            Reviser.with_device_edits(Reviser.with_device_report(p12, 0.25)), [b"a", b"bc"], hand_back=False)), 3, 4, 50)):
        p30 = Reviser.with_device_accuracy(base, truth, toff)
        p = Reviser.with_device_error_classes(p30)
        assert len(p) == 31 and all(p[k] is p30[k] for k in range(30))
        assert p[30].shape == (2, 6) and p[30].dtype == np.uint64
        del rv._lib.calls[:]
        t = rv.begin_packed_raw(p)
        (name, args), = rv._lib.calls
        assert name == "nrv_revise_reads_raw_errclass_begin" and len(args) == 31 + 3 + 1
        assert addr(args[32]) == p[29].ctypes.data and addr(args[33]) == p[30].ctypes.data and addr(args[30]) == p[27].ctypes.data
        assert len(t) == 3 and len(t[1]) == 12 and t[1][11] is p[30] and t[1][10] is p[29]      # the block is the last output
        out = rv.run_packed_raw(p)
        assert rv._lib.calls[-1][0] == "nrv_revise_reads_raw_errclass" and len(rv._lib.calls[-1][1]) == 34
        assert len(out) == 12 and out[11] is p[30] and out[10] is p[29]
        assert (out[9] is None) == (len(base) < 27) and (out[6] is None) == (len(base) < 20)
        assert len(cli._host_merge_form(p)) == 7
    for bad in (p12, p30[:27], p):
        with pytest.raises(ValueError):
            Reviser.with_device_error_classes(bad)
    with pytest.raises(ValueError, match="27 or 30 elements"):
        rv.run_packed_raw(p + (None,))
    # a library without the entry points: found by presence
    rv._lib = _Recorder(without=("errclass", "edit_classes"))
    with pytest.raises(engine.NrvError):
        rv.begin_packed_raw(p)
    rv.begin_packed_raw(p30)                                             # ... and the form 30 call still goes through
    assert rv._lib.calls[-1][0] == "nrv_revise_reads_raw_accuracy_begin"
    with pytest.raises(engine.NrvError):
        rv.edit_classes_device([b"A"], [b"A"])
    with pytest.raises(engine.NrvError):
        rv.edit_classes_offsets(b"A", [0, 1], b"A", [0, 1])
    with pytest.raises(engine.NrvError):
        rv.merge_calls_errclass_device(np.frombuffer(b"ACGT", np.uint8), [4], [], [], b"", [0, 0])
    rv._lib = _Recorder()
    d, M = rv.edit_classes_device([b"ACG", b""], [b"A", b"CC"])
    (name, args), = rv._lib.calls
    assert name == "nrv_edit_classes" and len(args) == 8 and args[5] == 2 and d.shape == M.shape == (2,)
    rv._h = None


def test_route_batch_with_error_classes():
    class Full:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = with_device_trim = with_device_accuracy = with_device_error_classes = None

    class NoClasses:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = with_device_trim = with_device_accuracy = None

    class NoAccuracy:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = with_device_trim = with_device_error_classes = None
    bundle = {"bases": np.zeros(5, "S1"), "meta": np.array([[0, 5, 0, 0]])}
    route = lambda rv, dm, **kw: cli._route_batch(rv, bundle, 1, True, True, dm, False, **kw)
    assert route(Full, True, accuracy=True, error_classes=True) == (31, "pipelined")
    assert route(Full, True, accuracy=True, error_classes=True, trim=True, combined=True, summary=True, edits=True) == (31, "pipelined")
    assert cli._route_batch(Full, bundle, 1, False, True, True, True, accuracy=True, error_classes=True) == (31, "packed+finish_bundle")
    assert route(NoClasses, True, accuracy=True, error_classes=True) == ("host-merge", "pipelined")
    assert route(NoAccuracy, True, accuracy=True, error_classes=True) == ("host-merge", "pipelined")
    # the switch off: the existing answers, form 30 among them
    assert route(Full, True, accuracy=True) == (30, "pipelined") and route(NoClasses, True, accuracy=True) == (30, "pipelined")
    assert route(Full, True) == (12, "pipelined") and route(Full, True, trim=True) == (27, "pipelined")
    assert route(Full, False, accuracy=True, error_classes=True) == (7, "pipelined")
    doc = cli._route_batch.__doc__
    assert "30 [9]" in doc and "[9] " in doc and "31 [10]" in doc and "[10] " in doc


# ---- the switch --------------------------------------------------------------------------------------------------------------------
def test_error_classes_flag_parsing(monkeypatch, capsys):
    for k in ("NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES", "NRV_TRIM_Q"):
        monkeypatch.delenv(k, raising=False)
    base = ["-d", "x", "-o", "y"]
    both = ["--truth", "t.fa", "--accuracy", "a.tsv"]
    assert cli.get_args(base).error_classes is None and cli.get_args(base + both).error_classes is None
    a = cli.get_args(base + both + ["--error_classes", "e.tsv", "--accuracy_max_len", "9000"])
    assert (a.truth, a.accuracy, a.error_classes, a.accuracy_max_len) == ("t.fa", "a.tsv", "e.tsv", 9000)
    monkeypatch.setenv("NRV_ERROR_CLASSES", "env.tsv")
    assert cli.get_args(base + both).error_classes == "env.tsv"
    assert cli.get_args(base + both + ["--error_classes", "e.tsv"]).error_classes == "e.tsv"
    with pytest.raises(SystemExit) as e:                                  # the environment's switch is refused alone as well
        cli.get_args(base)
    assert e.value.code == 2 and "--error_classes goes with --truth and --accuracy" in capsys.readouterr().err
    monkeypatch.delenv("NRV_ERROR_CLASSES")
    with pytest.raises(SystemExit) as e:
        cli.get_args(base + ["--error_classes", "e.tsv"])
    assert e.value.code == 2 and "--error_classes goes with --truth and --accuracy" in capsys.readouterr().err
    # the refusals that were there stay as they are, with their own messages
    for bad, msg in ((["--truth", "t.fa", "--error_classes", "e.tsv"], "--truth and --accuracy go together"),
                     (["--accuracy", "a.tsv", "--error_classes", "e.tsv"], "--truth and --accuracy go together"),
                     (both + ["--error_classes", "e.tsv", "--resume"], "--resume cannot be used with --accuracy")):
        with pytest.raises(SystemExit) as e:
            cli.get_args(base + bad)
        err = capsys.readouterr().err
        assert e.value.code == 2 and msg in err and "--error_classes goes with" not in err, bad


def test_line_and_total_format():
    assert cli.ERRCLASS_HEADER.split("\t") == ["name", "status", "truth_len", "len_in", "match_in", "sub_in", "ins_in", "del_in",
                                              "len_out", "match_out", "sub_out", "ins_out", "del_out"]
    # truth 100; original 97 long, d = 12, M = 90: S = 100 + 97 - 180 - 12 = 5, I = 12 - 10 = 2, D = 12 - 7 = 5
    #            revised 101 long, d = 3, M = 99: S = 0, I = 2, D = 1
    v = [100, 97, 12, 90, 101, 3, 99, cli.ACC_WITH_TRUTH]
    assert cli.error_class_fields(v) == ["100", "97", "90", "5", "2", "5", "101", "99", "0", "2", "1"]
    assert cli.error_class_fields(v, rates=True)[11:] == ["0.050000", "0.020000", "0.050000", "0.000000", "0.020000", "0.010000"]
    assert cli.error_class_fields([300, 1, 2, 3, 4, 5, 6, cli.ACC_WITH_TRUTH], rates=True)[11] == f"{(300 + 1 - 6 - 2) / 300:.6f}"
    for flag in (cli.ACC_NO_TRUTH, cli.ACC_TOO_LONG):
        assert cli.error_class_fields([0, 97, 0, 0, 101, 0, 0, flag]) == ["0"] + ["."] * 10
    assert cli.error_class_fields([0] * 7 + [cli.ACC_WITH_TRUTH], rates=True)[11:] == ["0.000000"] * 6   # no read with a truth
    for m, n, d, M in ((2, 2, 2, 1), (7, 3, 5, 2), (3, 7, 4, 3)):
        f = cli.error_class_fields([m, n, d, M, n, d, M, 0])
        assert [int(x) for x in f[3:6]] == list(counts(m, n, d, M)) and f[1:6] == f[6:11]
    rows = cli.ErrclassPart.rows(np.array([[100, 12, 90, 3, 99, 0], [0] * 6, [5, 1, 4, 1, 4, 0]], np.uint64), [97, 8, 5], [101, 9, 5],
                                 [cli.ACC_WITH_TRUTH, cli.ACC_NO_TRUTH, cli.ACC_TOO_LONG])
    assert rows == [v, [0, 8, 0, 0, 9, 0, 0, cli.ACC_NO_TRUTH], [0, 5, 0, 0, 5, 0, 0, cli.ACC_TOO_LONG]]


# ---- the command line on stand-in engines ----------------------------------------------------------------------------------------
class ClassesHash(AccuracyHash):
    """AccuracyHash with form 31: the error-class block by the host definition from the same calls."""
    with_device_error_classes = staticmethod(lambda *a, **k: AccuracyHash._cls().with_device_error_classes(*a, **k))

    def begin_packed_raw(self, packed):
        if len(packed) != 31:
            return super().begin_packed_raw(packed)
        t, outs, merged = super().begin_packed_raw(tuple(packed[:30]))
        self.forms[-1] = 31
        _, _, a1, a2 = HashEngine.predict_read(self, None, packed[2])
        el = [int(d.ev_len) for d in packed[3]]
        seq, _, off = hs.emit_calls(packed[9], el, a1, a2, None, self.T)
        return t, outs + (hs.read_error_classes(packed[9], el, seq, off, packed[27], packed[28]),), merged


_CLASSES = {}


def _expected_classes():
    """`test_accuracy_host._expected` with (d, M) of the original and of the revised read by `diagonal_classes`, once per process."""
    if not _CLASSES:
        for k, (orig, seq, truth, d_in, d_out) in _expected().items():
            c_in, c_out = diagonal_classes(truth, orig), diagonal_classes(truth, seq)
            assert c_in[0] == d_in and c_out[0] == d_out
            _CLASSES[k] = (orig, seq, truth, c_in, c_out)
    return _CLASSES


def _want_tsv(names, leave_out=(), too_long=(), unrevised=()):
    exp = _expected_classes()
    lines, tot, n_reads = [cli.ERRCLASS_HEADER], np.zeros(11, np.int64), [0, 0, 0]
    for i, fn in enumerate(sorted(names)):
        orig, seq, truth, c_in, c_out = exp[i % 2]
        status = "unrevised" if fn in unrevised else "revised"
        if fn in leave_out or fn in too_long:
            lines.append(f"{fn}\t{status}\t0" + "\t." * 10)
            n_reads[2 if fn in too_long else 1] += 1
            continue
        m = len(truth)
        if fn in unrevised:
            seq, c_out = orig, c_in
        v = [m, len(orig), c_in[1], *counts(m, len(orig), *c_in), len(seq), c_out[1], *counts(m, len(seq), *c_out)]
        lines.append(f"{fn}\t{status}\t" + "\t".join(str(x) for x in v))
        tot += v
        n_reads[0] += 1
    rates = [f"{int(tot[k]) / int(tot[0]):.6f}" for k in (3, 4, 5, 8, 9, 10)]
    lines.append("#total\twith_truth\t" + "\t".join(str(int(x)) for x in tot) + "\t" + "\t".join(rates))
    lines.append("#reads\t" + "\t".join(str(x) for x in n_reads))
    return ("\n".join(lines) + "\n").encode()


def _memoised(monkeypatch):
    """hoststage.edit_classes behind a table keyed by the pair: the routes below ask for the same few long pairs again and again."""
    real, table = hs.edit_classes, {}

    def edit_classes(truth, seq):
        key = (bytes(hs._as_u8(truth)), bytes(hs._as_u8(seq)))
        if key not in table:
            table[key] = real(truth, seq)
        return table[key]
    monkeypatch.setattr(hs, "edit_classes", edit_classes)
    return table


def test_error_classes_file_is_the_same_on_every_route(tmp_path, monkeypatch, capsys):
    import __graft_entry__ as g
    from nanoreviser_amd import hostlib
    g.build_host()
    _clean_env(monkeypatch)
    monkeypatch.delenv("NRV_ERROR_CLASSES", raising=False)
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib, "_lib", None)
    assert hostlib.load() is not None
    table = _memoised(monkeypatch)
    exp = _expected_classes()
    for orig, seq, truth, c_in, c_out in exp.values():                     # the revision moved the classes, not only the distance
        assert counts(len(truth), len(orig), *c_in) != counts(len(truth), len(seq), *c_out) and c_out[0] > 0
    src = _many(tmp_path, 6)
    names = sorted(os.listdir(src))
    leave_out = (names[1], names[4])
    fa = _write_truth(str(tmp_path / "truth.fa"), names, leave_out)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                           # several device calls for these reads
    want = _want_tsv(names, leave_out)

    def run(tag, extra=(), classes=True, **kw):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "--batch", "1024", "--truth", fa, "--accuracy", out + "acc.tsv"] + list(extra)
        if classes:
            argv += ["--error_classes", out + "ecl.tsv"]
        assert cli.main(argv, **kw) == 0
        assert not [f for f in os.listdir(out) if ".part" in f or ".tmp" in f]
        return out

    eng_0 = ClassesHash()
    plain = _files(run("plain", ["--device_merge"], classes=False, reviser_factory=lambda a, dev: eng_0))
    assert "ecl.tsv" not in plain and set(eng_0.forms) == {30} and not table        # the switch off: form 30, as it was
    eng_p = ClassesHash()
    capsys.readouterr()
    piped = run("piped", reviser_factory=lambda a, dev: eng_p)
    assert capsys.readouterr().out.count("--error_classes: the error classes are computed by the host stage") == 1
    eng_m = ClassesHash()
    merged = run("merged", ["--device_merge"], reviser_factory=lambda a, dev: eng_m)
    assert "--error_classes: the error classes are computed" not in capsys.readouterr().out
    assert set(eng_p.forms) == {7} and set(eng_m.forms) == {31} and len(eng_m.forms) >= 2
    eng_t = ClassesHash()
    trimmed = run("trimmed", ["--device_merge", "--trim_q", "3", "--report", str(tmp_path / "t.rep")], reviser_factory=lambda a, dev: eng_t)
    assert set(eng_t.forms) == {31}
    seq_run = run("seq", ["--thread", "1"], reviser_factory=lambda a, dev: HashEngine())
    for o in (piped, merged, seq_run):
        f = _files(o)
        assert f.pop("ecl.tsv") == want, o
        assert f == plain, o                                            # every other output, acc.tsv included, is that of a run without it
    assert _files(trimmed)["ecl.tsv"] == want                          # the classes describe the untrimmed revision
    # an engine with the accuracy call and without this one: the host merge, the same file
    eng_o = AccuracyHash()
    old = run("old", ["--device_merge"], reviser_factory=lambda a, dev: eng_o)
    assert set(eng_o.forms) == {7} and _files(old)["ecl.tsv"] == want
    # --accuracy_max_len is shared: the longer kind has no truth in either file
    lens = [max(len(exp[k][0]), len(exp[k][2])) for k in (0, 1)]
    long_kind = int(np.argmax(lens))
    too_long = [fn for i, fn in enumerate(names) if i % 2 == long_kind and fn not in leave_out]
    want_cut = _want_tsv(names, leave_out, too_long)
    for tag, extra in (("cut_host", []), ("cut_dev", ["--device_merge"])):
        f = _files(run(tag, extra + ["--accuracy_max_len", str(min(lens))], reviser_factory=lambda a, dev: ClassesHash()))
        assert f["ecl.tsv"] == want_cut, tag
        assert f["ecl.tsv"].decode().split("\n")[-2] == f["acc.tsv"].decode().split("\n")[-2] == f"#reads\t{6 - 2 - len(too_long)}\t2\t{len(too_long)}"


def test_error_classes_file_is_the_same_for_1_and_2_workers(tmp_path, monkeypatch):
    _clean_env(monkeypatch)
    monkeypatch.delenv("NRV_ERROR_CLASSES", raising=False)
    src = _many(tmp_path, 4)
    names = sorted(os.listdir(src))
    fa = _write_truth(str(tmp_path / "truth.fa"), names, (names[2],))
    outs = {}
    for world in (1, 2):
        out = str(tmp_path / f"w{world}") + "/"
        assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "--truth", fa, "--accuracy", out + "acc.tsv",
                         "--error_classes", out + "ecl.tsv"], worker_factory=hash_factory, world=world) == 0
        outs[world] = _files(out)
    assert outs[1]["ecl.tsv"] == _want_tsv(names, (names[2],)) and outs[2] == outs[1]


def test_an_unrevised_read_has_the_classes_of_what_was_written(tmp_path, monkeypatch):
    _clean_env(monkeypatch)
    monkeypatch.delenv("NRV_ERROR_CLASSES", raising=False)
    _memoised(monkeypatch)
    src = _many(tmp_path, 4)
    names = sorted(os.listdir(src))
    _, rdA, rtA = load_read("_".join(os.path.basename(FAST5[0]).split("_")[-3:-1]))
    fa = _write_truth(str(tmp_path / "truth.fa"), names)
    out = str(tmp_path / "o") + "/"
    eng = EchoEngine(fail_marker=rtA.feat_ev[0])                        # every call that STARTS with a read A fails
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "-e", "bad.txt", "--truth", fa, "--accuracy", out + "acc.tsv",
                     "--error_classes", out + "ecl.tsv"], reviser_factory=lambda a, dev: eng) == 0
    failed = set(open(out + "bad.txt").read().split())
    assert failed and "r00_A.fast5" in failed
    # the echo engine writes the original read back: revised or not, out = in
    want = _want_tsv(names, unrevised=names).decode().split("\n")
    got = open(out + "ecl.tsv").read().split("\n")
    assert [ln.split("\t")[1] for ln in got[1:5]] == ["unrevised" if fn in failed else "revised" for fn in names]
    assert [ln.split("\t")[:1] + ln.split("\t")[2:] for ln in got[1:5]] == [ln.split("\t")[:1] + ln.split("\t")[2:] for ln in want[1:5]]
    assert got[5:] == want[5:] and got[0] == want[0]
