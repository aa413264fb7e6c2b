"""Edit distance to a truth set on the host (no GPU): hoststage.edit_distance against two references that share no code with it,
hoststage.read_accuracy, the packed form 30, the routing table, the --truth loader and the command line's --truth / --accuracy
on stand-in engines on every host route.  Integers and bytes only: nothing here has a tolerance."""
import ctypes as C
import glob
import os
import shutil

import numpy as np
import pytest

from accuracy_cases import SMALL, loop_distance, mutate, planted_cases, reference, row_distance, truth_for_reads
from conftest import GOLD, load_read
from echo_engine import EchoEngine, HashEngine, PipelinedEcho, hash_factory
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from report_cases import report_case

T = 11
FAST5 = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")))


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def test_edit_distance_equals_both_references_on_every_planted_pair():
    cases, known = planted_cases()
    ref = reference()
    assert len(cases) > 400 and sum(len(t) >= 4095 for t, _ in cases.values()) <= 24
    for name, (t, s) in cases.items():
        got = hs.edit_distance(t, s)
        assert got == ref[name], name
        if len(t) <= SMALL and len(s) <= SMALL:
            assert got == loop_distance(t, s), name
        if name in known:
            assert got == known[name], name
    # the known answers are there: 0, m, max(m, n), the chunk length
    for m in (1, 64, 65, 4096, 4097, 8193):
        assert known[f"m={m} itself*"] == 0 and known[f"m={m} empty*"] == m
    assert known["m=129 A against C"] == 134 and known["m=129 C against longer A"] == 129
    assert known["m=4160 G x 64 removed at 4096"] == 64 and known["m=4160 G x 100 inserted at 2000"] == 100
    # an empty truth is no truth to read_accuracy; the bare distance is D[0][n] = n; arrays and str work like bytes
    assert hs.edit_distance(b"", b"ACGT") == 4 and hs.edit_distance(b"", b"") == 0
    assert hs.edit_distance("ACGT", np.frombuffer(b"AGT", np.uint8)) == 1
    assert hs.edit_distance(b"NNNN", b"NNNN") == 4 and hs.edit_distance(b"acgt", b"acgt") == 4


def test_edit_distance_on_random_pairs():
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b"ACGTNa", np.uint8)
    for _ in range(300):
        m, n = int(rng.integers(0, 200)), int(rng.integers(0, 200))
        t, s = alphabet[rng.integers(0, 6, m)].tobytes(), alphabet[rng.integers(0, 6, n)].tobytes()
        assert hs.edit_distance(t, s) == loop_distance(t, s) == row_distance(t, s), (t, s)


@pytest.mark.parametrize("T_", [1, 2, 11, 32])
def test_read_accuracy_on_report_case_inputs(T_):
    c = report_case(T=T_)
    seq, _, off = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], None, T_)
    rng = np.random.default_rng(T_)
    R = len(c["ev_len"])
    without = (1, R - 2)
    truth, toff = truth_for_reads(rng, seq, off, 0.1, without)
    acc = hs.read_accuracy(c["bases"], c["ev_len"], seq, off, truth, toff)
    assert acc.dtype == np.uint64 and acc.shape == (R, 4)
    ev_off = np.cumsum(c["ev_len"]) - c["ev_len"]
    some = 0
    for r in range(R):
        t = truth[toff[r]:toff[r + 1]].tobytes()
        if not t:
            assert not acc[r].any()
            continue
        b, s = c["bases"][ev_off[r]:ev_off[r] + c["ev_len"][r]].tobytes(), seq[off[r]:off[r + 1]].tobytes()
        assert acc[r].tolist() == [len(t), row_distance(t, b), row_distance(t, s), 0], r
        some += acc[r, 1] != acc[r, 2]
    assert not acc[list(without)].any() and (T_ > 2 or some >= 3)
    with pytest.raises(ValueError):
        hs.read_accuracy(c["bases"], c["ev_len"], seq, off[:-1], truth, toff)


# ---- form 30 ----------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """A stand-in for libnanorev_hip.so that records the calls it gets."""

    def __init__(self, without=()):
        self.calls, self.without = [], without

    def __getattr__(self, name):
        if not name.startswith("nrv_") or any(w in name for w in self.without):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


def _packed12(fastq=True, N=30):
    from nanoreviser_amd.engine import Reviser
    ev = [N - N // 2, N // 2]
    raw = np.zeros(N * 4, np.int16)
    starts = np.concatenate([np.arange(e, dtype=np.int32) * 4 for e in ev])
    p = Reviser.pack_reads_raw([raw[:ev[0] * 4], raw[:ev[1] * 4]], [starts[:ev[0]], starts[ev[0]:]],
                               [np.zeros((e, 6), np.float32) for e in ev], [0.0, 0.0], [1.0, 1.0], T)
    return Reviser.with_device_merge(p, np.frombuffer(b"ACGT" * N, np.uint8)[:N], fastq)


def test_form_30_marshals_the_truth_behind_every_other_block():
    from nanoreviser_amd import engine
    from nanoreviser_amd.engine import Reviser
    assert 30 not in engine._RAW_FORMS and 30 in engine._RAW_FORMS_TRUTH and engine.ACCURACY_COLS == hs.ACCURACY_COLS == 4
    assert {"nrv_revise_reads_raw_accuracy_begin", "nrv_revise_reads_raw_accuracy", "nrv_merge_calls_accuracy",
            "nrv_edit_distance"} <= set(engine.SYMBOLS)
    p12 = _packed12()
    p14 = Reviser.with_device_report(p12, 0.25)
    p16 = Reviser.with_device_edits(p14)
    p20 = Reviser.with_device_records(p16, [b"a", b"bc"], hand_back=False)
    p22 = Reviser.with_device_profile(p20)
    p27 = Reviser.with_device_trim(p22, 3, 4, 50)
    truth, toff = np.frombuffer(b"ACGTAC", np.uint8), np.array([0, 4, 6], np.int64)
    rv = Reviser.__new__(Reviser)
    rv._lib, rv._h = _Recorder(), C.c_void_p(0)
    addr = lambda x: C.cast(x, C.c_void_p).value
    for base in (p12, p14, p16, p20, p22, p27):
        p = Reviser.with_device_accuracy(base, truth, toff)
        assert len(p) == 30 and all(p[k] is base[k] for k in range(len(base)) if k != 12)
        assert all(p[k] is None for k in range(max(len(base), 13), 22))                # blocks not carried: "not asked for"
        if len(base) < 27:
            assert p[22] is None and p[23:26] == (0, 0, 0) and p[26] is None           # ... a NULL trim included
        assert p[27].tobytes() == b"ACGTAC" and p[28].tolist() == [0, 4, 6] and p[28].dtype == np.int64
        assert p[29].shape == (2, 4) and p[29].dtype == np.uint64
        del rv._lib.calls[:]
        t = rv.begin_packed_raw(p)
        (name, args), = rv._lib.calls
        assert name == "nrv_revise_reads_raw_accuracy_begin" and len(args) == 30 + 3 + 1
        assert addr(args[30]) == p[27].ctypes.data and addr(args[31]) == p[28].ctypes.data and addr(args[32]) == p[29].ctypes.data
        assert (args[29] is None) == (len(base) < 27) and (args[25] is None) == (len(base) < 27)
        assert (args[23] is None) == (len(base) < 22) and (args[22] is None) == (len(base) < 20)
        assert len(t) == 3 and len(t[1]) == 11 and t[1][10] is p[29]                   # accuracy is the last output
        out = rv.run_packed_raw(p)
        assert rv._lib.calls[-1][0] == "nrv_revise_reads_raw_accuracy" and len(rv._lib.calls[-1][1]) == 33
        assert len(out) == 11 and out[10] is p[29]
        assert (out[9] is None) == (len(base) < 27) and (out[8] is None) == (len(base) < 22) and (out[6] is None) == (len(base) < 20)
        assert len(cli._host_merge_form(p)) == 7
    for bad_off in ([0, 4], [1, 4, 6], [0, 5, 4], [0, 4, 7]):
        with pytest.raises(ValueError):
            Reviser.with_device_accuracy(p12, truth, bad_off)
    with pytest.raises(ValueError):
        Reviser.with_device_accuracy(tuple(p12[:9]), truth, toff)
    with pytest.raises(ValueError, match="27 or 30 elements"):
        rv.run_packed_raw(p12 + (None,))
    # an empty truth set still hands a pointer over
    assert Reviser.with_device_accuracy(p12, b"", [0, 0, 0])[27].size == 1
    # a library without the entry points: found by presence
    rv._lib = _Recorder(without=("accuracy", "edit_distance"))
    with pytest.raises(engine.NrvError):
        rv.begin_packed_raw(Reviser.with_device_accuracy(p12, truth, toff))
    with pytest.raises(engine.NrvError):
        rv.edit_distance_device([b"A"], [b"A"])
    with pytest.raises(engine.NrvError):
        rv.merge_calls_accuracy_device(np.frombuffer(b"ACGT", np.uint8), [4], [], [], b"", [0, 0])
    rv._lib = _Recorder()
    d = rv.edit_distance_device([b"ACG", b""], [b"A", b"CC"])
    (name, args), = rv._lib.calls
    assert name == "nrv_edit_distance" and len(args) == 7 and args[5] == 2 and d.shape == (2,)
    rv._h = None


def test_route_batch_with_accuracy():
    class Full:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = with_device_trim = with_device_accuracy = None

    class NoAccuracy:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = with_device_trim = None

    class NoTrim:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = with_device_accuracy = None
    bundle = {"bases": np.zeros(5, "S1"), "meta": np.array([[0, 5, 0, 0]])}
    route = lambda rv, dm, **kw: cli._route_batch(rv, bundle, 1, True, True, dm, False, **kw)
    assert route(Full, True, accuracy=True) == (30, "pipelined")
    assert route(Full, True, accuracy=True, trim=True, combined=True, summary=True, edits=True) == (30, "pipelined")
    assert cli._route_batch(Full, bundle, 1, True, True, True, True, accuracy=True) == (30, "pipelined")
    assert cli._route_batch(Full, bundle, 1, False, True, True, True, accuracy=True) == (30, "packed+finish_bundle")
    assert route(NoAccuracy, True, accuracy=True) == ("host-merge", "pipelined")
    assert route(NoTrim, True, accuracy=True, trim=True) == ("host-merge", "pipelined") and route(NoTrim, True, accuracy=True) == (30, "pipelined")
    # without the switch, or without --device_merge, nothing moves
    assert route(Full, True) == (12, "pipelined") and route(Full, True, trim=True) == (27, "pipelined")
    assert route(Full, False, accuracy=True) == (7, "pipelined")
    assert "30 [9]" in cli._route_batch.__doc__ and "[9] " in cli._route_batch.__doc__


# ---- the switches and the loader -------------------------------------------------------------------------------------------------
def test_accuracy_flag_parsing(monkeypatch, capsys):
    for k in ("NRV_TRUTH", "NRV_ACCURACY", "NRV_TRIM_Q"):
        monkeypatch.delenv(k, raising=False)
    base = ["-d", "x", "-o", "y"]
    a = cli.get_args(base)
    assert a.truth is None and a.accuracy is None and a.accuracy_max_len == 65536
    a = cli.get_args(base + ["--truth", "t.fa", "--accuracy", "a.tsv", "--accuracy_max_len", "9000"])
    assert (a.truth, a.accuracy, a.accuracy_max_len) == ("t.fa", "a.tsv", 9000)
    monkeypatch.setenv("NRV_TRUTH", "env.fa")
    monkeypatch.setenv("NRV_ACCURACY", "env.tsv")
    a = cli.get_args(base)
    assert (a.truth, a.accuracy) == ("env.fa", "env.tsv") and cli.get_args(base + ["--truth", "t.fa"]).truth == "t.fa"
    monkeypatch.delenv("NRV_TRUTH")
    monkeypatch.delenv("NRV_ACCURACY")
    for bad in (["--truth", "t.fa"], ["--accuracy", "a.tsv"], ["--truth", "t.fa", "--accuracy", "a.tsv", "--resume"],
                ["--truth", "t.fa", "--accuracy", "a.tsv", "--accuracy_max_len", "-1"]):
        with pytest.raises(SystemExit) as e:
            cli.get_args(base + bad)
        assert e.value.code == 2, bad
    err = capsys.readouterr().err
    assert "--truth and --accuracy go together" in err and "--resume cannot be used with --accuracy" in err


def test_truth_loader(tmp_path):
    fa = tmp_path / "t.fa"
    fa.write_text(">r1.fast5 some words\nACGT\nacgtnn\n\n>r2\tx\nAC\r\nGT\n>empty\n>r3\nA")
    t = cli.load_truth(str(fa))
    assert t == {"r1": b"ACGTACGTNN", "r2": b"ACGT", "empty": b"", "r3": b"A"}
    assert cli.truth_of(t, "r1.fast5") == b"ACGTACGTNN" and cli.truth_of(t, "r2.fast5") == b"ACGT" and cli.truth_of(t, "r2") == b"ACGT"
    assert cli.truth_of(t, "r4.fast5") is None and cli.truth_of(t, "r1") == b"ACGTACGTNN"
    for twice in (">r1\nAC\n>r2\nG\n>r1 again\nT\n", ">r1\nAC\n>r1.fast5\nT\n"):     # the same read, named with and without .fast5
        fa.write_text(twice)
        with pytest.raises(ValueError, match="r1 occurs twice"):
            cli.load_truth(str(fa))
    # max_len: the truth's or the original's length
    part = cli.AccuracyPart(None, {"a": b"ACGT", "b": b"ACGTACGT", "e": b""}, 6)
    truth, toff, flags = part.block(["a.fast5", "b.fast5", "c.fast5", "a.fast5", "e.fast5"], [5, 5, 5, 7, 5])
    assert flags == [cli.ACC_WITH_TRUTH, cli.ACC_TOO_LONG, cli.ACC_NO_TRUTH, cli.ACC_TOO_LONG, cli.ACC_NO_TRUTH]
    assert truth.tobytes() == b"ACGT" and toff.tolist() == [0, 4, 4, 4, 4, 4]


def test_identity_and_line_format():
    assert cli.identity_field(0, 10) == "1.000000" and cli.identity_field(1, 3) == "0.666667" and cli.identity_field(10, 10) == "0.000000"
    assert cli.identity_field(0, 0) == "1.000000"
    assert cli.accuracy_fields([100, 90, 12, 101, 3, 0]) == ["100", "90", "12", "101", "3", "0.880000", "0.970297"]
    assert cli.accuracy_fields([0, 90, 0, 101, 0, cli.ACC_NO_TRUTH]) == ["0"] + ["."] * 6
    assert cli.accuracy_fields([0, 90, 0, 101, 0, cli.ACC_TOO_LONG]) == ["0"] + ["."] * 6
    assert cli.ACCURACY_HEADER.split("\t") == ["name", "status", "truth_len", "len_in", "dist_in", "len_out", "dist_out", "id_in", "id_out"]


# ---- the command line on stand-in engines ----------------------------------------------------------------------------------------
class AccuracyHash(PipelinedEcho):
    """PipelinedEcho whose calls are HashEngine's (real revisions: insertions, deletions, substitutions) on every surface, with
    the merge forms of engine.Reviser, form 30 included: the blocks of a `with_device_*` tuple are filled by the host
    definitions from those calls, so the command line's --device_merge routes run without a device."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.forms = []

    @staticmethod
    def _cls():
        from nanoreviser_amd.engine import Reviser
        return Reviser

    with_device_merge = staticmethod(lambda *a, **k: AccuracyHash._cls().with_device_merge(*a, **k))
    with_device_report = staticmethod(lambda *a, **k: AccuracyHash._cls().with_device_report(*a, **k))
    with_device_edits = staticmethod(lambda *a, **k: AccuracyHash._cls().with_device_edits(*a, **k))
    with_device_records = staticmethod(lambda *a, **k: AccuracyHash._cls().with_device_records(*a, **k))
    with_device_profile = staticmethod(lambda *a, **k: AccuracyHash._cls().with_device_profile(*a, **k))
    with_device_trim = staticmethod(lambda *a, **k: AccuracyHash._cls().with_device_trim(*a, **k))
    with_device_accuracy = staticmethod(lambda *a, **k: AccuracyHash._cls().with_device_accuracy(*a, **k))

    def predict_read(self, sig_ev, feat_ev):
        return HashEngine.predict_read(self, sig_ev, feat_ev)

    def _hashed(self, packed, out):
        for dst, src in zip(out, HashEngine.predict_read(self, None, packed[2])):
            dst[...] = src
        return out

    def run_packed_raw(self, packed):
        return self._hashed(packed, super().run_packed_raw(packed))

    def begin_packed_raw(self, packed):
        self.forms.append(len(packed))
        if len(packed) <= 9:
            t, out = super().begin_packed_raw(packed)
            return t, self._hashed(packed, out)
        p = tuple(packed) + (None,) * (30 - len(packed))
        t, out = super().begin_packed_raw(tuple(p[:7]))
        p1, p2, a1, a2 = self._hashed(p, out)
        el = [int(d.ev_len) for d in p[3]]
        fastq = p[10] is not None
        qc = (cli.phred_chars(p1, p2, a1, a2) if len(a1) else np.zeros(0, np.uint8)) if fastq else None
        seq, qual, off = hs.emit_calls(p[9], el, a1, a2, qc, self.T)
        rep = hs.revision_report(p[9], el, a1, a2, p1, p2, qc, self.T, p[12]) if p[13] is not None else None
        ed, eoff = hs.revision_edits(p[9], el, a1, a2, p1, p2, qc, self.T) if p[15] is not None else (None, None)
        trim = cli.trim_rows(self.T, p[9], el, p1, p2, a1, a2, p[23], p[24]) if p[26] is not None else None
        blob, roff = (None, None)
        if p[19] is not None:
            names = [p[16][int(p[17][r]):int(p[17][r + 1])].tobytes() for r in range(len(el))]
            blob, roff = hs.pack_records(names, seq, qual, off, trim, p[25] if trim is not None else 1)
        prof = cli.profile_rows(self.T, p[9], el, p1, p2, a1, a2) if p[21] is not None else None
        acc = hs.read_accuracy(p[9], el, seq, off, p[27], p[28]) if p[29] is not None else None
        back = p[11][0] is not None
        outs = (seq if back else None, qual if back else None, off, rep, ed, eoff, blob, roff, prof, trim, acc)
        keep = {12: 3, 14: 4, 16: 6, 20: 8, 22: 9, 27: 10, 30: 11}[len(packed)]
        return t, outs[:keep], "merged"

    def end_packed_raw(self, ticket):
        out = super().end_packed_raw(ticket[:2])
        return ticket[1] if len(ticket) == 3 else out


def _many(tmp_path, copies):
    d = tmp_path / "in"
    d.mkdir()
    for i in range(copies):
        shutil.copy(FAST5[i % 2], d / f"r{i:02d}_{'AB'[i % 2]}.fast5")
    return str(d)


def _files(out):
    return {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}


_EXPECTED = {}


def _expected():
    """Per fixture read (A, B) of the hash engine: (original, revised, a truth = a seeded 5 % mutation of the revised read,
    d(truth, original), d(truth, revised)) - the distances by `row_distance`, once per process."""
    if not _EXPECTED:
        rng = np.random.default_rng(77)
        for k in (0, 1):
            _, rd, rt = load_read("_".join(os.path.basename(FAST5[k]).split("_")[-3:-1]))
            calls = HashEngine().predict_read(np.zeros((len(rt.feat_ev), 50), np.float32), rt.feat_ev)
            seq, _ = cli._finish_read(T, rt, *calls, want_qual=False)
            orig = b"".join(np.asarray(rd.bases).tolist())
            truth = mutate(rng, seq.encode(), 0.05)
            _EXPECTED[k] = (orig, seq.encode(), truth, row_distance(truth, orig), row_distance(truth, seq.encode()))
    return _EXPECTED


def _write_truth(path, names, leave_out=()):
    """A wrapped FASTA with mixed case, names with and without .fast5, a header with further words; `leave_out`: no record."""
    exp = _expected()
    with open(path, "w") as fp:
        for i, fn in enumerate(names):
            if fn in leave_out:
                continue
            t = exp[i % 2][2].decode()
            t = t.lower() if i % 3 == 0 else t
            fp.write(f">{fn if i % 2 else fn[:-6]} truth of read {i}\n" + "".join(t[k:k + 60] + "\n" for k in range(0, len(t), 60)))
    return path


def _want_tsv(names, leave_out=(), too_long=(), unrevised=()):
    exp = _expected()
    lines, tot, den, counts = [cli.ACCURACY_HEADER], [0] * 5, [0, 0], [0, 0, 0]
    for i, fn in enumerate(sorted(names)):
        orig, seq, truth, d_in, d_out = exp[i % 2]
        status = "unrevised" if fn in unrevised else "revised"
        if fn in leave_out or fn in too_long:
            lines.append(f"{fn}\t{status}\t0" + "\t." * 6)
            counts[2 if fn in too_long else 1] += 1
            continue
        v = [len(truth), len(orig), d_in, len(orig), d_in] if fn in unrevised else [len(truth), len(orig), d_in, len(seq), d_out]
        lines.append(f"{fn}\t{status}\t" + "\t".join(str(x) for x in v)
                     + f"\t{1 - v[2] / max(v[1], v[0]):.6f}\t{1 - v[4] / max(v[3], v[0]):.6f}")
        tot = [a + b for a, b in zip(tot, v)]
        den = [den[0] + max(v[1], v[0]), den[1] + max(v[3], v[0])]
        counts[0] += 1
    lines.append("#total\twith_truth\t" + "\t".join(str(x) for x in tot) + f"\t{1 - tot[2] / den[0]:.6f}\t{1 - tot[4] / den[1]:.6f}")
    lines.append("#reads\t" + "\t".join(str(x) for x in counts))
    return ("\n".join(lines) + "\n").encode()


def _clean_env(monkeypatch):
    for k in ("NRV_TRUTH", "NRV_ACCURACY", "NRV_SUMMARY", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_DEVICE_MERGE", "NRV_DEVICE_STATS",
              "NRV_CLI_PIPELINE", "NRV_HOST_LIB", "NRV_HOST_THREADS", "NRV_TRIM_Q"):
        monkeypatch.delenv(k, raising=False)


def test_accuracy_file_is_the_same_on_every_route(tmp_path, monkeypatch, capsys):
    import __graft_entry__ as g
    from nanoreviser_amd import hostlib
    g.build_host()
    _clean_env(monkeypatch)
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib, "_lib", None)
    assert hostlib.load() is not None
    exp = _expected()
    assert all(0 < d_out and d_in != d_out for _, _, _, d_in, d_out in exp.values())      # the revision moved the distance
    src = _many(tmp_path, 6)
    names = sorted(os.listdir(src))
    leave_out = (names[1], names[4])
    fa = _write_truth(str(tmp_path / "truth.fa"), names, leave_out)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                           # several device calls for these reads
    want = _want_tsv(names, leave_out)

    def run(tag, extra=(), accuracy=True, **kw):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "--batch", "1024"] + list(extra)
        if accuracy:
            argv += ["--truth", fa, "--accuracy", out + "acc.tsv"]
        assert cli.main(argv, **kw) == 0
        assert not [f for f in os.listdir(out) if ".part" in f or ".tmp" in f]
        return out

    plain = _files(run("plain", accuracy=False, reviser_factory=lambda a, dev: AccuracyHash()))
    assert "acc.tsv" not in plain
    eng_p = AccuracyHash()
    capsys.readouterr()
    piped = run("piped", reviser_factory=lambda a, dev: eng_p)
    assert capsys.readouterr().out.count("--accuracy: the edit distances are computed by the host stage") == 1
    eng_m = AccuracyHash()
    merged = run("merged", ["--device_merge"], reviser_factory=lambda a, dev: eng_m)
    assert "computed by the host stage" not in capsys.readouterr().out
    assert set(eng_p.forms) == {7} and set(eng_m.forms) == {30} and len(eng_m.forms) >= 2
    eng_t = AccuracyHash()
    trimmed = run("trimmed", ["--device_merge", "--trim_q", "3", "--report", str(tmp_path / "t.rep")], reviser_factory=lambda a, dev: eng_t)
    assert set(eng_t.forms) == {30}
    seq_run = run("seq", ["--thread", "1"], reviser_factory=lambda a, dev: HashEngine())
    for o in (piped, merged, seq_run):
        f = _files(o)
        assert f.pop("acc.tsv") == want, o
        assert f == plain, o                                            # every read output is that of a run without --truth
    assert _files(trimmed)["acc.tsv"] == want                          # dist_out describes the untrimmed revision
    # a library without the entry points: the host merge, the same file
    class Old(AccuracyHash):
        with_device_accuracy = property(lambda self: (_ for _ in ()).throw(AttributeError("with_device_accuracy")))
    eng_o = Old()
    old = run("old", ["--device_merge"], reviser_factory=lambda a, dev: eng_o)
    assert set(eng_o.forms) == {7} and _files(old)["acc.tsv"] == want
    # --accuracy_max_len between the two reads' lengths: the longer kind has no truth and is counted as too long
    lens = [max(len(exp[k][0]), len(exp[k][2])) for k in (0, 1)]
    long_kind = int(np.argmax(lens))
    assert min(lens) < max(lens)
    cut = ["--accuracy_max_len", str(min(lens))]
    too_long = [fn for i, fn in enumerate(names) if i % 2 == long_kind and fn not in leave_out]
    want_cut = _want_tsv(names, leave_out, too_long)
    for tag, extra in (("cut_host", []), ("cut_dev", ["--device_merge"])):
        assert _files(run(tag, extra + cut, reviser_factory=lambda a, dev: AccuracyHash()))["acc.tsv"] == want_cut, tag
    assert want_cut.decode().split("\n")[-2] == f"#reads\t{6 - 2 - len(too_long)}\t2\t{len(too_long)}"
    # a duplicate name is an error at start-up
    with open(fa, "a") as fp:
        fp.write(f">{names[0]}\nACGT\n")
    assert cli.main(["-d", src, "-o", str(tmp_path / "dup") + "/", "-S", "ecoli", "--truth", fa, "--accuracy", str(tmp_path / "dup.tsv")],
                    reviser_factory=lambda a, dev: AccuracyHash()) == 2
    assert not os.path.exists(str(tmp_path / "dup.tsv"))


def test_accuracy_file_is_the_same_for_1_and_2_workers(tmp_path, monkeypatch):
    _clean_env(monkeypatch)
    src = _many(tmp_path, 4)
    names = sorted(os.listdir(src))
    fa = _write_truth(str(tmp_path / "truth.fa"), names, (names[2],))
    outs = {}
    for world in (1, 2):
        out = str(tmp_path / f"w{world}") + "/"
        assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "--truth", fa, "--accuracy", out + "acc.tsv"],
                        worker_factory=hash_factory, world=world) == 0
        outs[world] = _files(out)
    assert outs[1]["acc.tsv"] == _want_tsv(names, (names[2],)) and outs[2] == outs[1]


def test_an_unrevised_read_has_the_distance_of_what_was_written(tmp_path, monkeypatch):
    _clean_env(monkeypatch)
    src = _many(tmp_path, 4)
    names = sorted(os.listdir(src))
    _, rdA, rtA = load_read("_".join(os.path.basename(FAST5[0]).split("_")[-3:-1]))
    fa = _write_truth(str(tmp_path / "truth.fa"), names)
    out = str(tmp_path / "o") + "/"
    eng = EchoEngine(fail_marker=rtA.feat_ev[0])                        # every call that STARTS with a read A fails
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "-e", "bad.txt", "--truth", fa, "--accuracy", out + "acc.tsv"],
                    reviser_factory=lambda a, dev: eng) == 0
    failed = set(open(out + "bad.txt").read().split())
    assert failed and "r00_A.fast5" in failed
    exp = _expected()
    lines = [ln.split("\t") for ln in open(out + "acc.tsv").read().split("\n")[1:-3]]
    assert [c[0] for c in lines] == names
    for i, c in enumerate(lines):
        orig, _, truth, d_in, _ = exp[i % 2]
        # the echo engine writes the original read back: revised or not, both distances are the original's
        assert c[1] == ("unrevised" if c[0] in failed else "revised")
        assert c[2:7] == [str(len(truth)), str(len(orig)), str(d_in), str(len(orig)), str(d_in)] and c[7] == c[8], c[0]
