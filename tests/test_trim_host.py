"""Sliding-window quality trimming and the length filter on the host (no GPU): hoststage.trim_bounds against a transcription of
the rule, hoststage.pack_records with a trim against slicing by hand, the packed form 27, the routing table, and the command
line's --trim_q / --trim_window / --min_len / --trim_log on stand-in engines on every host route.  Integers and bytes only:
nothing here has a tolerance."""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD, load_read
from echo_engine import EchoEngine, HashEngine, PipelinedEcho, hash_factory
from nanoreviser_amd import cli, hostlib
from nanoreviser_amd import hoststage as hs
from records_cases import loop_records, name_lengths_case, names_for, tiny_reads_case
from trim_cases import WINDOWS, loop_trim, loop_trimmed_records, planted_cases

T = 11
FAST5 = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")))


# ---- the definition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WINDOWS)
def test_trim_bounds_equals_the_rule_text_on_planted_inputs(W):
    for name, (qual, off, Q) in planted_cases(W).items():
        if name == "70000 in one read":                                # (the loop is quadratic in nothing, but 70 k x 64 is slow enough)
            qual, off = qual[:int(off[2])][:4000 + 5], np.array([0, 5, 4005], np.int64)
        got, want = hs.trim_bounds(qual, off, Q, W), loop_trim(qual, off, Q, W)
        assert got.dtype == np.int64 and got.shape == (len(off) - 1, 2) and np.array_equal(got, want), (W, name)
    c = planted_cases(W)
    L = 2 * 256 + 77
    assert hs.trim_bounds(*c["only window at 0"], W).tolist() == [[0, 0], [0, W], [0, 0]]
    assert hs.trim_bounds(*c["only window at L - W"], W).tolist() == [[0, 0], [L - W, L], [0, 0]]
    assert hs.trim_bounds(*c["only window across a tile edge"], W).tolist() == [[0, 0], [155, 155 + W], [0, 0]]
    assert not hs.trim_bounds(*c["lengths, all bad"][:2], 20, W).any()
    lens = np.diff(c["lengths, all 40"][1])
    assert np.array_equal(hs.trim_bounds(*c["lengths, all 40"][:2], 40, W), np.stack([0 * lens, np.where(lens >= W, lens, 0)], 1))
    assert hs.trim_bounds(*c["sum exactly Q W"][:2], 20, W).tolist() == [[7, 7 + W], [0, 0]]
    if W > 1:                                                           # the windows that reach into the next read do not count
        assert not hs.trim_bounds(*c["window reaching into the next read"], W).any()
        assert not hs.trim_bounds(*c["window reaching into the next read over a tile edge"], W).any()


def test_trim_bounds_equals_the_rule_text_on_random_inputs():
    rng = np.random.default_rng(17)
    for _ in range(60):
        R = int(rng.integers(1, 9))
        L = rng.integers(0, 90, R)
        off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
        qual = rng.integers(25, 33 + 42, int(off[-1])).astype(np.uint8)     # characters below '!' count as Phred 0
        Q, W = int(rng.integers(1, 41)), int(rng.integers(1, 65))
        assert np.array_equal(hs.trim_bounds(qual, off, Q, W), loop_trim(qual, off, Q, W)), (Q, W, L.tolist())
    for Q, W in ((0, 4), (41, 4), (3, 0), (3, 65)):
        with pytest.raises(ValueError):
            hs.trim_bounds(np.zeros(4, np.uint8), [0, 4], Q, W)


def _random_trim(off, rng, drop):
    L = np.diff(off)
    lo = (rng.random(L.size) * (L + 1)).astype(np.int64)
    hi = lo + (rng.random(L.size) * (L - lo + 1)).astype(np.int64)
    t = np.stack([lo, hi], 1)
    t[list(drop)] = 0                                                   # lo = hi = 0: nothing good
    return t


@pytest.mark.parametrize("fastq", [False, True])
def test_pack_records_with_a_trim_equals_slicing_by_hand(fastq):
    rng = np.random.default_rng(23)
    for case in (name_lengths_case(fastq), tiny_reads_case(fastq, R=300)):
        names, seq, qual, off = case["names"], case["seq"], case["qual"], case["off"]
        R = len(names)
        # without a trim: today's bytes
        blob, rec_off = hs.pack_records(names, seq, qual, off)
        want, want_off = loop_records(names, seq, qual, off)
        assert blob.tobytes() == want and rec_off.tolist() == want_off
        for drop in ((), (0,), (R - 1,), (3, 4, 5), (0, 1, 2, R - 2, R - 1), range(R)):
            t = _random_trim(off, rng, drop)
            for min_len in (0, 1, 5):
                blob, rec_off = hs.pack_records(names, seq, qual, off, t, min_len)
                want, want_off = loop_trimmed_records(names, seq, qual, off, t, min_len)
                assert blob.tobytes() == want and rec_off.tolist() == want_off and rec_off.dtype == np.int64, (drop, min_len)
                kept = hs.trim_kept(t, min_len)
                assert np.array_equal(np.diff(rec_off) > 0, kept)
                if min_len == 0:
                    assert kept.all()                                   # lo = hi: an empty record, kept
        whole = np.stack([0 * np.diff(off), np.diff(off)], 1)
        assert hs.pack_records(names, seq, qual, off, whole, 0)[0].tobytes() == hs.pack_records(names, seq, qual, off)[0].tobytes()
        with pytest.raises(ValueError):
            hs.pack_records(names, seq, qual, off, whole + 1, 0)


# ---- the switches -----------------------------------------------------------------------------------------------------------------
def test_trim_flag_parsing(monkeypatch, capsys):
    for k in ("NRV_TRIM_Q", "NRV_COMBINED", "NRV_SUMMARY", "NRV_REPORT", "NRV_EDITS"):
        monkeypatch.delenv(k, raising=False)
    base = ["-d", "x", "-o", "y"]
    a = cli.get_args(base)
    assert a.trim_q is None and a.trim_window == 10 and a.min_len == 1 and a.trim_log is None and cli.trim_rule(a) is None
    a = cli.get_args(base + ["--trim_q", "7", "--trim_window", "4", "--min_len", "100", "--trim_log", "t.tsv"])
    assert cli.trim_rule(a) == (7, 4, 100) and a.trim_log == "t.tsv"
    monkeypatch.setenv("NRV_TRIM_Q", "9")
    assert cli.trim_rule(cli.get_args(base)) == (9, 10, 1) and cli.trim_rule(cli.get_args(base + ["--trim_q", "3"])) == (3, 10, 1)
    monkeypatch.delenv("NRV_TRIM_Q")
    for bad in (["--trim_q", "0"], ["--trim_q", "41"], ["--trim_q", "5", "--trim_window", "65"], ["--trim_q", "5", "--trim_window", "0"],
                ["--trim_q", "5", "--min_len", "-1"], ["--trim_q", "5", "--resume"], ["--trim_log", "t.tsv"]):
        with pytest.raises(SystemExit) as e:
            cli.get_args(base + bad)
        assert e.value.code == 2, bad
    assert "--resume cannot be used with --trim_q" in capsys.readouterr().err


def test_route_batch_with_trim():
    class Full:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = with_device_trim = None

    class NoTrim:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None
        with_device_records = with_device_profile = None
    bundle = {"bases": np.zeros(5, "S1"), "meta": np.array([[0, 5, 0, 0]])}
    route = lambda rv, dm, **kw: cli._route_batch(rv, bundle, 1, True, True, dm, False, **kw)
    assert route(Full, True, trim=True) == (27, "pipelined")
    assert route(Full, True, trim=True, combined=True, summary=True, edits=True) == (27, "pipelined")
    assert route(Full, True) == (12, "pipelined") and route(Full, True, summary=True) == (22, "pipelined")
    assert route(NoTrim, True, trim=True) == ("host-merge", "pipelined")
    assert route(Full, False, trim=True) == (7, "pipelined")


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("nrv_"):
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


def test_form_27_marshals_the_trim_behind_every_other_block():
    import ctypes as C
    from nanoreviser_amd import engine
    from nanoreviser_amd.engine import Reviser
    assert 27 in engine._RAW_FORMS and max(engine._RAW_FORMS) == 27
    assert {"nrv_revise_reads_raw_trim_begin", "nrv_revise_reads_raw_trim", "nrv_merge_calls_trim", "nrv_trim_reads",
            "nrv_pack_records_trim"} <= set(engine.SYMBOLS)
    p12 = _packed12()
    p20 = Reviser.with_device_records(Reviser.with_device_edits(Reviser.with_device_report(p12, 0.25)), [b"a", b"bc"], hand_back=False)
    p22 = Reviser.with_device_profile(p20)
    rv = Reviser.__new__(Reviser)
    rv._lib, rv._h = _RecordingLib(), C.c_void_p(0)
    addr = lambda x: C.cast(x, C.c_void_p).value
    for base in (p12, p20, p22):
        p = Reviser.with_device_trim(base, 3, 4, 50)
        assert len(p) == 27 and all(p[k] is base[k] for k in range(len(base)) if k != 12) and all(p[k] is None for k in range(max(len(base), 13), 22))
        assert np.array_equal(p[22], cli.phred_thresholds()) and p[23:26] == (3, 4, 50) and p[26].shape == (2, 2) and p[26].dtype == np.int64
        del rv._lib.calls[:]
        t = rv.begin_packed_raw(p)
        (name, args), = rv._lib.calls
        assert name == "nrv_revise_reads_raw_trim_begin" and len(args) == 25 + 5 + 1
        assert addr(args[25]) == p[22].ctypes.data and args[26:29] == (3, 4, 50) and addr(args[29]) == p[26].ctypes.data
        assert (args[23] is None) == (len(base) < 22) and (args[22] is None) == (len(base) < 20)
        assert len(t) == 3 and len(t[1]) == 10 and t[1][9] is p[26]
        out = rv.run_packed_raw(p)
        assert rv._lib.calls[-1][0] == "nrv_revise_reads_raw_trim" and len(out) == 10 and out[9] is p[26]
        assert (out[8] is None) == (len(base) < 22) and (out[6] is None) == (len(base) < 20)
        assert len(cli._host_merge_form(p)) == 7
    for bad in ((0, 4, 1), (41, 4, 1), (3, 65, 1), (3, 4, -1)):
        with pytest.raises(ValueError):
            Reviser.with_device_trim(p12, *bad)
    with pytest.raises(ValueError):
        Reviser.with_device_trim(tuple(p12[:9]), 3)

    class _Old(_RecordingLib):
        def __getattr__(self, name):
            if "trim" in name:
                raise AttributeError(name)
            return super().__getattr__(name)
    rv._lib = _Old()
    with pytest.raises(engine.NrvError):
        rv.begin_packed_raw(Reviser.with_device_trim(p12, 3))
    with pytest.raises(engine.NrvError):
        rv.trim_reads(np.zeros(3, np.uint8), [0, 3], 3)
    rv._h = None


# ---- the command line on stand-in engines ----------------------------------------------------------------------------------------
class TrimEcho(PipelinedEcho):
    """PipelinedEcho with the merge forms of engine.Reviser, form 27 included: the blocks of a `with_device_*` tuple are filled by
    the host definitions from the echo's calls, so the command line's --device_merge routes run without a device."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.forms = []

    @staticmethod
    def _cls():
        from nanoreviser_amd.engine import Reviser
        return Reviser

    with_device_merge = staticmethod(lambda *a, **k: TrimEcho._cls().with_device_merge(*a, **k))
    with_device_report = staticmethod(lambda *a, **k: TrimEcho._cls().with_device_report(*a, **k))
    with_device_edits = staticmethod(lambda *a, **k: TrimEcho._cls().with_device_edits(*a, **k))
    with_device_records = staticmethod(lambda *a, **k: TrimEcho._cls().with_device_records(*a, **k))
    with_device_profile = staticmethod(lambda *a, **k: TrimEcho._cls().with_device_profile(*a, **k))
    with_device_trim = staticmethod(lambda *a, **k: TrimEcho._cls().with_device_trim(*a, **k))

    def begin_packed_raw(self, packed):
        self.forms.append(len(packed))
        if len(packed) <= 9:
            return super().begin_packed_raw(packed)
        p = tuple(packed) + (None,) * (27 - len(packed))
        t, (p1, p2, a1, a2) = super().begin_packed_raw(tuple(p[:7]))
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
        back = p[11][0] is not None
        outs = (seq if back else None, qual if back else None, off, rep, ed, eoff, blob, roff, prof, trim)
        keep = {12: 3, 14: 4, 16: 6, 20: 8, 22: 9, 27: 10}[len(packed)]
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


def _expected(engine, Q, W, fmt):
    """Per fixture read (A, B): (revised sequence, quality or None, lo, hi) by the definitions on the engine's calls."""
    out = []
    for k in (0, 1):
        _, rd, rt = load_read("_".join(os.path.basename(FAST5[k]).split("_")[-3:-1]))
        calls = engine.predict_read(np.zeros((len(rt.feat_ev), 50), np.float32), rt.feat_ev)
        seq, qual = cli._finish_read(T, rt, *calls, want_qual=fmt == "fastq")
        (lo, hi), = cli.trim_rows(T, rd.bases, [len(rd.bases)], *calls, Q, W).tolist()
        out.append((seq, qual, lo, hi))
    return out


def _record_text(fn, seq, qual, fmt):
    return (hs.fastq_record(fn, list(seq), list(qual)) if fmt == "fastq" else hs.fasta_record(fn, list(seq))).encode()


def _check_fai(blob, fai, fastq, want):
    """Every index line cuts its read's sequence (and quality) out of the file; want: {name: (seq, qual | None)}."""
    lines = fai.decode().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == len(want)
    for ln in lines[:-1]:
        c = ln.split("\t")
        n, o = int(c[1]), int(c[2])
        seq, qual = want[c[0]]
        assert blob[o:o + n].decode() == seq and n == len(seq) and c[3:5] == [str(n), str(n + 1)], c[0]
        if fastq:
            assert blob[int(c[5]):int(c[5]) + n].decode() == qual, c[0]


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_trimmed_output_is_the_same_on_every_host_route(tmp_path, monkeypatch, fmt):
    import __graft_entry__ as g
    g.build_host()
    for k in ("NRV_SUMMARY", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_DEVICE_MERGE", "NRV_DEVICE_STATS", "NRV_CLI_PIPELINE",
              "NRV_HOST_LIB", "NRV_HOST_THREADS", "NRV_TRIM_Q"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib, "_lib", None)
    assert hostlib.load() is not None
    src = _many(tmp_path, 8)
    names = sorted(os.listdir(src))
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                           # several device calls for these reads
    Q, W = 3, 4
    exp = _expected(EchoEngine(), Q, W, fmt)
    kept_len = [hi - lo for _, _, lo, hi in exp]
    assert all(0 < lo < hi < len(s) for s, _, lo, hi in exp) and kept_len[0] != kept_len[1]
    short = int(np.argmin(kept_len))                                   # --min_len between the two: the reads of that kind are dropped
    min_len = min(kept_len) + 1

    def run(tag, extra=(), trim=True, drop=False, rc=0, **kw):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "-F", fmt, "--thread", "2", "--batch", "1024"] + list(extra)
        if trim:
            argv += ["--trim_q", str(Q), "--trim_window", str(W), "--trim_log", out + "trim.tsv"] + (["--min_len", str(min_len)] if drop else [])
        assert cli.main(argv, **kw) == rc
        assert not [f for f in os.listdir(out) if ".part" in f or ".tmp" in f]
        return out

    def want_files(drop):
        w = {"failed_reads.txt": b""}
        for i, fn in enumerate(names):
            s, q, lo, hi = exp[i % 2]
            if not (drop and i % 2 == short):
                w[fn.split(".")[0] + "_out." + fmt] = _record_text(fn, s[lo:hi], q[lo:hi] if q is not None else None, fmt)
        return w

    def want_log(drop):
        rows = []
        for i, fn in enumerate(names):
            s, _, lo, hi = exp[i % 2]
            rows.append([fn, "revised", len(s), lo, hi, int(not (drop and i % 2 == short))])
        total = ["#total", "revised"] + [sum(r[k] for r in rows) for k in range(2, 6)]
        return ("\n".join([cli.TRIM_HEADER] + ["\t".join(str(x) for x in r) for r in rows + [total]]) + "\n").encode()

    # without --trim_q: the untrimmed reads, and no log
    plain = run("plain", trim=False, reviser_factory=lambda a, dev: TrimEcho())
    want_plain = {"failed_reads.txt": b""}
    for i, fn in enumerate(names):
        want_plain[fn.split(".")[0] + "_out." + fmt] = _record_text(fn, exp[i % 2][0], exp[i % 2][1], fmt)
    assert _files(plain) == want_plain
    for drop in (False, True):
        tag = "d" if drop else "k"
        eng_p = TrimEcho()
        piped = run(tag + "piped", drop=drop, reviser_factory=lambda a, dev: eng_p)
        monkeypatch.setenv("NRV_CLI_PIPELINE", "0")
        eng_s = TrimEcho()
        staged = run(tag + "staged", drop=drop, reviser_factory=lambda a, dev: eng_s)
        monkeypatch.delenv("NRV_CLI_PIPELINE")
        assert eng_p.begun >= 2 and set(eng_p.forms) == {7} and eng_s.begun == 0 and eng_s.calls >= 2
        eng_m = TrimEcho()
        merged = run(tag + "merged", ["--device_merge"], drop=drop, reviser_factory=lambda a, dev: eng_m)
        assert set(eng_m.forms) == {27} and len(eng_m.forms) >= 2
        seq_run = run(tag + "seq", ["--thread", "1"], drop=drop, reviser_factory=lambda a, dev: EchoEngine())
        monkeypatch.setenv("NRV_HOST_LIB", "0")                         # the Python reader (no native host stage)
        monkeypatch.setattr(hostlib, "_tried", False)
        monkeypatch.setattr(hostlib, "_lib", None)
        python = run(tag + "python", drop=drop, reviser_factory=lambda a, dev: TrimEcho())
        monkeypatch.delenv("NRV_HOST_LIB")
        monkeypatch.setattr(hostlib, "_tried", False)
        monkeypatch.setattr(hostlib, "_lib", None)
        for o in (piped, staged, merged, seq_run, python):
            f = _files(o)
            assert f.pop("trim.tsv") == want_log(drop), o
            assert f == want_files(drop), (o, sorted(f))
        # --combined, host and device: the same records, an index that cuts them out, dropped reads in neither
        aux = lambda t: ["--report", str(tmp_path / (t + ".rep")), "--edits", str(tmp_path / (t + "_edits")), "--summary", str(tmp_path / (t + ".sum"))]
        eng_c = TrimEcho()
        dev_c = run(tag + "devc", ["--device_merge", "--combined", str(tmp_path / (tag + "dev.out"))] + aux(tag + "dev"), drop=drop,
                    reviser_factory=lambda a, dev: eng_c)
        host_c = run(tag + "hostc", ["--combined", str(tmp_path / (tag + "host.out"))] + aux(tag + "host"), drop=drop,
                     reviser_factory=lambda a, dev: TrimEcho())
        assert set(eng_c.forms) == {27}
        want_recs = {}
        for i, fn in enumerate(names):
            s, q, lo, hi = exp[i % 2]
            if not (drop and i % 2 == short):
                want_recs[hs.record_name(fn).decode()] = (s[lo:hi], q[lo:hi] if q is not None else None)
        for t, o in ((tag + "dev", dev_c), (tag + "host", host_c)):
            assert _files(o) == {"failed_reads.txt": b"", "trim.tsv": want_log(drop)}, o
            blob = open(str(tmp_path / (t + ".out")), "rb").read()
            _check_fai(blob, open(str(tmp_path / (t + ".out.fai")), "rb").read(), fmt == "fastq", want_recs)
            assert len(blob) == sum(len(n) + (2 * len(s) + 6 if fmt == "fastq" else len(s) + 3) for n, (s, _) in want_recs.items())
        # --report / --edits / --summary describe the untrimmed revision: their bytes next to --trim_q are those without it
        if not drop:
            no_trim = run("notrim", ["--combined", str(tmp_path / "notrim.out")] + aux("notrim"), trim=False, reviser_factory=lambda a, dev: TrimEcho())
            assert not os.path.exists(no_trim + "trim.tsv")
        for t in (tag + "dev", tag + "host"):
            for ext in (".rep", ".sum"):
                assert open(str(tmp_path / (t + ext)), "rb").read() == open(str(tmp_path / ("notrim" + ext)), "rb").read(), (t, ext)
            assert _files(str(tmp_path / (t + "_edits")) + "/") == _files(str(tmp_path / "notrim_edits") + "/"), t


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_trim_log_and_files_are_the_same_for_1_2_and_3_workers(tmp_path, monkeypatch, fmt):
    """The hash engine revises for real (insertions, deletions, confidences all over the range); with three workers the two
    largest reads are split over the workers and merged by the parent."""
    for k in ("NRV_TRIM_Q", "NRV_COMBINED", "NRV_SUMMARY", "NRV_REPORT", "NRV_EDITS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE"):
        monkeypatch.delenv(k, raising=False)
    src = _many(tmp_path, 6)
    names = sorted(os.listdir(src))
    Q, W = 5, 10
    exp = _expected(HashEngine(), Q, W, fmt)
    kept_len = [hi - lo for _, _, lo, hi in exp]
    assert all(0 < lo < hi < len(s) for s, _, lo, hi in exp) and kept_len[0] != kept_len[1]
    short, min_len = int(np.argmin(kept_len)), min(kept_len) + 1
    outs = {}
    for world, extra in ((1, []), (2, []), (3, ["--split_reads_above", "0.2"])):
        out = str(tmp_path / f"w{world}") + "/"
        assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "-F", fmt, "--thread", "2", "--trim_q", str(Q), "--trim_window", str(W),
                         "--min_len", str(min_len), "--trim_log", out + "trim.tsv"] + extra, worker_factory=hash_factory, world=world) == 0
        outs[world] = _files(out)
    want = {"failed_reads.txt": b""}
    rows = []
    for i, fn in enumerate(names):
        s, q, lo, hi = exp[i % 2]
        rows.append([fn, "revised", len(s), lo, hi, int(i % 2 != short)])
        if i % 2 != short:
            want[fn.split(".")[0] + "_out." + fmt] = _record_text(fn, s[lo:hi], q[lo:hi] if q is not None else None, fmt)
    total = ["#total", "revised"] + [sum(r[k] for r in rows) for k in range(2, 6)]
    want["trim.tsv"] = ("\n".join([cli.TRIM_HEADER] + ["\t".join(str(x) for x in r) for r in rows + [total]]) + "\n").encode()
    for world in (1, 2, 3):
        assert outs[world] == want, (world, sorted(outs[world]))


def test_an_unrevised_read_is_written_whole_and_is_no_dropped_read(tmp_path, monkeypatch):
    monkeypatch.delenv("NRV_TRIM_Q", raising=False)
    src = _many(tmp_path, 4)
    _, rdA, rtA = load_read("_".join(os.path.basename(FAST5[0]).split("_")[-3:-1]))
    out = str(tmp_path / "o") + "/"
    eng = EchoEngine(fail_marker=rtA.feat_ev[0])                        # every call that STARTS with a read A fails
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "-e", "bad.txt", "--trim_q", "3", "--trim_window", "4",
                     "--trim_log", out + "trim.tsv"], reviser_factory=lambda a, dev: eng) == 0
    failed = set(open(out + "bad.txt").read().split())
    assert failed and "r00_A.fast5" in failed
    lines = [ln.split("\t") for ln in open(out + "trim.tsv").read().split("\n")[1:-2]]
    assert [c[0] for c in lines] == sorted(os.listdir(src))
    for c in lines:
        body = open(out + c[0].split(".")[0] + "_out.fasta").read().split("\n")[1]
        if c[0] in failed:
            assert c[1:] == ["unrevised", str(len(body)), "0", str(len(body)), "1"] and len(body) == len(rdA.bases)
        else:
            assert c[1] == "revised" and c[5] == "1" and len(body) == int(c[4]) - int(c[3]) < int(c[2])
