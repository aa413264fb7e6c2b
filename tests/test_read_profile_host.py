"""The per-read quality and base profile on the host (CPU only): hoststage.read_profile - the definition profile_kernel of
csrc/nrv_profile.h is held to -, the summary line (cli.summary_fields, cli.n50), the routing and marshalling of form 22, and the
command line's --summary on stand-in engines."""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD, load_read
from nanoreviser_amd import cli, hostlib
from nanoreviser_amd import hoststage as hs
from echo_engine import EchoEngine, HashEngine, PipelinedEcho, hash_factory
from profile_cases import loop_profile, profile_case
from report_cases import T, report_case

FAST5 = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")))


def _definition(c, T=T):
    return hs.read_profile(*hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"], T))


def _identities(prof, off):
    p = prof.astype(np.int64)
    assert hs.PROFILE_COLS == 48 and prof.dtype == np.uint64 and prof.shape == (len(off) - 1, 48)
    assert np.array_equal(p[:, :42].sum(1), np.diff(off)) and np.array_equal(p[:, 42:47].sum(1), np.diff(off))
    assert not p[:, 47].any()


# ---- the definition --------------------------------------------------------------------------------------------------------------
def test_read_profile_equals_the_rule_text():
    c = profile_case()
    prof = _definition(c)
    assert np.array_equal(prof, loop_profile(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"]))
    _identities(prof, hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"], T)[2])
    assert (prof[:, 1:41].sum(0) > 0).all() and prof[:, 46].sum() > 0
    assert len(hs.PROFILE_NAMES) == 47 and hs.PROFILE_NAMES[42:] == ("A", "C", "G", "T", "other")
    # the host routes' function: phred_chars -> emit_calls -> read_profile (labels in range: what an argmax gives)
    a1, a2 = np.clip(c["a1"], 0, 5), np.clip(c["a2"], 0, 4)
    got = cli.profile_rows(T, c["bases"], c["ev_len"], c["p1"], c["p2"], a1, a2)
    i = np.arange(c["n"])
    qc = cli.phred_lookup(np.minimum(c["p1"][i, a1], c["p2"][i, a2]))
    assert np.array_equal(got, loop_profile(c["bases"], c["ev_len"], a1, a2, qc))


@pytest.mark.parametrize("Tw", [1, 2, 12, 32])
def test_read_profile_at_other_window_lengths(Tw):
    c = report_case(T=Tw)
    prof = _definition(c, Tw)
    assert np.array_equal(prof, loop_profile(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"], Tw))
    _identities(prof, hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"], Tw)[2])
    assert prof[:, 2].sum() >= min(Tw, 1)                                # the edge events' '#'


def test_read_profile_clips_the_quality_and_counts_exact_bases():
    seq = np.frombuffer(b"ACGTNacgt-A", np.uint8)
    qual = np.array([0, 32, 33, 34, 74, 75, 255, 43, 43, 53, 63], np.uint8)
    prof = hs.read_profile(seq, qual, [0, 0, 7, 11])
    want = np.zeros((3, 48), np.uint64)
    want[1, 0], want[1, 1], want[1, 41] = 3, 1, 3                        # 0, 32, 33 -> 0; 34 -> 1; 74, 75, 255 -> 41
    want[1, 42:47] = [1, 1, 1, 1, 3]                                     # 'N', 'a', 'c' are "other"
    want[2, 10], want[2, 20], want[2, 30] = 2, 1, 1
    want[2, 42:47] = [1, 0, 0, 0, 3]                                     # 'g', 't', '-' are "other"
    assert np.array_equal(prof, want)
    _identities(prof, [0, 0, 7, 11])
    assert hs.read_profile(np.zeros(0, np.uint8), np.zeros(0, np.uint8), [0]).shape == (0, 48)
    # arrays longer than off[-1] (the engine's capacity arrays) are read up to it; shorter ones are an error
    assert np.array_equal(hs.read_profile(np.concatenate([seq, seq]), np.concatenate([qual, qual]), [0, 0, 7, 11]), want)
    with pytest.raises(ValueError):
        hs.read_profile(seq[:5], qual[:5], [0, 7])


def test_calls_without_a_window_have_phred_2_and_their_own_bases():
    z = np.zeros(0, np.int8)
    bases = np.frombuffer(b"ACGTNACG", np.uint8)
    prof = cli.profile_rows(T, bases, [5, 0, 3], np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32), z, z)
    assert prof[:, 2].tolist() == [5, 0, 3] and prof[:, :42].sum() == 8
    assert prof[:, 42:47].tolist() == [[1, 1, 1, 1, 1], [0] * 5, [1, 1, 1, 0, 0]]


# ---- the summary line ------------------------------------------------------------------------------------------------------------
def _row(hist=None, acgt=(0, 0, 0, 0, 0)):
    r = np.zeros(48, np.uint64)
    for k, v in (hist or {}).items():
        r[k] = v
    r[42:47] = acgt
    return r


def test_summary_fields_on_hand_made_rows():
    assert cli.SUMMARY_HEADER.split("\t") == ["name", "status", "bases", "mean_q", "median_q", "q10", "q20", "q30", "gc", "A", "C", "G", "T", "other"]
    f = cli.summary_fields(_row({10: 7}, (2, 1, 2, 1, 1)))
    assert f == ["7", "10.0000", "10", "7", "0", "0", "0.4286", "2", "1", "2", "1", "1"]
    f = cli.summary_fields(_row({10: 5, 20: 5}, (10, 0, 0, 0, 0)))
    assert f[:7] == ["10", "12.5964", "10", "10", "5", "0", "0.0000"]       # the mean of the error probabilities; an even split: the lower bin
    assert cli.summary_fields(_row({10: 4, 20: 5}))[2] == "20" and cli.summary_fields(_row({10: 5, 20: 4}))[2] == "10"
    assert cli.summary_fields(_row()) == ["0", "0.0000", "0", "0", "0", "0", "0.0000", "0", "0", "0", "0", "0"]   # L = 0, bases = 0
    f = cli.summary_fields(_row({}, (1, 2, 3, 4, 0)))                      # an unrevised read: base counts, no histogram
    assert f == ["10", "0.0000", "0", "0", "0", "0", "0.5000", "1", "2", "3", "4", "0"]
    f = cli.summary_fields(_row({2: 3, 9: 1, 10: 1, 29: 2, 30: 1, 41: 1}))
    assert f[3:6] == ["5", "4", "2"] and f[2] == "10"
    assert cli.summary_fields(list(_row({10: 7}))) == cli.summary_fields(_row({10: 7})[:47])
    assert cli.n50([5, 3, 2]) == 5 and cli.n50([]) == 0 and cli.n50([2, 3, 5, 1, 1]) == 3 and cli.n50([4]) == 4 and cli.n50([0, 0]) == 0
    u = cli.unrevised_profile("ACGTNNa")
    assert u[:42].sum() == 0 and u[42:47].tolist() == [1, 1, 1, 1, 3] and cli.unrevised_profile(b"").sum() == 0


def test_summary_flag_parsing(monkeypatch):
    monkeypatch.delenv("NRV_SUMMARY", raising=False)
    assert cli.get_args(["-d", "x", "-o", "y"]).summary is None
    assert cli.get_args(["-d", "x", "-o", "y", "--summary", "s.tsv"]).summary == "s.tsv"
    monkeypatch.setenv("NRV_SUMMARY", "e.tsv")
    assert cli.get_args(["-d", "x", "-o", "y"]).summary == "e.tsv"


# ---- routing and marshalling of form 22 -------------------------------------------------------------------------------------------
class _Offers:
    def __init__(self, *names):
        for n in names:
            setattr(self, n, lambda *a, **k: None)


def test_route_batch_with_summary():
    every = ("run_packed_raw", "begin_packed_raw", "with_device_merge", "with_device_report", "with_device_edits", "with_device_records",
             "with_device_profile")
    bundle = {"bases": np.zeros(5, np.uint8), "meta": np.array([[0, 5]])}
    full, old = _Offers(*every), _Offers(*every[:-1])
    for report, edits, combined, inner in ((False, False, False, 12), (True, False, False, 14), (False, True, False, 16),
                                           (True, True, False, 16), (False, False, True, 20), (True, True, True, 20)):
        kw = dict(edits=edits, combined=combined)
        assert cli._route_batch(full, bundle, 2, True, True, True, report, **kw) == (inner, "pipelined")
        assert cli._route_batch(full, bundle, 2, True, True, True, report, summary=False, **kw) == (inner, "pipelined")
        assert cli._route_batch(full, bundle, 2, True, True, True, report, summary=True, **kw) == (22, "pipelined")
        assert cli._route_batch(old, bundle, 2, True, True, True, report, summary=True, **kw) == ("host-merge", "pipelined")
    # a host-merge form stays one; without --device_merge the summary changes nothing
    no_report = _Offers(*(n for n in every if n != "with_device_report"))
    assert cli._route_batch(no_report, bundle, 2, True, True, True, True, summary=True)[0] == "host-merge"
    assert cli._route_batch(full, bundle, 2, True, True, False, False, summary=True) == (7, "pipelined")
    assert cli._route_batch(full, dict(bundle, device_stats=1), 2, False, True, False, False, summary=True) == (9, "packed+finish_bundle")
    assert cli._route_batch(full, None, 3, True, True, True, False, summary=True)[1] == "predict_many"


class _RecordingLib:
    """Stands where libnanorev_hip.so stands in engine.Reviser._raw_call: records the C arguments, returns NRV_OK."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("nrv_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


def _packed12(nr=2, N=30, fastq=True):
    from nanoreviser_amd.engine import Reviser
    meta = np.zeros((nr, 4), np.int64)
    ev = [N - N // 2, N // 2]
    raw = np.zeros(N * 4, np.int16)
    starts = np.concatenate([np.arange(e, dtype=np.int32) * 4 for e in ev])
    p = Reviser.pack_reads_raw([raw[:ev[0] * 4], raw[:ev[1] * 4]], [starts[:ev[0]], starts[ev[0]:]],
                               [np.zeros((e, 6), np.float32) for e in ev], [0.0, 0.0], [1.0, 1.0], T)
    return Reviser.with_device_merge(p, np.frombuffer(b"ACGT" * N, np.uint8)[:N], fastq)


def test_form_22_marshals_every_block_from_the_one_table():
    import ctypes as C
    from nanoreviser_amd import engine
    from nanoreviser_amd.engine import Reviser
    assert 22 in engine._RAW_FORMS and engine.PROFILE_COLS == hs.PROFILE_COLS
    assert {"nrv_revise_reads_raw_profile_begin", "nrv_revise_reads_raw_profile", "nrv_merge_calls_profile"} <= set(engine.SYMBOLS)
    p12 = _packed12()
    p14 = Reviser.with_device_report(p12, 0.25)
    p16 = Reviser.with_device_edits(p14)
    p20 = Reviser.with_device_records(p16, [b"a", b"bc"], hand_back=False)
    thr = np.linspace(0.1, 0.9, 39).astype(np.float32)
    rv = Reviser.__new__(Reviser)
    rv._lib, rv._h = _RecordingLib(), C.c_void_p(0)
    for base, carried in ((p12, ()), (p14, (12, 13)), (p16, (12, 13, 14, 15)), (p20, tuple(range(12, 20)))):
        p = Reviser.with_device_profile(base, thr)
        assert len(p) == 22 and all(p[k] is base[k] for k in range(12)) and p[20] is not thr and np.array_equal(p[20], thr)
        assert p[21].shape == (2, 48) and p[21].dtype == np.uint64 and not p[21].any()
        assert all(p[k] is base[k] for k in carried if k != 12) and all(p[k] is None for k in range(13, 20) if k not in carried)
        del rv._lib.calls[:]
        t = rv.begin_packed_raw(p)
        (name, args), = rv._lib.calls
        assert name == "nrv_revise_reads_raw_profile_begin" and len(args) == 8 + 2 + 5 + 2 + 2 + 4 + 2 + 1
        assert len(t) == 3 and t[2] == "merged" and len(t[1]) == 9 and t[1][8] is p[21]
        addr = lambda x: C.cast(x, C.c_void_p).value
        assert args[15].value == np.float32(p[12]) and addr(args[23]) == p[20].ctypes.data and addr(args[24]) == p[21].ctypes.data
        assert (args[16] is None) == (p[13] is None) and (args[18] is None) == (p[15] is None) and (args[22] is None) == (p[19] is None)
        assert addr(args[10]) == p[9].ctypes.data and addr(args[11]) == p[10].ctypes.data and addr(args[14]) == p[11][2].ctypes.data
        out = rv.run_packed_raw(p)
        assert rv._lib.calls[-1][0] == "nrv_revise_reads_raw_profile" and len(rv._lib.calls[-1][1]) == 25
        assert len(out) == 9 and out[8] is p[21] and all((out[3 + k] is None) == (p[v] is None) for k, v in enumerate((13, 14, 15, 18, 19)))
    # defaults and refusals
    assert np.array_equal(Reviser.with_device_profile(p12)[20], cli.phred_thresholds())
    with pytest.raises(ValueError):
        Reviser.with_device_profile(tuple(p12[:9]))
    with pytest.raises(ValueError):
        Reviser.with_device_profile(p12, thr[:38])
    with pytest.raises(ValueError):
        rv.run_packed_raw(tuple(p12) + (None,) * 9)
    # the host-merge form of a 22 tuple is the call that returns (p1, p2, a1, a2)
    assert len(cli._host_merge_form(Reviser.with_device_profile(p20))) == 7
    # an older library: the symbols are found by presence
    class _Old(_RecordingLib):
        def __getattr__(self, name):
            if "profile" in name:
                raise AttributeError(name)
            return super().__getattr__(name)
    rv._lib = _Old()
    with pytest.raises(engine.NrvError):
        rv.begin_packed_raw(Reviser.with_device_profile(p12))
    with pytest.raises(engine.NrvError):
        rv.merge_calls_profile_device(np.zeros(3, np.uint8), [3], [], [], np.zeros((0, 6)), np.zeros((0, 5)))
    rv._h = None


# ---- the command line on stand-in engines -----------------------------------------------------------------------------------------
class ProfileEcho(PipelinedEcho):
    """PipelinedEcho with the merge forms of engine.Reviser, form 22 included: the blocks of a `with_device_*` tuple are filled by the
    host definitions from the echo's calls, so the command line's --device_merge routes run without a device."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.forms = []

    @staticmethod
    def _cls():
        from nanoreviser_amd.engine import Reviser
        return Reviser

    with_device_merge = staticmethod(lambda *a, **k: ProfileEcho._cls().with_device_merge(*a, **k))
    with_device_report = staticmethod(lambda *a, **k: ProfileEcho._cls().with_device_report(*a, **k))
    with_device_edits = staticmethod(lambda *a, **k: ProfileEcho._cls().with_device_edits(*a, **k))
    with_device_records = staticmethod(lambda *a, **k: ProfileEcho._cls().with_device_records(*a, **k))
    with_device_profile = staticmethod(lambda *a, **k: ProfileEcho._cls().with_device_profile(*a, **k))

    def begin_packed_raw(self, packed):
        self.forms.append(len(packed))
        if len(packed) <= 9:
            return super().begin_packed_raw(packed)
        p = tuple(packed) + (None,) * (22 - len(packed))
        t, (p1, p2, a1, a2) = super().begin_packed_raw(tuple(p[:7]))
        el = [int(d.ev_len) for d in p[3]]
        fastq = p[10] is not None
        qc = (cli.phred_chars(p1, p2, a1, a2) if len(a1) else np.zeros(0, np.uint8)) if fastq else None
        seq, qual, off = hs.emit_calls(p[9], el, a1, a2, qc, self.T)
        rep = hs.revision_report(p[9], el, a1, a2, p1, p2, qc, self.T, p[12]) if p[13] is not None else None
        ed, eoff = hs.revision_edits(p[9], el, a1, a2, p1, p2, qc, self.T) if p[15] is not None else (None, None)
        blob, roff = (None, None)
        if p[19] is not None:
            names = [p[16][int(p[17][r]):int(p[17][r + 1])].tobytes() for r in range(len(el))]
            blob, roff = hs.pack_records(names, seq, qual, off)
        prof = cli.profile_rows(self.T, p[9], el, p1, p2, a1, a2) if p[21] is not None else None
        back = p[11][0] is not None
        outs = (seq if back else None, qual if back else None, off, rep, ed, eoff, blob, roff, prof)
        keep = {12: 3, 14: 4, 16: 6, 20: 8, 22: 9}[len(packed)]
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


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0] == cli.SUMMARY_HEADER
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert all(len(r) == 14 for r in rows[:-1]) and rows[-2][:2] == ["#total", "revised"] and rows[-1][0] == "#reads" and len(rows[-1]) == 4
    return rows[:-2], rows[-2], rows[-1]


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_summary_file_is_the_same_on_every_host_route(tmp_path, monkeypatch, fmt):
    import __graft_entry__ as g
    g.build_host()
    for k in ("NRV_SUMMARY", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_DEVICE_MERGE", "NRV_DEVICE_STATS", "NRV_CLI_PIPELINE",
              "NRV_HOST_LIB", "NRV_HOST_THREADS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib, "_lib", None)
    assert hostlib.load() is not None
    src = _many(tmp_path, 8)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                           # several device calls for these reads

    def run(tag, extra=(), summary=True, **kw):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "-F", fmt, "--thread", "2", "--batch", "1024"] + list(extra)
        assert cli.main(argv + (["--summary", out + "summary.tsv"] if summary else []), **kw) == 0
        assert not [f for f in os.listdir(out) if ".part" in f or ".tmp" in f]
        return out

    plain = run("plain", summary=False, reviser_factory=lambda a, dev: ProfileEcho())
    assert not os.path.exists(plain + "summary.tsv") and len(_files(plain)) == 9
    eng_p = ProfileEcho()
    piped = run("piped", reviser_factory=lambda a, dev: eng_p)
    monkeypatch.setenv("NRV_CLI_PIPELINE", "0")
    eng_s = ProfileEcho()
    staged = run("staged", reviser_factory=lambda a, dev: eng_s)
    monkeypatch.delenv("NRV_CLI_PIPELINE")
    assert eng_p.begun >= 2 and set(eng_p.forms) == {7} and eng_s.begun == 0 and eng_s.calls >= 2
    # the merge forms: --device_merge turns every call into form 22, alone and with the report, the edit list and the records
    eng_m = ProfileEcho()
    merged = run("merged", ["--device_merge"], reviser_factory=lambda a, dev: eng_m)
    eng_a = ProfileEcho()
    allof = run("allof", ["--device_merge", "--report", str(tmp_path / "allof.rep"), "--edits", str(tmp_path / "allof_edits"),
                          "--combined", str(tmp_path / "allof.out")], reviser_factory=lambda a, dev: eng_a)
    assert set(eng_m.forms) == {22} and set(eng_a.forms) == {22} and len(eng_m.forms) >= 2
    host_all = run("host_all", ["--report", str(tmp_path / "host.rep"), "--edits", str(tmp_path / "host_edits"),
                                "--combined", str(tmp_path / "host.out")], reviser_factory=lambda a, dev: ProfileEcho())
    workers = run("workers", ["--split_reads_above", "0.2"], worker_factory=hash_factory, world=3)
    one = run("one", worker_factory=hash_factory, world=1)
    # the Python reader (no native host stage)
    monkeypatch.setenv("NRV_HOST_LIB", "0")
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib, "_lib", None)
    python = run("python", reviser_factory=lambda a, dev: ProfileEcho())
    monkeypatch.delenv("NRV_HOST_LIB")
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib, "_lib", None)

    ref = open(piped + "summary.tsv", "rb").read()
    for o in (staged, merged, python):
        assert open(o + "summary.tsv", "rb").read() == ref, o
        assert {k: v for k, v in _files(o).items() if k != "summary.tsv"} == _files(plain), o
    for o in (allof, host_all):
        assert open(o + "summary.tsv", "rb").read() == ref, o
    assert open(str(tmp_path / "allof.rep"), "rb").read() == open(str(tmp_path / "host.rep"), "rb").read()
    assert sorted(open(str(tmp_path / "allof.out"), "rb").read().split(b"\n")) == sorted(open(str(tmp_path / "host.out"), "rb").read().split(b"\n"))
    assert _files(str(tmp_path / "allof_edits") + "/") == _files(str(tmp_path / "host_edits") + "/")
    assert open(workers + "summary.tsv", "rb").read() == open(one + "summary.tsv", "rb").read()

    rows, total, reads = _table(piped + "summary.tsv")
    names = sorted(os.listdir(src))
    assert [r[0] for r in rows] == names and all(r[1] == "revised" for r in rows)
    for k in (0, 1):                                                    # a line is the summary of the definition on that read's calls
        _, rd, rt = load_read("_".join(os.path.basename(FAST5[k]).split("_")[-3:-1]))
        calls = EchoEngine().predict_read(np.zeros((len(rt.feat_ev), 50), np.float32), rt.feat_ev)
        want = cli.profile_rows(T, rd.bases, [len(rd.bases)], *calls)[0]
        assert rows[k][2:] == cli.summary_fields(want)
        rec = _files(plain)[names[k].split(".")[0] + "_out." + fmt].split(b"\n")
        assert int(rows[k][2]) == len(rec[1].split(b"+")[0]) == len(rd.bases)      # (the per-read FASTQ has '+' at the end of the sequence line)
        if fmt == "fastq":
            assert len(rec[2]) == len(rd.bases) and int(rows[k][5]) == sum(ch >= ord("+") for ch in rec[2])
    assert int(total[2]) == sum(int(r[2]) for r in rows) and [int(total[k]) for k in range(9, 14)] == [sum(int(r[k]) for r in rows) for k in range(9, 14)]
    assert reads[1:] == ["8", "0", str(cli.n50([int(r[2]) for r in rows]))]
    # the hash engine revises for real: a line is still the definition on its calls
    rows_h, _, reads_h = _table(one + "summary.tsv")
    for k in (0, 1):
        _, rd, rt = load_read("_".join(os.path.basename(FAST5[k]).split("_")[-3:-1]))
        want = cli.profile_rows(T, rd.bases, [len(rd.bases)], *HashEngine().predict_read(None, rt.feat_ev))[0]
        assert rows_h[k][2:] == cli.summary_fields(want) and int(rows_h[k][2]) != len(rd.bases)
    assert reads_h[1:3] == ["8", "0"]


def _written(out, fn, fmt):
    """The sequence in a per-read output file (the per-read FASTQ has '+' at the end of the sequence line, which is not a base)."""
    line = open(out + fn.split(".")[0] + "_out." + fmt).read().split("\n")[1]
    assert (fmt == "fastq") == line.endswith("+")
    return line[:-1] if fmt == "fastq" else line


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_summary_marks_fallback_and_resumed_reads_unrevised(tmp_path, monkeypatch, fmt):
    src = _many(tmp_path, 6)
    _, rdA, rtA = load_read("_".join(os.path.basename(FAST5[0]).split("_")[-3:-1]))
    out = str(tmp_path / "o") + "/"
    monkeypatch.setenv("NRV_SUMMARY", out + "sum.tsv")                  # the environment form of --summary
    eng = EchoEngine(fail_marker=rtA.feat_ev[0])                        # every call that STARTS with a read A fails
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "-F", fmt, "--thread", "2", "-e", "bad.txt"], reviser_factory=lambda a, dev: eng) == 0
    failed = set(open(out + "bad.txt").read().split())
    rows, total, reads = _table(out + "sum.tsv")
    assert failed and "r00_A.fast5" in failed and [r[0] for r in rows] == sorted(os.listdir(src))
    for r in rows:
        text = _written(out, r[0], fmt)
        assert r[1] == ("unrevised" if r[0] in failed else "revised")
        assert int(r[2]) == len(text) and [int(v) for v in r[9:13]] == [text.count(c) for c in "ACGT"]
        assert int(r[13]) == len(text) - sum(text.count(c) for c in "ACGT")
        if r[0] in failed:
            assert r[3:8] == ["0.0000", "0", "0", "0", "0"]
        else:
            assert float(r[3]) > 2 and int(r[5]) > 0                    # in a FASTA run too: the profile is that of the FASTQ form
    rev = [int(r[2]) for r in rows if r[1] == "revised"]
    assert reads[1:] == [str(len(rev)), str(len(failed)), str(cli.n50(rev))] and int(total[2]) == sum(rev)
    # --resume: the reads that already have an output are summarised as what lies on disk
    monkeypatch.delenv("NRV_SUMMARY")
    good = EchoEngine()
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "-F", fmt, "--thread", "2", "-e", "bad.txt", "--resume", "--summary", out + "sum2.tsv"],
                    reviser_factory=lambda a, dev: good) == 0
    rows2, total2, reads2 = _table(out + "sum2.tsv")
    for r, r2 in zip(rows, rows2):
        text = _written(out, r[0], fmt)                                 # a skipped read: bases and counts are the file's sequence
        assert r2[0] == r[0] and int(r2[2]) == len(text) and [int(v) for v in r2[9:13]] == [text.count(c) for c in "ACGT"]
        assert int(r2[13]) == len(text) - sum(text.count(c) for c in "ACGT") == 0
        assert r2[8] == format((text.count("C") + text.count("G")) / len(text), ".4f")
        if r[0] not in failed:
            assert r2[2] == r[2] and r2[8:] == r[8:]
        assert r2[1] == ("revised" if r[0] in failed else "unrevised")
        assert (r2[3] == "0.0000") == (r[0] not in failed)
    assert reads2[1:3] == [str(len(failed)), str(len(rows) - len(failed))]
    assert int(total2[2]) == sum(int(r2[2]) for r2 in rows2 if r2[1] == "revised")
    # the function itself, on a six-base record of either format
    for f, rec in (("fasta", ">r\nACGTAC"), ("fastq", "@r\nACGTAC+\n######")):
        (tmp_path / ("six." + f)).write_text(rec)
        assert cli.written_sequence(str(tmp_path / ("six." + f)), f == "fastq") == b"ACGTAC"
        assert cli.summary_fields(cli.unrevised_profile(cli.written_sequence(str(tmp_path / ("six." + f)), f == "fastq")))[:1] + \
            cli.summary_fields(cli.unrevised_profile(b"ACGTAC"))[6:] == ["6", "0.5000", "2", "2", "1", "1", "0"]
    assert cli.written_sequence(str(tmp_path / "none"), True) == b""
