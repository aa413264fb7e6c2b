"""Host side of the device merge (CPU only): the definition the kernels of csrc/nrv_merge.h are held to, the Phred threshold
table that replaces log10 on the device, the native record writer, and the command line's --device_merge switch.

  * hoststage.emit_calls (the per-event, per-call form the device computes) against cli._finish_read read by read, byte for
    byte: the five fixture reads with seeded random calls - random calls exercise more rules than real ones - overwritten with
    the model goldens' calls where tests/golden/model_goldens.npz has them; FASTA and FASTQ; one read per call and all in one
    call; reads of ev_len <= T and T + 1 among them;
  * cli.phred_thresholds: strictly increasing, and the table lookup equals cli.phred_chars at every step +- 1 ulp, at 0, 1,
    nextafter(1, 0) and on 10^6 random f32 values; nrvh_phred_thresholds (C, f64 log10) gives the same 39 bit patterns;
  * nrvh_write_records against nrvh_finish_bundle on the same calls: file bytes, n_written, status; a name with blanks; an
    unwritable destination for one read of three;
  * the sanitizer driver's new cases through the gate script;
  * the switch: parsing and help; off = exactly the calls of before; on = the pipelined path takes the new packed form and the
    output files are the same bytes, alone and with --device_stats; the host-fed paths never see the new form; a read that
    fails in the native writer, and a call that fails in its second half, end in `fallback` / the per-read retry as before.
"""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLD
from nanoreviser_amd import cli, hostlib
from nanoreviser_amd import hoststage as hs
from echo_engine import PipelinedEcho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST5 = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")))
MORE5 = sorted(glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))
T = 11


@pytest.fixture(scope="module", autouse=True)
def _host_library():
    import __graft_entry__ as g
    g.build_host()
    assert hostlib.has_write_records(), "libnanorev_host.so lacks nrvh_write_records / nrvh_phred_thresholds"


# ---- the definition --------------------------------------------------------------------------------------------------------------
class _Read:
    def __init__(self, bases):
        self.bases = bases


def _fixture_calls(reads, model_goldens, sp="ecoli"):
    """Per fixture read: (bases S1[N], p1, p2, a1, a2) - random calls, the goldens' calls at the windows they cover."""
    rng = np.random.default_rng(2511)
    out = []
    for key in reads.keys:
        _, rd, _ = reads(key)
        n = len(rd.bases) - T
        a1, a2 = rng.integers(0, 6, n).astype(np.int8), rng.integers(0, 5, n).astype(np.int8)
        p1, p2 = rng.random((n, 6), dtype=np.float32), rng.random((n, 5), dtype=np.float32)
        idx = np.asarray(model_goldens[f"{key}/idx"])
        idx = idx[idx < n]
        for name, arr in (("p1", p1), ("p2", p2), ("a1", a1), ("a2", a2)):
            arr[idx] = np.asarray(model_goldens[f"{key}/{sp}/{name}"])[: len(idx)]
        out.append((np.asarray(rd.bases, "S1"), p1, p2, a1, a2))
    # a read without a window, one with exactly T bases and one with a single window
    for el in (4, T, T + 1):
        n = max(el - T, 0)
        out.append((rng.choice(np.frombuffer(b"ACGT", "S1"), el), rng.random((n, 6), dtype=np.float32), rng.random((n, 5), dtype=np.float32),
                    rng.integers(0, 6, n).astype(np.int8), rng.integers(0, 5, n).astype(np.int8)))
    return out


def _as_one_call(rs):
    """Reads -> the arrays of ONE device call: window i of a read is window ev_off + i; the T windows between two reads are nobody's."""
    ev_len = [len(r[0]) for r in rs]
    N = sum(ev_len)
    n = max(N - T, 0)
    p1, p2 = np.full((n, 6), np.nan, np.float32), np.full((n, 5), np.nan, np.float32)
    a1, a2 = np.full(n, 1, np.int8), np.full(n, 0, np.int8)              # (what lies between reads would DROP a base if it were used)
    e0 = 0
    for b, q1, q2, x1, x2 in rs:
        k = len(x1)
        p1[e0:e0 + k], p2[e0:e0 + k], a1[e0:e0 + k], a2[e0:e0 + k] = q1, q2, x1, x2
        e0 += len(b)
    return np.concatenate([r[0] for r in rs]), ev_len, p1, p2, a1, a2


@pytest.mark.parametrize("fastq", [False, True])
def test_emit_calls_equals_finish_read(reads, model_goldens, fastq):
    rs = _fixture_calls(reads, model_goldens)
    want = [cli._finish_read(T, _Read(b), p1, p2, a1, a2, want_qual=fastq) for b, p1, p2, a1, a2 in rs]
    assert any("D" not in w[0] and len(w[0]) != len(r[0]) for w, r in zip(want, rs))          # the calls do change lengths
    for group in [[r] for r in rs] + [rs, rs[::-1], rs[5:] + rs[:2]]:
        bases, ev_len, p1, p2, a1, a2 = _as_one_call(group)
        with np.errstate(invalid="ignore"):
            qc = cli.phred_chars(np.nan_to_num(p1), np.nan_to_num(p2), a1, a2) if fastq and len(a1) else (np.zeros(0, np.uint8) if fastq else None)
        seq, qual, off = hs.emit_calls(bases.view(np.uint8), ev_len, a1, a2, qc, T)
        assert off.dtype == np.int64 and len(off) == len(group) + 1 and off[0] == 0 and off[-1] == len(seq)
        assert (qual is None) == (not fastq)
        for r, one in enumerate(group):
            s, q = want[[id(x) for x in rs].index(id(one))]
            assert seq[off[r]:off[r + 1]].tobytes().decode("ascii") == s, (len(group), r)
            if fastq:
                assert qual[off[r]:off[r + 1]].tobytes().decode("ascii") == q, (len(group), r)
    # S1 bases are taken as well, and a mismatch between bases and ev_len is refused
    b, el, p1, p2, a1, a2 = _as_one_call(rs[:2])
    assert np.array_equal(hs.emit_calls(b, el, a1, a2, None, T)[0], hs.emit_calls(b.view(np.uint8), el, a1, a2, None, T)[0])
    with pytest.raises(ValueError):
        hs.emit_calls(b[:-1], el, a1, a2, None, T)


# ---- Phred thresholds --------------------------------------------------------------------------------------------------------------
def _phred_of(conf):
    c = np.asarray(conf, np.float32).reshape(-1, 1)
    return cli.phred_chars(c, c)


def test_phred_thresholds_reproduce_phred_chars():
    thr = cli.phred_thresholds()
    assert thr.dtype == np.float32 and thr.shape == (39,) and (np.diff(thr) > 0).all()
    assert thr is cli.phred_thresholds()                                 # cached
    assert abs(float(thr[0]) - 0.29205424) < 1e-7 and abs(float(thr[-1]) - 0.9998878) < 1e-7
    below, above = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(2))
    k = np.arange(2, 41)
    assert np.array_equal(_phred_of(thr) - 33, k) and np.array_equal(_phred_of(below) - 33, k - 1)     # each entry IS the step
    pts = np.concatenate([thr, below, above, np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(0))], np.float32)])
    assert np.array_equal(cli.phred_lookup(pts), _phred_of(pts))
    rng = np.random.default_rng(40)
    c = np.concatenate([rng.random(700_000, dtype=np.float32), (1 - rng.random(300_000, dtype=np.float32) ** 4).astype(np.float32)])
    got, want = cli.phred_lookup(c), _phred_of(c)
    assert np.array_equal(got, want) and len(np.unique(want)) == 40
    # the lookup on gathered confidences is phred_chars on the probabilities
    p1, p2 = rng.random((5000, 6), dtype=np.float32), rng.random((5000, 5), dtype=np.float32)
    a1, a2 = p1.argmax(1).astype(np.int8), p2.argmax(1).astype(np.int8)
    i = np.arange(5000)
    assert np.array_equal(cli.phred_lookup(np.minimum(p1[i, a1], p2[i, a2])), cli.phred_chars(p1, p2, a1, a2))


def test_native_phred_thresholds_are_the_same_bit_patterns():
    """If the C library's log10 ever disagreed with NumPy's at a step, this says so (the command line passes the Python table)."""
    thr = hostlib.phred_thresholds()
    assert thr is not None and np.array_equal(thr.view(np.uint32), cli.phred_thresholds().view(np.uint32))


# ---- the record writer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fastq", [False, True])
def test_write_records_equals_finish_bundle(reads, model_goldens, tmp_path, fastq):
    rs = _fixture_calls(reads, model_goldens)
    bases, ev_len, p1, p2, a1, a2 = _as_one_call(rs)
    with np.errstate(invalid="ignore"):
        qc = cli.phred_chars(np.nan_to_num(p1), np.nan_to_num(p2), a1, a2) if fastq else None
    names = [f"read {i} of a run.fast5".replace(" ", "|||") for i in range(len(rs))]
    ext = "fastq" if fastq else "fasta"
    da = [str(tmp_path / f"a{i}_out.{ext}") for i in range(len(rs))]
    db = [str(tmp_path / f"b{i}_out.{ext}") for i in range(len(rs))]
    da[1] = db[1] = str(tmp_path / "no_such_dir" / "x")                   # one read cannot be written: the others still are
    nw_a, st_a = hostlib.finish_bundle(bases, ev_len, a1, a2, T, qc, names, da, fastq)
    seq, qual, off = hs.emit_calls(bases.view(np.uint8), ev_len, a1, a2, qc, T)
    nw_b, st_b = hostlib.write_records(seq, qual, off, names, db, fastq)
    assert np.array_equal(st_a, st_b) and st_b[1] == hostlib.E_IO and not np.delete(st_b, 1).any()
    assert np.array_equal(np.delete(nw_a, 1), np.delete(nw_b, 1)) and nw_b[1] == 0
    assert np.array_equal(np.delete(nw_b, 1), np.delete(np.diff(off), 1))
    for i, (x, y) in enumerate(zip(da, db)):
        if i != 1:
            assert open(x, "rb").read() == open(y, "rb").read(), i
    txt = open(db[0], "rb").read()
    assert txt.startswith((b"@" if fastq else b">") + b"read|||0|||of|||a|||run.fast5\n") and not txt.endswith(b"\n")
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for i, p in enumerate(da + db) if i % len(rs) != 1)   # no temporary left
    # FASTQ without a quality array: '#' per base, what cli.write_read writes
    if fastq:
        nw, st = hostlib.write_records(seq, None, off[:2], names[:1], [str(tmp_path / "plain.fastq")], True)
        assert st[0] == hostlib.OK and open(tmp_path / "plain.fastq", "rb").read().endswith(b"+\n" + b"#" * int(off[1]))
    # offsets that are not ascending or leave the buffer refuse that read alone
    bad = off.copy()
    bad[2] = bad[3] + 5
    dc = [str(tmp_path / f"c{i}_out.{ext}") for i in range(len(rs))]
    nw, st = hostlib.write_records(seq, qual, bad, names, dc, fastq)
    assert st[2] == hostlib.E_ARG and nw[2] == 0 and not np.delete(st, 2).any() and not os.path.exists(dc[2])
    bad = off.copy()
    bad[-1] += 1
    assert hostlib.write_records(seq, qual, bad, names, dc, fastq)[1].tolist() == [0] * (len(rs) - 1) + [hostlib.E_ARG]
    nw, st = hostlib.write_records(seq, qual, off[:1], [], [], fastq)       # zero reads
    assert len(nw) == 0 and len(st) == 0


def _have_sanitizers():
    if shutil.which("gcc") is None:
        return False
    r = subprocess.run(["gcc", "-fsanitize=address,undefined", "-x", "c", "-", "-o", os.devnull], input="int main(void){return 0;}",
                       capture_output=True, text=True)
    return r.returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason="gcc with libasan / libubsan is not in this image")
def test_sanitizer_driver_covers_the_record_writer():
    """The gate script with a handful of mutations: its `api` mode drives nrvh_write_records (zero reads, offsets that are not
    monotone, negative or past the buffer, an empty read, NULL qual with fastq) and nrvh_phred_thresholds under ASan + UBSan, its
    `threads` mode the writer from eight threads under TSan."""
    src = open(os.path.join(ROOT, "tools", "hostfuzz", "host_fuzz.c")).read()
    assert "nrvh_write_records" in src and "nrvh_phred_thresholds" in src and "off_bad" in src
    r = subprocess.run(["bash", os.path.join(ROOT, "scripts", "host_sanitize.sh"), "8", "3"], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "api ok" in out and "threads ok: 8 x 6" in out and "SANITIZE OK" in out, out[-2000:]
    for word in ("runtime error", "ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "WARNING: ThreadSanitizer", "SANITIZE FAIL"):
        assert word not in out, out[-4000:]


# ---- the command-line switch -----------------------------------------------------------------------------------------------------------
class MergingEcho(PipelinedEcho):
    """PipelinedEcho that knows the packed forms of engine.Reviser (device statistics, device merge) and answers a merge call
    with hoststage.emit_calls on its own echo - what the device does, by definition - and writes down every call it receives."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.log = []

    @staticmethod
    def with_device_stats(packed, last_dur, on_device):
        from nanoreviser_amd.engine import Reviser
        return Reviser.with_device_stats(packed, last_dur, on_device)

    @staticmethod
    def with_device_merge(packed, bases, fastq, q_thr=None):
        from nanoreviser_amd.engine import Reviser
        return Reviser.with_device_merge(packed, bases, fastq, q_thr)

    def begin_packed_raw(self, packed):
        self.log.append(("begin", len(packed), len(packed) == 12 and packed[7] is not None))
        t, out = super().begin_packed_raw(packed[:7])
        return (t, (out, packed), "merged") if len(packed) == 12 else (t, out)

    def end_packed_raw(self, ticket):
        if len(ticket) == 2:
            return super().end_packed_raw(ticket)
        t, ((p1, p2, a1, a2), packed), _ = ticket
        super().end_packed_raw((t, (p1, p2, a1, a2)))
        descs, nr, bases, thr = packed[3], packed[4], packed[9], packed[10]
        qc = None
        if thr is not None:
            i = np.arange(len(a1))
            qc = (33 + 1 + np.searchsorted(thr, np.minimum(p1[i, a1], p2[i, a2]), "right")).astype(np.uint8)
        return hs.emit_calls(bases, [descs[r].ev_len for r in range(nr)], a1, a2, qc, self.T)

    def run_packed_raw(self, packed):
        self.log.append(("run", len(packed), False))
        return super().run_packed_raw(packed)

    def predict_reads_raw(self, raws, starts, feats, shifts, scales):
        self.log.append(("predict_reads_raw", 0, False))
        return super().predict_reads_raw(raws, starts, feats, shifts, scales)


def _inputs(tmp_path, n=12):
    d = tmp_path / "in"
    d.mkdir()
    src = FAST5 + MORE5
    for i in range(n):
        shutil.copy(src[i % len(src)], d / f"r{i:02d}.fast5")
    return str(d)


def _run(tmp_path, tag, d, extra, eng=None, **kw):
    eng = eng or MergingEcho()
    out = str(tmp_path / tag) + "/"
    if "worker_factory" in kw:
        rc = cli.main(["-d", d, "-o", out, "-S", "ecoli", "--thread", "3"] + extra, **kw)
    else:
        rc = cli.main(["-d", d, "-o", out, "-S", "ecoli", "--thread", "3"] + extra, reviser_factory=lambda a, dev: eng)
    return eng, {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}, rc


def _env(monkeypatch):
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_ENGINES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NRV_CLI_GROUPS", "1")                           # small device calls: several bundles
    monkeypatch.setenv("NRV_CLI_PIPELINE", "1")


def test_switch_parsing_and_help(monkeypatch, capsys):
    _env(monkeypatch)
    base = ["-d", "x", "-o", "y"]
    assert cli.get_args(base).device_merge is False
    assert cli.get_args(base + ["--device_merge"]).device_merge is True and cli.get_args(base + ["--device_merge"]).device_stats is False
    for v, want in (("1", True), ("0", False), ("", False), ("yes", True)):
        monkeypatch.setenv("NRV_DEVICE_MERGE", v)
        assert cli.get_args(base).device_merge is want, v
    monkeypatch.delenv("NRV_DEVICE_MERGE")
    with pytest.raises(SystemExit):
        cli.get_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--device_merge" in text and "NRV_DEVICE_MERGE=1" in text
    for path in ("Python fallback reader", "NRV_CLI_PIPELINE=0", "several engines", "split over GPU workers", "per-read retry"):
        assert path in text, path


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_switch_off_changes_no_call_and_on_writes_the_same_bytes(tmp_path, monkeypatch, fmt):
    _env(monkeypatch)
    d = _inputs(tmp_path)
    seen = []
    real_fb, real_wr, real_ph = hostlib.finish_bundle, hostlib.write_records, cli.phred_chars
    monkeypatch.setattr(hostlib, "finish_bundle", lambda *a: seen.append("finish_bundle") or real_fb(*a))
    monkeypatch.setattr(hostlib, "write_records", lambda *a: seen.append("write_records") or real_wr(*a))
    monkeypatch.setattr(cli, "phred_chars", lambda *a: seen.append("phred_chars") or real_ph(*a))
    off, files_off, rc = _run(tmp_path, "off", d, ["-F", fmt])
    assert rc == 0 and off.log and all(x == ("begin", 7, False) for x in off.log)
    assert set(seen) == ({"finish_bundle", "phred_chars"} if fmt == "fastq" else {"finish_bundle"})
    assert len(files_off) == 13 and files_off["failed_reads.txt"] == b""
    for tag, extra, form in (("on", ["--device_merge"], ("begin", 12, False)), ("both", ["--device_merge", "--device_stats"], ("begin", 12, True))):
        del seen[:]
        on, files_on, rc = _run(tmp_path, tag, d, ["-F", fmt] + extra)
        assert rc == 0 and len(on.log) == len(off.log) and all(x == form for x in on.log), on.log
        assert set(seen) == {"write_records"}                            # no phred_chars, no nrvh_finish_bundle in the finisher
        assert files_on == files_off and not on.violations
    del seen[:]
    monkeypatch.setenv("NRV_DEVICE_MERGE", "1")                          # the environment form, no flag
    env, files_env, rc = _run(tmp_path, "env", d, ["-F", fmt])
    assert rc == 0 and all(x == ("begin", 12, False) for x in env.log) and files_env == files_off


def test_other_paths_keep_the_host_merge(tmp_path, monkeypatch):
    _env(monkeypatch)
    d = _inputs(tmp_path)
    _, ref, _ = _run(tmp_path, "ref", d, [])

    def host_merge(eng):
        return eng.log and all(n in (0, 7) for _, n, _ in eng.log)
    monkeypatch.setenv("NRV_CLI_PIPELINE", "0")                          # one call at a time
    eng, files, _ = _run(tmp_path, "nopipe", d, ["--device_merge"])
    assert host_merge(eng) and files == ref
    monkeypatch.setenv("NRV_CLI_PIPELINE", "1")
    made = []                                                            # several engines on the device
    monkeypatch.setenv("NRV_CLI_ENGINES", "2")
    _, files, _ = _run(tmp_path, "two", d, ["--device_merge"], worker_factory=lambda a, dev: made.append(MergingEcho()) or made[-1], world=1)
    assert len(made) == 2 and all(host_merge(e) for e in made if e.log) and any(e.log for e in made) and files == ref
    monkeypatch.delenv("NRV_CLI_ENGINES")
    calls = []                                                           # an engine without the new calls

    class Old(PipelinedEcho):
        def begin_packed_raw(self, packed):
            calls.append(len(packed))
            return super().begin_packed_raw(packed)
    _, files, _ = _run(tmp_path, "old", d, ["--device_merge"], eng=Old())
    assert calls and set(calls) == {7} and files == ref
    eng = MergingEcho()                                                  # no pool (sequential reads)
    out = str(tmp_path / "seq") + "/"
    assert cli.main(["-d", d, "-o", out, "-S", "ecoli", "--thread", "1", "--device_merge"], reviser_factory=lambda a, dev: eng) == 0
    assert host_merge(eng) and {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))} == ref
    # a host library without the new symbols
    monkeypatch.setattr(hostlib, "has_write_records", lambda: False)
    eng, files, _ = _run(tmp_path, "oldlib", d, ["--device_merge"])
    assert host_merge(eng) and files == ref
    monkeypatch.undo()
    _env(monkeypatch)
    monkeypatch.setattr(hostlib, "load", lambda: None)                   # the Python fallback reader (no native library)
    eng = MergingEcho()
    out = str(tmp_path / "py") + "/"
    assert cli.main(["-d", d, "-o", out, "-S", "ecoli", "--thread", "1", "--device_merge"], reviser_factory=lambda a, dev: eng) == 0
    assert host_merge(eng) and {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))} == ref
    monkeypatch.undo()
    eng = MergingEcho()                                                  # a slice of a read split over GPU workers
    args = cli.get_args(["-d", os.path.dirname(FAST5[0]), "-o", str(tmp_path), "-S", "ecoli", "--device_merge"])
    payload, err = cli.revise_part(args, eng, os.path.basename(FAST5[0]), 1, 3)
    assert err is None and len(payload["a1"]) > 0 and [x[0] for x in eng.log] == ["predict_reads_raw"]


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_failures_end_where_they_ended_before(tmp_path, monkeypatch, fmt):
    """A read the native writer cannot write goes to `fallback` (original basecalls, listed as failed); a call that fails in its
    second half is retried read by read on the host merge.  Files, failed-reads file and exit code are those of the switch off."""
    _env(monkeypatch)
    d = _inputs(tmp_path)

    def misdirect(real, at):
        def f(*a):
            a = list(a)
            a[at] = [os.path.join(os.path.dirname(x), "no_such_dir", "x") if "r07_out" in x else x for x in a[at]]
            return real(*a)
        return f
    monkeypatch.setattr(hostlib, "finish_bundle", misdirect(hostlib.finish_bundle, 7))
    monkeypatch.setattr(hostlib, "write_records", misdirect(hostlib.write_records, 4))
    _, off, rc_off = _run(tmp_path, "w_off", d, ["-F", fmt])
    _, on, rc_on = _run(tmp_path, "w_on", d, ["-F", fmt, "--device_merge"])
    assert off["failed_reads.txt"].split() == [b"r07.fast5"] and on == off and rc_on == rc_off and len(on) == 13
    monkeypatch.undo()
    _env(monkeypatch)
    code, o = hostlib.load_fast5(os.path.join(d, "r04.fast5"), "Basecall_1D_000", "BaseCalled_template", False)
    assert code == hostlib.OK
    marker = o["feat"][0].copy()
    _, off, rc_off = _run(tmp_path, "e_off", d, ["-F", fmt], eng=MergingEcho(fail_marker=marker, fail_in_end=True))
    eng, on, rc_on = _run(tmp_path, "e_on", d, ["-F", fmt, "--device_merge"], eng=MergingEcho(fail_marker=marker, fail_in_end=True))
    assert on == off and rc_on == rc_off and not eng.violations
    assert ("begin", 12, False) in eng.log and any(w == "predict_reads_raw" for w, _, _ in eng.log)      # the retry is host-fed
