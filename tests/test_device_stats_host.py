"""Read statistics on the device, the HOST side (no GPU): the loader mode that leaves them out, and the command-line switch.

  * nrvh_load_fast5_ex / nrvh_load_bundle_ex with NRVH_DEVICE_STATS against the plain loaders, on every fixture file and on the
    truncated / corrupted inputs of test_hostlib_fast5.py: the same status codes; raw, starts, bases, feature columns 0, 3, 4, 5
    and last_dur identical; shift / scale / columns 1 - 2 left as zeros with the flag set - except for a read with a base of
    more than 16 384 samples, which comes back unflagged and complete.
  * --device_stats / NRV_DEVICE_STATS: parsing, the help text, and - with an engine that records the calls it receives - that
    the switch off issues exactly the calls of before, that the switch on reaches the pipelined native-bundle path, and that the
    paths that stay host-fed (Python reader, NRV_CLI_PIPELINE=0, several engines, split reads, an engine without the new
    calls) never see the new form.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD
from nanoreviser_amd import cli, h5lite, hostlib
from nanoreviser_amd import hoststage as hs
from echo_engine import PipelinedEcho

FAST5 = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")))
MORE5 = sorted(glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))
G, SG = "Basecall_1D_000", "BaseCalled_template"

pytestmark = pytest.mark.skipif(hostlib.load() is None, reason="libnanorev_host.so not built")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_but_stats(dev, full):
    """`dev` (device-statistics mode) against `full` (plain mode) of one accepted read."""
    assert np.array_equal(dev["raw"], full["raw"]) and np.array_equal(dev["starts"], full["starts"])
    assert np.array_equal(dev["bases"], full["bases"]) and dev["fastq"] == full["fastq"]
    assert np.array_equal(_u32(dev["feat"][:, [0, 3, 4, 5]]), _u32(full["feat"][:, [0, 3, 4, 5]]))
    assert dev["last_dur"] in (3, 5) and dev["last_dur"] == int(round(float(full["feat"][-1, 3]) * 10))
    if dev["device_stats"]:
        assert dev["shift"] == 0.0 and dev["scale"] == 0.0 and not dev["feat"][:, 1:3].any()
    else:
        assert dev["shift"] == full["shift"] and dev["scale"] == full["scale"]
        assert np.array_equal(_u32(dev["feat"]), _u32(full["feat"]))


def _both(path, want_fastq=True):
    return hostlib.load_fast5(path, G, SG, want_fastq), hostlib.load_fast5(path, G, SG, want_fastq, device_stats=True)


def test_abi_version_is_3_and_a_stale_library_is_rejected(monkeypatch):
    lib = hostlib.load()
    assert lib.nrvh_abi_version() == 3

    class Stale:                                                      # a build of the previous header
        class _Version:
            restype = None

            def __call__(self):
                return 2
        nrvh_abi_version = _Version()

        def __init__(self, path):
            pass
    monkeypatch.setattr(hostlib, "_lib", None)
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib.C, "CDLL", Stale)
    assert hostlib.load() is None                                     # not half used: the NumPy path runs


@pytest.mark.parametrize("path", FAST5 + MORE5)
def test_device_stats_loader_equals_the_full_loader_but_for_the_statistics(path):
    for want_fastq in (True, False):
        (rc, full), (rc2, dev) = _both(path, want_fastq)
        assert rc == rc2 == hostlib.OK
        assert dev["device_stats"] is True                            # fixture bases are at most 465 samples long
        _same_but_stats(dev, full)
        # what the device is to fill in is what hoststage defines: the plain loader's numbers
        sh, sc, c1, c2 = hs.stats_columns(dev["raw"], dev["starts"], dev["last_dur"])
        assert sh == full["shift"] and sc == full["scale"]
        assert np.array_equal(_u32(c1), _u32(full["feat"][:, 1])) and np.array_equal(_u32(c2), _u32(full["feat"][:, 2]))


def test_bundle_in_device_stats_mode(tmp_path):
    bad = tmp_path / "broken.fast5"
    bad.write_bytes(b"\x89HDF\r\n\x1a\n" + b"\x00" * 64)
    paths = [FAST5[0], str(bad), MORE5[0], str(tmp_path / "nothing_here.fast5"), FAST5[1]]
    full = hostlib.load_bundle(paths, G, SG, True)
    dev = hostlib.load_bundle(paths, G, SG, True, device_stats=True)
    assert "last_dur" not in full and "device_stats" not in full
    assert list(dev["status"]) == list(full["status"]) == [hostlib.OK, hostlib.UNSUPPORTED, hostlib.OK, hostlib.E_IO, hostlib.OK]
    assert dev["errors"] == full["errors"] and dev["fastq"] == full["fastq"]
    assert list(dev["device_stats"]) == [1, 0, 1, 0, 1] and list(dev["last_dur"]) == [3, 0, 5, 0, 3]
    for k in ("raw", "starts", "bases"):
        assert np.array_equal(dev[k], full[k])
    assert np.array_equal(_u32(dev["feat"][:, [0, 3, 4, 5]]), _u32(full["feat"][:, [0, 3, 4, 5]])) and not dev["feat"][:, 1:3].any()
    assert np.array_equal(dev["meta"][:, :2], full["meta"][:, :2]) and not dev["meta"][:, 2:].any()


def test_truncated_and_corrupted_files_get_the_same_status_in_both_modes(tmp_path):
    """The inputs of test_hostlib_fast5.py::test_wrong_group_and_truncated_files_are_declined_never_guessed."""
    assert hostlib.load_fast5(FAST5[0], "Basecall_1D_007", SG, device_stats=True)[0] == hostlib.UNSUPPORTED
    data = open(FAST5[0], "rb").read()
    rng = np.random.default_rng(5)
    cuts = sorted({8, 96, 2048, len(data) // 2, len(data) - 1} | {int(x) for x in rng.integers(9, len(data) - 1, 40)})
    t = tmp_path / "cut.fast5"
    for n in cuts:
        t.write_bytes(data[:n])
        (rc, full), (rc2, dev) = _both(str(t))
        assert rc == rc2, n
        if rc == hostlib.OK:
            _same_but_stats(dev, full)
        else:
            assert full == dev                                        # the same reason
    flip = bytearray(data)
    for pos in rng.integers(8, 4096, 24):
        flip[int(pos)] ^= 0xFF
    t.write_bytes(bytes(flip))
    (rc, full), (rc2, dev) = _both(str(t))
    assert rc == rc2 and (rc != hostlib.OK or _same_but_stats(dev, full) is None)
    for seed in range(40):                                            # and random corruption anywhere, as the fuzz test does
        r2 = np.random.default_rng(100 + seed)
        m = bytearray(data)
        for pos in r2.integers(8, len(data), 1 + int(r2.integers(16))):
            m[int(pos)] = int(r2.integers(256))
        t.write_bytes(bytes(m))
        (rc, full), (rc2, dev) = _both(str(t))
        assert rc == rc2, seed
        if rc == hostlib.OK:
            _same_but_stats(dev, full)


def _patch_moves(path, dst, first_row, n_rows):
    """A copy of `path` whose (uncompressed) Events rows [first_row, first_row + n_rows) have move = 0."""
    ev = h5lite.read_fast5(path, G, SG)["events"]
    data = bytearray(open(path, "rb").read())
    at = bytes(data).find(ev[:8].tobytes())
    assert at > 0 and bytes(data).find(ev[:8].tobytes(), at + 1) < 0, "Events table not stored plain"
    es, off = ev.dtype.itemsize, ev.dtype.fields["move"][1]
    assert ev.dtype.fields["move"][0] == np.dtype("<i4")
    for r in range(first_row, first_row + n_rows):
        data[at + r * es + off:at + r * es + off + 4] = (0).to_bytes(4, "little")
    open(dst, "wb").write(bytes(data))


def test_a_read_with_a_base_above_16384_samples_is_declined_and_comes_back_complete(tmp_path):
    dst = str(tmp_path / "stalled.fast5")
    _patch_moves(FAST5[0], dst, 3000, 4000)
    (rc, full), (rc2, dev) = _both(dst)
    assert rc == rc2 == hostlib.OK
    assert int(np.diff(full["starts"]).max()) > hostlib.DEVICE_STATS_MAX_BASE
    assert dev["device_stats"] is False and dev["scale"] > 0
    _same_but_stats(dev, full)
    rd, _ = cli.parse_read(dst, G, SG)                                # ... and both are the Python host stage's numbers
    rt = hs.read_tensors_raw(rd)
    assert np.array_equal(_u32(dev["feat"]), _u32(rt.feat_ev)) and dev["shift"] == rt.shift and dev["scale"] == rt.scale
    # just below the cap the read is left to the device
    ok = str(tmp_path / "slow.fast5")
    _patch_moves(FAST5[0], ok, 3000, 1500)
    rc3, dev3 = hostlib.load_fast5(ok, G, SG, True, device_stats=True)
    assert rc3 == hostlib.OK and 3000 < int(np.diff(dev3["starts"]).max()) <= hostlib.DEVICE_STATS_MAX_BASE and dev3["device_stats"] is True
    # in a bundle the declined read sits beside flagged ones
    b = hostlib.load_bundle([FAST5[1], dst, ok], G, SG, False, device_stats=True)
    assert list(b["device_stats"]) == [1, 0, 1] and b["meta"][1, 3] == full["scale"] and not b["meta"][[0, 2], 2:].any()


# ---- the command-line switch ------------------------------------------------------------------------------------------------
class RecordingEngine(PipelinedEcho):
    """PipelinedEcho that knows the packed form with device statistics and writes down every call it receives."""

    def __init__(self):
        super().__init__()
        self.log = []

    @staticmethod
    def with_device_stats(packed, last_dur, on_device):
        from nanoreviser_amd.engine import Reviser
        return Reviser.with_device_stats(packed, last_dur, on_device)

    def _note(self, what, packed):
        raw, st, feat, descs, nr = packed[:5]
        flags = [int(x) for x in packed[8]] if len(packed) == 9 else None
        self.log.append((what, len(packed), flags, [(descs[r].shift, descs[r].scale) for r in range(nr)],
                         bool(np.asarray(feat)[:, 1:3].any())))

    def begin_packed_raw(self, packed):
        self._note("begin", packed)
        return super().begin_packed_raw(packed[:7])

    def run_packed_raw(self, packed):
        self._note("run", packed)
        return super().run_packed_raw(packed[:7])

    def predict_reads_raw(self, raws, starts, feats, shifts, scales):
        self.log.append(("predict_reads_raw", 0, None, list(zip(shifts, scales)), bool(np.concatenate(feats)[:, 1:3].any())))
        return super().predict_reads_raw(raws, starts, feats, shifts, scales)


def _inputs(tmp_path, n=12):
    d = tmp_path / "in"
    d.mkdir()
    src = FAST5 + MORE5
    for i in range(n):
        shutil.copy(src[i % len(src)], d / f"r{i:02d}.fast5")
    return str(d)


def _run(tmp_path, tag, d, extra, eng=None, **kw):
    eng = eng or RecordingEngine()
    out = str(tmp_path / tag) + "/"
    if "worker_factory" in kw:
        assert cli.main(["-d", d, "-o", out, "-S", "ecoli", "--thread", "3"] + extra, **kw) == 0
    else:
        assert cli.main(["-d", d, "-o", out, "-S", "ecoli", "--thread", "3"] + extra, reviser_factory=lambda a, dev: eng) == 0
    return eng, {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}


def _spy_loader(monkeypatch):
    seen = []
    real = hostlib.load_bundle

    def spy(paths, group, subgroup, want_fastq=True, **kw):
        seen.append(dict(kw))
        return real(paths, group, subgroup, want_fastq=want_fastq, **kw)
    monkeypatch.setattr(hostlib, "load_bundle", spy)
    return seen


def test_switch_parsing_and_help(monkeypatch, capsys):
    monkeypatch.delenv("NRV_DEVICE_STATS", raising=False)
    base = ["-d", "x", "-o", "y"]
    assert cli.get_args(base).device_stats is False
    assert cli.get_args(base + ["--device_stats"]).device_stats is True
    for v, want in (("1", True), ("0", False), ("", False), ("yes", True)):
        monkeypatch.setenv("NRV_DEVICE_STATS", v)
        assert cli.get_args(base).device_stats is want, v
    monkeypatch.delenv("NRV_DEVICE_STATS")
    with pytest.raises(SystemExit):
        cli.get_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--device_stats" in text and "NRV_DEVICE_STATS=1" in text and "Off by default" in text
    for path in ("Python fallback reader", "NRV_CLI_PIPELINE=0", "several engines", "split over GPU workers", "16384 samples"):
        assert path in text, path


def test_switch_off_issues_exactly_the_calls_of_before_and_on_reaches_the_pipelined_path(tmp_path, monkeypatch):
    monkeypatch.delenv("NRV_DEVICE_STATS", raising=False)
    monkeypatch.setenv("NRV_CLI_GROUPS", "1")                           # small device calls: several bundles
    monkeypatch.setenv("NRV_CLI_PIPELINE", "1")
    d = _inputs(tmp_path)
    seen = _spy_loader(monkeypatch)
    off, files_off = _run(tmp_path, "off", d, [])
    assert seen and all(kw == {} for kw in seen)                        # hostlib.load_bundle as ever: no new keyword
    assert off.log and all(w == "begin" and n == 7 and fl is None and all(sc > 0 for _, sc in ss) and cols
                           for w, n, fl, ss, cols in off.log)
    assert len(files_off) == 13 and files_off["failed_reads.txt"] == b""
    del seen[:]
    on, files_on = _run(tmp_path, "on", d, ["--device_stats"])
    assert seen and all(kw == {"device_stats": True} for kw in seen)
    assert len(on.log) == len(off.log) and all(w == "begin" and n == 9 and fl and all(fl) and not cols and not np.any(ss)
                                               for w, n, fl, ss, cols in on.log)
    assert files_on == files_off and not on.violations
    del seen[:]
    monkeypatch.setenv("NRV_DEVICE_STATS", "1")                         # the environment form, no flag
    env, files_env = _run(tmp_path, "env", d, [])
    assert [x[:3] for x in env.log] == [x[:3] for x in on.log] and files_env == files_off


def test_host_fed_paths_never_issue_the_new_calls(tmp_path, monkeypatch):
    monkeypatch.delenv("NRV_DEVICE_STATS", raising=False)
    monkeypatch.setenv("NRV_CLI_GROUPS", "1")
    d = _inputs(tmp_path)
    _, ref = _run(tmp_path, "ref", d, [])

    def host_fed(eng):
        return eng.log and all(n in (0, 7) and fl is None and cols and all(sc > 0 for _, sc in ss) for _, n, fl, ss, cols in eng.log)
    seen = _spy_loader(monkeypatch)
    # one call at a time
    monkeypatch.setenv("NRV_CLI_PIPELINE", "0")
    eng, files = _run(tmp_path, "nopipe", d, ["--device_stats"])
    assert host_fed(eng) and files == ref and all(kw == {} for kw in seen)
    monkeypatch.setenv("NRV_CLI_PIPELINE", "1")
    # several engines on the device
    del seen[:]
    made = []
    monkeypatch.setenv("NRV_CLI_ENGINES", "2")
    _, files = _run(tmp_path, "two", d, ["--device_stats"], worker_factory=lambda a, dev: made.append(RecordingEngine()) or made[-1], world=1)
    assert len(made) == 2 and all(host_fed(e) for e in made if e.log) and any(e.log for e in made)
    assert files == ref and all(kw == {} for kw in seen)
    monkeypatch.delenv("NRV_CLI_ENGINES")
    # an engine without the new calls: the loader skipped the statistics, the command line computes them after all
    del seen[:]
    calls = []

    class Old(PipelinedEcho):
        def begin_packed_raw(self, packed):
            calls.append((len(packed), bool(np.asarray(packed[2])[:, 1:3].any()), all(packed[3][r].scale > 0 for r in range(packed[4]))))
            return super().begin_packed_raw(packed)
    _, files = _run(tmp_path, "old", d, ["--device_stats"], eng=Old())
    assert calls and all(c == (7, True, True) for c in calls) and files == ref
    # no pool (sequential reads): the per-read loader, host statistics
    del seen[:]
    eng = RecordingEngine()
    out = str(tmp_path / "seq") + "/"
    assert cli.main(["-d", d, "-o", out, "-S", "ecoli", "--thread", "1", "--device_stats"], reviser_factory=lambda a, dev: eng) == 0
    assert host_fed(eng) and not seen and {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))} == ref
    # the Python fallback reader (no native library)
    monkeypatch.setattr(hostlib, "load", lambda: None)
    eng = RecordingEngine()
    out = str(tmp_path / "py") + "/"
    assert cli.main(["-d", d, "-o", out, "-S", "ecoli", "--thread", "1", "--device_stats"], reviser_factory=lambda a, dev: eng) == 0
    assert host_fed(eng) and {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))} == ref
    monkeypatch.undo()
    # a slice of a read split over GPU workers: the whole read's median, from the host
    eng = RecordingEngine()
    args = cli.get_args(["-d", os.path.dirname(FAST5[0]), "-o", str(tmp_path), "-S", "ecoli", "--device_stats"])
    payload, err = cli.revise_part(args, eng, os.path.basename(FAST5[0]), 1, 3)
    assert err is None and len(payload["a1"]) > 0 and [x[0] for x in eng.log] == ["predict_reads_raw"] and host_fed(eng)


def test_host_statistics_of_a_device_stats_bundle_are_the_plain_loaders(tmp_path):
    """cli._bundle_host_stats (an engine without the new calls, the per-read retries after a failed call): bit for bit what
    the plain loader delivers, for flagged and declined reads alike."""
    dst = str(tmp_path / "stalled.fast5")
    _patch_moves(FAST5[1], dst, 2000, 4000)
    jobs = [(p, os.path.basename(p), G, SG, False) for p in (FAST5[0], dst, MORE5[1])]
    _, full = cli._load_bundle(jobs)
    ent, dev = cli._load_bundle(jobs, True)
    assert list(dev["device_stats"]) == [1, 0, 1] and "device_stats" not in full
    fixed = cli._bundle_host_stats(dev)
    assert "device_stats" not in fixed and "last_dur" not in fixed
    assert np.array_equal(_u32(fixed["feat"]), _u32(full["feat"])) and np.array_equal(fixed["meta"], full["meta"])
    for a, b in zip(cli._bundle_reads(dev), cli._bundle_reads(full)):
        assert a.shift == b.shift and a.scale == b.scale and np.array_equal(_u32(a.feat_ev), _u32(b.feat_ev))
