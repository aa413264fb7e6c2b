"""Which way a batch of reads goes through the command line (CPU only, echo engines).

  * `cli._route_batch` against the table in its docstring: one case per row, over the engine surfaces the command line meets
    (no packed call; packed; packed in two halves; the device statistics and merge forms; the report form), with and without
    the native thread pool, pipelined or not, --device_merge and --report on and off;
  * one run of `cli.main` per route on six fixture files, told apart by the calls the engine receives and the finisher used.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD
from nanoreviser_amd import cli, hostlib
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd.engine import Reviser
from echo_engine import EchoEngine, PackedEcho, PipelinedEcho
from test_device_merge_host import MergingEcho

FAST5 = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5"))) + sorted(glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))


class ReportingEcho(MergingEcho):
    """MergingEcho that also offers the report form: the rows are hoststage.revision_report on its own echo."""

    @staticmethod
    def with_device_report(packed, tie_eps=None):
        return Reviser.with_device_report(packed, tie_eps)

    def begin_packed_raw(self, packed):
        if len(packed) != 14:
            return super().begin_packed_raw(packed)
        self.log.append(("begin", 14, packed[7] is not None))
        t, out = PipelinedEcho.begin_packed_raw(self, packed[:7])
        return t, (out, packed), "merged"

    def end_packed_raw(self, ticket):
        merged = super().end_packed_raw(ticket)
        if len(ticket) == 2 or len(ticket[1][1]) != 14:
            return merged
        (p1, p2, a1, a2), packed = ticket[1]
        ev_len = [packed[3][r].ev_len for r in range(packed[4])]
        return tuple(merged) + (hs.revision_report(packed[9], ev_len, a1, a2, p1, p2, merged[1], self.T, packed[12]),)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _bundle(stats=False, bases=True):
    b = {"idx": [0, 1], "meta": np.array([[70, 7, 0, 1], [90, 9, 0, 1]], np.float64)}
    if bases:
        b["bases"] = np.frombuffer(b"ACGTACGTACGTACGT", "S1")
    if stats:
        b["device_stats"], b["last_dur"] = np.ones(2, np.uint8), np.array([4, 6], np.int32)
    return b


ENGINES = {"echo": EchoEngine, "packed": PackedEcho, "halves": PipelinedEcho, "merging": MergingEcho, "reporting": ReportingEcho,
           "reviser": lambda: object.__new__(_NoDel)}


class _NoDel(Reviser):
    """The real class' surface (pack_reads_raw and all the forms) without a handle."""
    def __del__(self):
        pass


# engine, bundle (None / "plain" / "stats" / "nobases"), reads, pipelined, native pool, device_merge, report -> form, route
P, B, S, M, PR = "pipelined", "packed+finish_bundle", "packed sliced", "predict_many", "per-read"
ROWS = [
    # reads that arrived one by one
    ("echo", None, 1, 1, 0, 0, 0, "none", PR),
    ("echo", None, 3, 1, 0, 0, 0, "none", M),
    ("merging", None, 3, 1, 1, 1, 1, "none", M),            # no pack_reads_raw: the switches change nothing
    ("reviser", None, 1, 1, 0, 0, 0, "none", PR),
    ("reviser", None, 3, 1, 0, 0, 0, "7", M),
    ("reviser", None, 3, 0, 1, 0, 1, "7", M),
    # a bundle, an engine without the packed call
    ("echo", "plain", 2, 1, 1, 0, 0, "none", M),
    ("echo", "plain", 1, 1, 1, 0, 0, "none", PR),
    ("echo", "plain", 2, 0, 0, 0, 1, "none", M),
    # the packed call in one piece
    ("packed", "plain", 2, 1, 1, 0, 0, "7", B),
    ("packed", "plain", 2, 0, 1, 0, 1, "7", B),
    ("packed", "plain", 2, 1, 0, 0, 0, "7", S),
    ("packed", "nobases", 2, 1, 1, 0, 0, "7", S),
    # ... in two halves
    ("halves", "plain", 2, 1, 1, 0, 0, "7", P),
    ("halves", "plain", 1, 1, 1, 0, 1, "7", P),
    ("halves", "plain", 2, 0, 1, 0, 0, "7", B),
    ("halves", "plain", 2, 1, 0, 0, 0, "7", S),
    ("halves", "plain", 2, 0, 0, 0, 0, "7", S),
    ("halves", "nobases", 2, 1, 1, 0, 0, "7", S),
    ("halves", "plain", 2, 1, 1, 1, 0, "7", P),             # --device_merge, an engine without with_device_merge
    ("halves", "plain", 2, 1, 1, 1, 1, "7", P),
    # the device statistics and the device merge
    ("merging", "plain", 2, 1, 1, 0, 0, "7", P),
    ("merging", "stats", 2, 1, 1, 0, 0, "9", P),
    ("merging", "stats", 2, 1, 1, 0, 1, "9", P),
    ("merging", "plain", 2, 1, 1, 1, 0, "12", P),
    ("merging", "stats", 2, 1, 1, 1, 0, "12", P),
    ("merging", "nobases", 2, 1, 1, 1, 0, "7", S),
    ("merging", "plain", 2, 1, 1, 1, 1, "host-merge", P),   # --report, no with_device_report: the whole bundle on the host
    ("merging", "stats", 2, 1, 1, 1, 1, "host-merge", P),
    ("merging", "plain", 2, 0, 1, 0, 0, "7", B),            # (device_merge is off wherever the run is not pipelined)
    ("merging", "plain", 2, 0, 0, 0, 1, "7", S),
    # the report form
    ("reporting", "plain", 2, 1, 1, 1, 1, "14", P),
    ("reporting", "stats", 2, 1, 1, 1, 1, "14", P),
    ("reporting", "plain", 2, 1, 1, 1, 0, "12", P),
    ("reporting", "plain", 2, 1, 1, 0, 1, "7", P),          # --report without --device_merge: counted on the host
    ("reporting", "nobases", 2, 1, 1, 1, 1, "7", S),
    ("reviser", "stats", 2, 1, 1, 1, 1, "14", P),
    ("reviser", "plain", 2, 0, 1, 0, 0, "7", B),
]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(str(x) for x in r[:7]))
def test_route_table(row):
    eng, kind, n, pipelined, pool, merge, report, form, route = row
    forms = {"none": None, "7": 7, "9": 9, "12": 12, "14": 14, "host-merge": "host-merge"}
    bundle = None if kind is None else _bundle(stats=kind == "stats", bases=kind != "nobases")
    got = cli._route_batch(ENGINES[eng](), bundle, n, bool(pipelined), bool(pool), bool(merge), bool(report))
    assert got == (forms[form], route)


def test_helpers_next_to_the_table():
    assert cli._bundle_has_bases(_bundle()) and not cli._bundle_has_bases(_bundle(bases=False))
    short = _bundle()
    short["bases"] = short["bases"][:-1]
    assert not cli._bundle_has_bases(short)
    assert cli._is_merged_ticket((3, (), "merged")) and not cli._is_merged_ticket((3, ())) and not cli._is_merged_ticket(None)
    plain = Reviser.pack_bundle(np.zeros(160, np.int16), np.arange(16, dtype=np.int32) * 10, np.zeros((16, 6), np.float32), _bundle()["meta"], 11)
    stats = Reviser.with_device_stats(plain, [4, 6], [1, 1])
    for base in (plain, stats):
        merged = Reviser.with_device_merge(base, _bundle()["bases"], False)
        for p in (merged, Reviser.with_device_report(merged, 1e-3)):
            back = cli._host_merge_form(p)
            assert len(back) == len(base) and all(a is b for a, b in zip(back, base))
        assert cli._host_merge_form(base) is base
    assert cli._host_merge_form(None) is None


# ---- one run per route -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six(tmp_path_factory):
    d = tmp_path_factory.mktemp("in")
    for i in range(6):
        shutil.copy(FAST5[i % len(FAST5)], d / f"r{i}.fast5")
    return str(d)


def _main(tmp_path, monkeypatch, d, eng, extra, **env):
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_HOST_THREADS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NRV_CLI_GROUPS", "1")
    monkeypatch.setenv("NRV_CLI_PIPELINE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seen = []
    for name in ("finish_bundle", "finish_read", "write_records"):
        monkeypatch.setattr(hostlib, name, (lambda real, name: lambda *a: seen.append(name) or real(*a))(getattr(hostlib, name), name))
    out = str(tmp_path / "out") + "/"
    assert cli.main(["-d", d, "-o", out, "-S", "ecoli"] + extra, reviser_factory=lambda a, dev: eng) == 0
    files = sorted(os.listdir(out))
    assert len(files) == 7 and open(out + "failed_reads.txt").read() == ""
    return [(m, n) for m, n, _ in eng.log], set(seen)


@pytest.fixture(scope="module", autouse=True)
def _host_library():
    import __graft_entry__ as g
    g.build_host()
    assert hostlib.load() is not None


def test_route_pipelined(tmp_path, monkeypatch, six):
    log, fin = _main(tmp_path, monkeypatch, six, MergingEcho(), ["--thread", "3"])
    assert len(log) >= 2 and set(log) == {("begin", 7)} and fin == {"finish_bundle"}


def test_route_pipelined_device_forms(tmp_path, monkeypatch, six):
    log, fin = _main(tmp_path, monkeypatch, six, MergingEcho(), ["--thread", "3", "--device_stats", "--device_merge"])
    assert len(log) >= 2 and set(log) == {("begin", 12)} and fin == {"write_records"}


def test_route_packed_finish_bundle(tmp_path, monkeypatch, six):
    log, fin = _main(tmp_path, monkeypatch, six, MergingEcho(), ["--thread", "3", "--device_merge"], NRV_CLI_PIPELINE="0")
    assert len(log) >= 2 and set(log) == {("run", 7)} and fin == {"finish_bundle"}


def test_route_packed_sliced(tmp_path, monkeypatch, six):
    monkeypatch.setattr(hostlib, "load_bundle", lambda *a, **k: None)    # bundles put together in Python carry no bases
    log, fin = _main(tmp_path, monkeypatch, six, MergingEcho(), ["--thread", "3"])
    assert len(log) >= 2 and set(log) == {("run", 7)} and fin == {"finish_read"}


def test_route_predict_many(tmp_path, monkeypatch, six):
    eng = MergingEcho()
    log, fin = _main(tmp_path, monkeypatch, six, eng, ["--thread", "1", "--batch", "32768"])
    assert set(log) == {("predict_reads_raw", 0)} and 1 <= len(log) < 6 and eng.calls == len(log)      # several reads per call
    assert not fin                                                       # no pool: merged and written by the finisher thread


def test_route_per_read(tmp_path, monkeypatch, six):
    eng = MergingEcho()
    log, fin = _main(tmp_path, monkeypatch, six, eng, ["--thread", "1"])
    assert log == [("predict_reads_raw", 0)] * 6 and eng.calls == 6 and not fin
