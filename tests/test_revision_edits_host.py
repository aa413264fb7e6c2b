"""The per-read edit list on the host (CPU only): hoststage.revision_edits - the definition the kernels of csrc/nrv_edits.h are
held to - and the command line's --edits.  Nothing here has a tolerance: integers and copied f32 bits, the records as bytes.

  (a) the definition against a plain per-read, per-window Python loop written from the rule text (tests/edits_cases.py; it shares
      no code with hoststage), on report_cases.report_case(): with qc + rows, with rows only, bare;
  (b) per read, the records of kind 1 / 2 / 3 are columns 5 / 6 / 7 of revision_report;
  (c) a read's records replayed on its original bases give its slice of emit_calls' seq, and seq[off[r] + pos_out] is what
      every record says it is;
  (d) all-deletion, all-insertion, no-edit calls: total == n_win, n_win, 0;
  (e) --edits with stand-in engines: one file per read, each with its header; without it no directory and the same outputs; the
      same files for 1 and 3 workers (reads split over workers among them) and for pipelined and staged calls; a read on the
      fallback path gets the header alone.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD, load_read
from nanoreviser_amd import cli, hostlib
from nanoreviser_amd import hoststage as hs
from echo_engine import EchoEngine, HashEngine, hash_factory
from edits_cases import EDIT_DTYPE, carry_case, density_case, loop_edits, replay
from report_cases import T, report_case

FAST5 = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")))
HEADER = "#pos_in\tpos_out\tkind\tref\talt\tqual\tconf"


@pytest.fixture(scope="module")
def case():
    return report_case()


def _check(c, p, qc):
    p1, p2 = (c["p1"], c["p2"]) if p else (None, None)
    edits, edit_off = hs.revision_edits(c["bases"], c["ev_len"], c["a1"], c["a2"], p1, p2, qc, T)
    assert edits.dtype == hs.EDIT_DTYPE and edits.dtype.itemsize == 16 and edit_off.dtype == np.int64
    blob, want_off = loop_edits(c["bases"], c["ev_len"], c["a1"], c["a2"], p1, p2, qc)
    assert edit_off.tolist() == want_off and len(edits) == want_off[-1]
    assert edits.tobytes() == blob
    return edits, edit_off


# ---- (a) the definition ------------------------------------------------------------------------------------------------------------
def test_revision_edits_equals_the_rule_text(case):
    c = case
    assert hs.EDIT_DTYPE == EDIT_DTYPE and hs.EDIT_DTYPE.names == ("pos_in", "pos_out", "kind", "ref", "alt", "qual", "conf")
    full, off = _check(c, True, c["qc"])
    rows, _ = _check(c, True, None)
    bare, _ = _check(c, False, None)
    assert len(full) > 300 and set(full["kind"].tolist()) == {1, 2, 3}
    assert full["qual"].min() >= 34 and not rows["qual"].any() and not bare["qual"].any() and not bare["conf"].any()
    assert full["conf"].tobytes() == rows["conf"].tobytes() and (full["conf"] > 0).sum() > 300
    for k in ("pos_in", "pos_out", "kind", "ref", "alt"):
        assert np.array_equal(full[k], rows[k]) and np.array_equal(full[k], bare[k])
    for r in range(len(c["ev_len"])):                                    # ascending in pos_in inside every read
        assert (np.diff(full["pos_in"][off[r]:off[r + 1]].astype(np.int64)) > 0).all()
    # S1 bases are the same bases
    e2, o2 = hs.revision_edits(c["bases"].view("S1"), c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], c["qc"], T)
    assert e2.tobytes() == full.tobytes() and np.array_equal(o2, off)
    with pytest.raises(ValueError):
        hs.revision_edits(np.zeros(3, np.uint8), [4], [], [], None, None, None, T)


# ---- (b) the report's columns ------------------------------------------------------------------------------------------------------
def test_kinds_are_the_reports_columns(case):
    c = case
    edits, off = hs.revision_edits(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], c["qc"], T)
    rep = hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], c["qc"], T)
    for r in range(len(c["ev_len"])):
        kinds = edits["kind"][off[r]:off[r + 1]]
        assert [int((kinds == k).sum()) for k in (1, 2, 3)] == rep[r, 5:8].astype(np.int64).tolist(), r
    assert rep[:, 5:8].sum() == len(edits)


# ---- (c) replay --------------------------------------------------------------------------------------------------------------------
def test_replaying_the_records_gives_the_revised_reads(case):
    c = case
    edits, eoff = hs.revision_edits(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], c["qc"], T)
    seq, qual, off = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"], T)
    ev_off = np.cumsum(c["ev_len"]) - c["ev_len"]
    for r, L in enumerate(c["ev_len"].tolist()):
        orig = c["bases"][ev_off[r]:ev_off[r] + L].tobytes()
        mine = edits[eoff[r]:eoff[r + 1]]
        out = seq[off[r]:off[r + 1]]
        assert replay(orig, mine) == out.tobytes(), r
        for e in mine:
            po = int(e["pos_out"])
            assert orig[int(e["pos_in"])] == e["ref"]
            if e["kind"] == 1:
                assert out[po] == e["alt"] != e["ref"] and qual[off[r] + po] == e["qual"]
            elif e["kind"] == 2:
                assert out[po] == e["ref"] and out[po + 1] == e["alt"] and qual[off[r] + po] == qual[off[r] + po + 1] == e["qual"]
            else:
                assert e["alt"] == ord("-") and 0 <= po <= len(out)


# ---- (d) densities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["deletion", "insertion", "none"])
def test_density_cases(what):
    c = density_case(what)
    n_win = max(c["N"] - T, 0)
    edits, off = _check(c, True, c["qc"])
    windows = int(np.maximum(c["ev_len"] - T, 0).sum())                  # only windows whose event lies inside one read's middle revise
    assert off[-1] == {"deletion": windows, "insertion": windows, "none": 0}[what] and off[-1] <= n_win
    if what != "none":
        assert set(edits["kind"].tolist()) == {{"deletion": 3, "insertion": 2}[what]}
    # one read alone: every window of the call revises, total == n_win
    one = density_case(what, ev_len=(700,))
    edits, off = _check(one, True, None)
    assert off.tolist() == [0, {"deletion": one["n"], "insertion": one["n"], "none": 0}[what]] and one["n"] == 700 - T


def test_calls_without_a_window():
    z = np.zeros(0, np.int8)
    for el in ([], [0], [5], [4, 0, 7], [11]):
        N = int(np.sum(el))
        bases = np.frombuffer(b"ACGT" * 4, np.uint8)[:N]
        edits, off = hs.revision_edits(bases, el, z, z, np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32), None, T)
        assert len(edits) == 0 and edits.dtype == hs.EDIT_DTYPE and off.tolist() == [0] * (len(el) + 1)


def test_carry_case_is_what_it_says():
    c = carry_case(True)
    assert c["N"] == 257 * 256 + 3 and len(c["ev_len"]) == 4 and c["ev_len"][1] > 256 * 256
    edits, off = hs.revision_edits(c["bases"], c["ev_len"], c["a1"], c["a2"], None, None, None, T)
    assert off[-1] == int(np.maximum(c["ev_len"] - T, 0).sum()) and (edits["kind"] == 3).all()


# ---- (e) the command line ----------------------------------------------------------------------------------------------------------
class PackedHash(HashEngine):
    """HashEngine with the packed and the two-halves surface of engine.Reviser: what the native host stage drives."""

    def __init__(self):
        super().__init__()
        self.begun = self.packed_calls = 0

    @staticmethod
    def pack_bundle(raw, starts, feat, meta, T):
        from nanoreviser_amd.engine import Reviser
        return Reviser.pack_bundle(raw, starts, feat, meta, T)

    def run_packed_raw(self, packed):
        self.packed_calls += 1
        feat, outs = packed[2], packed[6]
        for o, v in zip(outs, HashEngine.predict_read(self, None, feat)):
            o[...] = v
        return outs

    def begin_packed_raw(self, packed):
        self.begun += 1
        self.packed_calls -= 1
        return self.begun, self.run_packed_raw(packed)

    def end_packed_raw(self, ticket):
        return ticket[1]


def _many(tmp_path, copies):
    d = tmp_path / "in"
    d.mkdir()
    for i in range(copies):
        shutil.copy(FAST5[i % 2], d / f"r{i:02d}_{'AB'[i % 2]}.fast5")
    return str(d)


def _outputs(out):
    return {f: open(out + f, "rb").read() for f in sorted(os.listdir(out)) if "_out." in f}


def _edit_files(d):
    files = {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))}
    assert all(f.endswith("_edits.tsv") for f in files), sorted(files)
    assert all(t.split("\n")[0] == HEADER and t.endswith("\n") for t in files.values())
    return files


def test_edits_with_the_echo_engine(tmp_path):
    src = _many(tmp_path, 4)
    with_, without = str(tmp_path / "with") + "/", str(tmp_path / "without") + "/"
    ed = str(tmp_path / "ed")
    argv = ["-d", src, "-S", "ecoli", "--thread", "2"]
    assert cli.main(argv + ["-o", with_, "--edits", ed], reviser_factory=lambda a, dev: EchoEngine()) == 0
    assert cli.main(argv + ["-o", without], reviser_factory=lambda a, dev: EchoEngine()) == 0
    files = _edit_files(ed)
    assert sorted(files) == [f.split(".")[0] + "_edits.tsv" for f in sorted(os.listdir(src))]
    assert all(t == HEADER + "\n" for t in files.values())              # the echo engine confirms every base
    assert sorted(os.listdir(tmp_path)) == ["ed", "in", "with", "without"]
    assert _outputs(with_) == _outputs(without) and len(_outputs(with_)) == 4
    assert sorted(os.listdir(with_)) == sorted(os.listdir(without))


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_edit_files_do_not_depend_on_workers_or_on_the_call_path(tmp_path, monkeypatch, fmt):
    import __graft_entry__ as g
    g.build_host()
    assert hostlib.load() is not None
    src = _many(tmp_path, 6)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                           # several device calls for these reads
    monkeypatch.delenv("NRV_EDITS", raising=False)
    want_qual = fmt == "fastq"

    def run(tag, edits=True, **kw):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "-F", fmt, "--thread", "2", "--batch", "1024", "--split_reads_above", "0.2"]
        assert cli.main(argv + (["--edits", out + "ed"] if edits else []), **kw) == 0
        assert not [f for f in os.listdir(out) if ".tmp" in f]
        return out

    one = run("one", worker_factory=hash_factory, world=1)
    three = run("three", worker_factory=hash_factory, world=3)
    monkeypatch.setenv("NRV_CLI_PIPELINE", "1")
    eng_p = PackedHash()
    piped = run("piped", reviser_factory=lambda a, dev: eng_p)
    monkeypatch.setenv("NRV_CLI_PIPELINE", "0")
    eng_s = PackedHash()
    staged = run("staged", reviser_factory=lambda a, dev: eng_s)
    assert eng_p.begun >= 2 and eng_s.begun == 0 and eng_s.packed_calls >= 2
    plain = run("plain", edits=False, reviser_factory=lambda a, dev: PackedHash())
    assert not os.path.exists(plain + "ed")
    ref = _edit_files(one + "ed")
    assert len(ref) == 6
    for o in (three, piped, staged):
        assert _edit_files(o + "ed") == ref, o
        assert _outputs(o) == _outputs(one)
    assert _outputs(plain) == _outputs(one) and len(_outputs(one)) == 6

    # a file is the definition on that read's calls, and its lines replay to the read that was written
    names = sorted(os.listdir(src))
    for k in (0, 1):
        _, rd, rt = load_read("_".join(os.path.basename(FAST5[k]).split("_")[-3:-1]))
        calls = HashEngine().predict_read(None, rt.feat_ev)
        edits, off = cli.edit_rows(T, rd.bases, [len(rd.bases)], *calls, want_qual)
        lines = ref[names[k].split(".")[0] + "_edits.tsv"].split("\n")[1:-1]
        assert len(lines) == len(edits) == off[-1] > 100
        for ln, e in zip(lines, edits):
            assert ln == "\t".join([str(e["pos_in"]), str(e["pos_out"]), "SID"[e["kind"] - 1], chr(e["ref"]), chr(e["alt"]),
                                    chr(e["qual"]) if want_qual else ".", format(float(e["conf"]), ".9g")])
        text = open(one + names[k].split(".")[0] + "_out." + fmt).read().split("\n")[1].split("+")[0]
        assert replay(hostlib.bases_u8(rd.bases).tobytes(), edits) == text.encode()
    # reads whose window range is split over the workers: the parent forms the list from the merged slices
    gold = os.path.dirname(FAST5[0])
    whole, split = str(tmp_path / "whole") + "/", str(tmp_path / "split") + "/"
    assert cli.main(["-d", gold, "-o", whole, "-S", "ecoli", "-F", fmt, "--thread", "1", "--edits", whole + "ed"],
                    reviser_factory=lambda a, dev: HashEngine()) == 0
    assert cli.main(["-d", gold, "-o", split, "-S", "ecoli", "-F", fmt, "--thread", "1", "--split_reads_above", "0.2", "--edits", split + "ed"],
                    worker_factory=hash_factory, world=3) == 0
    assert _edit_files(split + "ed") == _edit_files(whole + "ed")
    assert sorted(_edit_files(whole + "ed").values()) == sorted(ref[names[k].split(".")[0] + "_edits.tsv"] for k in (0, 1))


def test_fallback_reads_get_the_header_alone_and_resume_writes_nothing(tmp_path, monkeypatch):
    src = _many(tmp_path, 6)
    _, rdA, rtA = load_read("_".join(os.path.basename(FAST5[0]).split("_")[-3:-1]))
    out = str(tmp_path / "o") + "/"
    ed = str(tmp_path / "ed")
    monkeypatch.setenv("NRV_EDITS", ed)                                 # the environment form of --edits
    eng = HashEngine(fail_marker=None)
    eng.fail_marker = rtA.feat_ev[0]

    def failing(sig_ev, feat_ev, real=eng.predict_read):
        if np.array_equal(feat_ev[0], eng.fail_marker):
            raise RuntimeError("injected engine failure")
        return real(sig_ev, feat_ev)
    eng.predict_read = failing
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "-e", "bad.txt"], reviser_factory=lambda a, dev: eng) == 0
    failed = set(open(out + "bad.txt").read().split())
    files = _edit_files(ed)
    assert failed and "r00_A.fast5" in failed and len(files) == 6
    for fn in sorted(os.listdir(src)):
        text = files[fn.split(".")[0] + "_edits.tsv"]
        assert (text == HEADER + "\n") == (fn in failed), fn
    # --resume: the reads that already have an output are skipped, and nothing is written for them
    ed2 = str(tmp_path / "ed2")
    monkeypatch.setenv("NRV_EDITS", ed2)
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "-e", "bad.txt", "--resume"],
                    reviser_factory=lambda a, dev: HashEngine()) == 0
    files2 = _edit_files(ed2)
    assert sorted(files2) == sorted(f.split(".")[0] + "_edits.tsv" for f in failed)
    assert all(t != HEADER + "\n" for t in files2.values())


def test_edits_flag_parsing_and_routing(monkeypatch):
    monkeypatch.delenv("NRV_EDITS", raising=False)
    assert cli.get_args(["-d", "x"]).edits is None
    assert cli.get_args(["-d", "x", "--edits", "dir"]).edits == "dir"
    monkeypatch.setenv("NRV_EDITS", " envdir ")
    assert cli.get_args(["-d", "x"]).edits == "envdir"

    class Full:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None

    class NoEdits:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = None

    bundle = {"bases": np.zeros(3, "S1"), "meta": np.array([[10, 3, 0., 1.]])}
    assert cli._route_batch(Full, bundle, 1, True, True, True, False)[0] == 12
    assert cli._route_batch(Full, bundle, 1, True, True, True, False, edits=True) == (16, "pipelined")
    assert cli._route_batch(Full, bundle, 1, True, True, True, True, edits=True) == (16, "pipelined")
    assert cli._route_batch(NoEdits, bundle, 1, True, True, True, True, edits=True)[0] == "host-merge"
    assert cli._route_batch(Full, bundle, 1, True, True, False, False, edits=True)[0] == 7
