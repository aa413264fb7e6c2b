"""The per-read revision report on the host (CPU only): hoststage.revision_report - the definition the kernel of
csrc/nrv_report.h is held to - and the command line's --report.

  * the definition against a plain per-read, per-window Python loop written from the rule text (tests/report_cases.py; it
    calls neither emit_calls nor merge_calls): random calls, read lengths {0, 1, 10, 11, 12, 13, 255, 256, 257, 600}, labels
    out of range, softmax rows with an exact tie, a margin one ulp either side of tie_eps, NaNs; the identities between
    the columns; bases_out and q_sum against hoststage.emit_calls;
  * --report with stand-in engines: one line per input, sorted, a #total line; the same bytes for 1 and 3 GPU workers (reads
    split over workers among them) and for pipelined and staged device calls; a read on the fallback path is `unrevised`;
    without --report no file appears and the outputs are the same bytes.
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
from report_cases import T, TIE_EPS, loop_report, report_case

FAST5 = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")))


@pytest.fixture(scope="module")
def case():
    return report_case()


# ---- the definition --------------------------------------------------------------------------------------------------------------
def _identities(rep):
    rep = rep.astype(np.int64)
    assert np.array_equal(rep[:, 4:9].sum(1), rep[:, 1])
    assert np.array_equal(rep[:, 9:15].sum(1), rep[:, 1])
    assert np.array_equal(rep[:, 15:20].sum(1), rep[:, 1])
    assert np.array_equal(rep[:, 2], rep[:, 3] + rep[:, 4] + rep[:, 5] + rep[:, 8] + 2 * rep[:, 6])
    assert np.array_equal(rep[:, 0], rep[:, 1] + rep[:, 3])
    assert not rep[:, 23].any()


def test_revision_report_equals_the_rule_text(case):
    c = case
    assert hs.REPORT_COLS == 24 and len(hs.REPORT_NAMES) == 23 and hs.REPORT_TIE_EPS == TIE_EPS
    assert set(c["ev_len"].tolist()) >= {0, 1, 10, 11, 12, 13, 255, 256, 257, 600}
    rep = hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], c["qc"], T, TIE_EPS)
    assert rep.dtype == np.uint64 and rep.shape == (len(c["ev_len"]), 24)
    want = loop_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], c["qc"])
    assert np.array_equal(rep, want), np.argwhere(rep != want)
    _identities(rep)
    # every class of the merge and every clipped label is populated, so that a swapped column cannot hide
    assert (rep[:, 4:9].sum(0) > 20).all() and (rep[:, 9:20].sum(0) > 20).all() and rep[:, 20].sum() > 100
    # the planted rows: ties, one ulp below tie_eps and the NaNs count; exactly tie_eps and one ulp above do not
    r600 = 10
    assert rep[r600, 21] == 7 and rep[:, 21].sum() == 7
    # bases_out and q_sum are emit_calls'
    seq, qual, off = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"], T)
    assert np.array_equal(rep[:, 2].astype(np.int64), np.diff(off))
    qs = [int((qual[off[r]:off[r + 1]].astype(np.int64) - 33).sum()) for r in range(len(c["ev_len"]))]
    assert rep[:, 22].astype(np.int64).tolist() == qs
    # S1 bases are the same bases
    assert np.array_equal(hs.revision_report(c["bases"].view("S1"), c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], c["qc"], T), rep)


def test_revision_report_without_quality_or_probabilities(case):
    c = case
    full = hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], c["qc"], T, TIE_EPS)
    fasta = hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], None, T, TIE_EPS)
    assert np.array_equal(fasta, loop_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], None))
    assert not fasta[:, 22].any() and np.array_equal(fasta[:, :22], full[:, :22])
    bare = hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], None, None, c["qc"], T, TIE_EPS)
    assert not bare[:, 21].any() and np.array_equal(np.delete(bare, 21, 1), np.delete(full, 21, 1))
    _identities(fasta)
    _identities(bare)
    # another margin moves the near-tie column alone
    wide = hs.revision_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], c["qc"], T, 0.05)
    assert np.array_equal(wide, loop_report(c["bases"], c["ev_len"], c["a1"], c["a2"], c["p1"], c["p2"], c["qc"], tie_eps=0.05))
    assert wide[:, 21].sum() > full[:, 21].sum() and np.array_equal(np.delete(wide, 21, 1), np.delete(full, 21, 1))


def test_revision_report_of_calls_without_a_window():
    for el in ([], [0], [5], [4, 0, 7], [11]):
        N = int(np.sum(el))
        bases = np.frombuffer(b"ACGT" * 4, np.uint8)[:N]
        z = np.zeros(0, np.int8)
        for qc in (None, np.zeros(0, np.uint8)):
            rep = hs.revision_report(bases, el, z, z, np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32), qc, T)
            assert np.array_equal(rep, loop_report(bases, el, z, z, None, None, qc))
            assert rep[:, 0].tolist() == rep[:, 2].tolist() == rep[:, 3].tolist() == list(el)
    with pytest.raises(ValueError):
        hs.revision_report(np.zeros(3, np.uint8), [4], [], [], None, None, None, T)


# ---- the command line ------------------------------------------------------------------------------------------------------------
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


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0] == "name\tstatus\t" + "\t".join(hs.REPORT_NAMES)
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert all(len(r) == 25 for r in rows) and rows[-1][0] == "#total"
    return rows[:-1], rows[-1]


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_report_file_does_not_depend_on_workers_or_on_the_call_path(tmp_path, monkeypatch, fmt):
    import __graft_entry__ as g
    g.build_host()
    assert hostlib.load() is not None
    src = _many(tmp_path, 8)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                           # several device calls for these reads
    want_qual = fmt == "fastq"

    def run(tag, report=True, **kw):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "-F", fmt, "--thread", "2", "--batch", "1024", "--split_reads_above", "0.2"]
        assert cli.main(argv + (["--report", out + "report.tsv"] if report else []), **kw) == 0
        assert not [f for f in os.listdir(out) if ".part" in f or ".tmp" in f]
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
    plain = run("plain", report=False, reviser_factory=lambda a, dev: PackedHash())
    assert not os.path.exists(plain + "report.tsv")
    ref = open(one + "report.tsv", "rb").read()
    for o in (three, piped, staged):
        assert open(o + "report.tsv", "rb").read() == ref, o
        assert _outputs(o) == _outputs(one)
    assert _outputs(plain) == _outputs(one) and len(_outputs(one)) == 8

    rows, total = _table(one + "report.tsv")
    names = sorted(os.listdir(src))
    assert [r[0] for r in rows] == names and all(r[1] == "revised" for r in rows)
    assert total[1] == "revised" and [int(v) for v in total[2:]] == [sum(int(r[2 + k]) for r in rows) for k in range(23)]
    # a line is the definition on that read's calls
    for k in (0, 1):
        _, rd, rt = load_read("_".join(os.path.basename(FAST5[k]).split("_")[-3:-1]))
        calls = HashEngine().predict_read(None, rt.feat_ev)
        want = cli.report_rows(T, rd.bases, [len(rd.bases)], *calls, want_qual, TIE_EPS)[0]
        assert [int(v) for v in rows[k][2:]] == want[:23].tolist()
        text = open(one + names[k].split(".")[0] + "_out." + fmt).read().split("\n")[1].split("+")[0]
        assert int(rows[k][4]) == len(text) and int(rows[k][2]) == len(rd.bases)
        assert (int(rows[k][24]) > 0) == want_qual and int(rows[k][7]) > 0 and int(rows[k][8]) > 0
    # another margin reaches the definition (the hash engine's margins are 0.1 .. 0.98)
    wide = str(tmp_path / "wide") + "/"
    assert cli.main(["-d", src, "-o", wide, "-S", "ecoli", "-F", fmt, "--thread", "2", "--report", wide + "r.tsv", "--report_tie_eps", "0.5"],
                    reviser_factory=lambda a, dev: HashEngine()) == 0
    rows_w, _ = _table(wide + "r.tsv")
    assert all(int(w[23]) > int(r[23]) == 0 and w[:23] == r[:23] and w[24] == r[24] for w, r in zip(rows_w, rows))
    # reads whose window range is split over the workers: the parent reports them from the merged slices
    gold = os.path.dirname(FAST5[0])
    whole, split = str(tmp_path / "whole") + "/", str(tmp_path / "split") + "/"
    assert cli.main(["-d", gold, "-o", whole, "-S", "ecoli", "-F", fmt, "--thread", "1", "--report", whole + "r.tsv"],
                    reviser_factory=lambda a, dev: HashEngine()) == 0
    assert cli.main(["-d", gold, "-o", split, "-S", "ecoli", "-F", fmt, "--thread", "1", "--split_reads_above", "0.2", "--report", split + "r.tsv"],
                    worker_factory=hash_factory, world=3) == 0
    assert open(split + "r.tsv", "rb").read() == open(whole + "r.tsv", "rb").read()
    assert [r[3:] for r in _table(whole + "r.tsv")[0]] == [r[3:] for r in rows[:2]]


def test_report_marks_fallback_and_resumed_reads_unrevised(tmp_path, monkeypatch):
    src = _many(tmp_path, 6)
    _, rdA, rtA = load_read("_".join(os.path.basename(FAST5[0]).split("_")[-3:-1]))
    out = str(tmp_path / "o") + "/"
    monkeypatch.setenv("NRV_REPORT", out + "rep.tsv")                   # the environment form of --report
    eng = EchoEngine(fail_marker=rtA.feat_ev[0])                        # every call that STARTS with a read A fails
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "-e", "bad.txt"], reviser_factory=lambda a, dev: eng) == 0
    failed = set(open(out + "bad.txt").read().split())
    rows, total = _table(out + "rep.tsv")
    assert failed and "r00_A.fast5" in failed and [r[0] for r in rows] == sorted(os.listdir(src))
    n_rev = 0
    for r in rows:
        v = [int(x) for x in r[2:]]
        written = len(open(out + r[0].split(".")[0] + "_out.fasta").read().split("\n")[1])
        assert r[1] == ("unrevised" if r[0] in failed else "revised")
        assert v[2] == written
        if r[0] in failed:
            assert v[0] == v[2] == v[3] == written and not any(v[4:]) and v[1] == 0
        else:                                                           # the echo engine confirms every base
            n_rev += 1
            assert v[4] == v[1] == v[0] - T and v[20] == v[1] and not any(v[5:9])
    assert n_rev >= 1 and int(total[2 + 1]) == sum(int(r[3]) for r in rows if r[1] == "revised")
    # --resume: the reads that already have an output are reported as what lies on disk
    monkeypatch.delenv("NRV_REPORT")
    good = EchoEngine()
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "-e", "bad.txt", "--resume", "--report", out + "rep2.tsv"],
                    reviser_factory=lambda a, dev: good) == 0
    rows2, _ = _table(out + "rep2.tsv")
    assert [r[0] for r in rows2] == [r[0] for r in rows]
    for r, r2 in zip(rows, rows2):
        if r[0] in failed:                                              # revised again by the second run
            assert r2[1] == "revised" and int(r2[6]) == int(r2[3])
        else:                                                           # skipped: its file is all this run knows
            assert r2[1] == "unrevised" and r2[2] == r2[4] == r2[5] == r[4] and not any(int(x) for x in r2[6:])


def test_report_flag_parsing():
    a = cli.get_args(["-d", "x"])
    assert a.report is None and a.report_tie_eps == 4e-4
    a = cli.get_args(["-d", "x", "--report", "r.tsv", "--report_tie_eps", "1e-3"])
    assert a.report == "r.tsv" and a.report_tie_eps == 1e-3
