"""The single-file output on the host (CPU only): hoststage.pack_records - the definition the kernels of csrc/nrv_pack.h are held
to - and the command line's --combined.  Nothing here has a tolerance: every comparison is bytes or integers.

  (a) the definition against a plain per-read Python loop written from the rule text (tests/records_cases.py; it shares no code
      with hoststage) on report_cases.report_case(), FASTQ and FASTA; rec_off is monotone and ends at the capacity formula's value
      minus the slack that deletions leave;
  (b) edge shapes: no read, only empty reads, names of 1 / 3 / 4 / 5 / 15 / 16 / 17 / 255 bytes and one with `|||`, 600 reads of
      0 - 40 bases in one call;
  (c) each record parses back into name / seq / qual, and the .fai columns computed for it address exactly those bytes;
  (d) --combined with stand-in engines on the fixture fast5 files: the set of records is, read by read, what the per-read files of
      a run without the switch hold, for 1 and 3 workers (reads split over workers among them), pipelined and staged calls, and a
      stand-in for the device route; a fallback read and a lost worker's reads are in FILE exactly once; no *_out.* file;
      FILE.fai addresses every record; --report / --edits are byte-identical; without --combined no FILE, no parts, and the
      per-read files are what the writers have always written; --resume --combined exits 2;
  (e) a part whose last record is cut short and a part whose read the parent rewrote: each read once, the index right, no stray
      bytes; one clean part is renamed;
  (f) `_route_batch`: the rows of --combined.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD, load_read
from nanoreviser_amd import cli, hostlib
from nanoreviser_amd import hoststage as hs
from echo_engine import HashEngine, dying_midway_factory, hash_factory
from records_cases import EDGE_CASES, NAME_LENS, fai_lines, loop_records, parse_records, report_records_case
from report_cases import T
from test_revision_edits_host import PackedHash

FAST5 = sorted(glob.glob(os.path.join(GOLD, "fast5", "*.fast5")))


def _check(c, what):
    blob, rec_off = hs.pack_records(c["names"], c["seq"], c["qual"], c["off"])
    assert blob.dtype == np.uint8 and rec_off.dtype == np.int64 and rec_off.shape == (len(c["names"]) + 1,), what
    want, want_off = loop_records(c["names"], c["seq"], c["qual"], c["off"])
    assert rec_off.tolist() == want_off and blob.tobytes() == want, what
    return blob, rec_off


# ---- (a) the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fastq", [True, False])
def test_pack_records_equals_the_rule_text(fastq):
    c = report_records_case(fastq)
    blob, rec_off = _check(c, fastq)
    R, calls = len(c["names"]), c["calls"]
    assert calls["ev_len"][0] == 0 and calls["ev_len"][-1] == 0 and 0 in calls["ev_len"][1:-1].tolist() and calls["ev_len"][1] == 256
    assert (np.diff(rec_off) > 0).all() and rec_off[0] == 0
    q = 2 if fastq else 1
    cap = sum(len(n) for n in c["names"]) + q * (calls["N"] + max(calls["N"] - T, 0)) + 3 * q * R
    slack = q * (calls["N"] + calls["n"] - int(c["off"][-1]))             # characters the deletions (and the single emissions) leave unused
    assert slack > 0 and rec_off[-1] == cap - slack == len(blob)
    # S1-free inputs of other integer types are the same records
    b2, o2 = hs.pack_records(c["names"], c["seq"].tolist(), None if c["qual"] is None else c["qual"].tolist(), c["off"].tolist())
    assert b2.tobytes() == blob.tobytes() and np.array_equal(o2, rec_off)
    with pytest.raises(ValueError):
        hs.pack_records(c["names"][:-1], c["seq"], c["qual"], c["off"])


# ---- (b) edge shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fastq", [True, False])
@pytest.mark.parametrize("what", sorted(EDGE_CASES))
def test_edge_shapes(what, fastq):
    c = EDGE_CASES[what](fastq)
    blob, rec_off = _check(c, (what, fastq))
    if what == "no reads":
        assert len(blob) == 0 and rec_off.tolist() == [0]
    if what == "empty reads":
        assert bytes(blob) == b"".join((b"@" if fastq else b">") + n + (b"\n\n+\n\n" if fastq else b"\n\n") for n in c["names"])
    if what == "name lengths":
        assert {len(n) for n in c["names"]} == set(NAME_LENS) and any(b"|||" in n for n in c["names"])
    if what == "600 tiny reads":
        L = np.diff(c["off"])
        assert len(L) == 600 and L.min() == 0 and L.max() == 40


# ---- (c) parsing back, and the index -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fastq", [True, False])
def test_records_parse_back_and_the_index_addresses_them(fastq):
    for c in [report_records_case(fastq)] + [EDGE_CASES[k](fastq) for k in sorted(EDGE_CASES)]:
        blob, rec_off = hs.pack_records(c["names"], c["seq"], c["qual"], c["off"])
        recs = parse_records(blob, fastq)
        assert len(recs) == len(c["names"])
        raw = blob.tobytes()
        lines = fai_lines(c["names"], c["off"], rec_off, fastq, base=1000)
        for r, (name, s, ql) in enumerate(recs):
            lo, hi = int(c["off"][r]), int(c["off"][r + 1])
            assert name == c["names"][r] and s == c["seq"][lo:hi].tobytes()
            assert (ql is None) if not fastq else (ql == c["qual"][lo:hi].tobytes())
            # the project's own index line for the record, against the loop's, and against the bytes
            assert cli._fai_line(name, hi - lo, 1000 + int(rec_off[r]), fastq).decode() == lines[r] + "\n"
            col = lines[r].split("\t")
            o = int(col[2]) - 1000
            assert col[0] == name.decode() and int(col[1]) == hi - lo == int(col[3]) == int(col[4]) - 1
            assert raw[o:o + hi - lo] == s and raw[o - 1:o] == b"\n" and raw[o + hi - lo:o + hi - lo + 1] == b"\n"
            if fastq:
                qo = int(col[5]) - 1000
                assert raw[qo:qo + hi - lo] == ql and raw[qo - 3:qo] == b"\n+\n"
            assert cli._fai_record([name] + col[1:], fastq) == (int(rec_off[r]) + 1000, int(rec_off[r + 1] - rec_off[r]))


# ---- (d) the command line ----------------------------------------------------------------------------------------------------------
class DeviceHash(PackedHash):
    """PackedHash with the merge / report / edits / records forms of engine.Reviser, answered from the host definitions: what the
    command line's device route drives.  Counts the uses of `with_device_records`."""
    records_used = 0

    def __init__(self):
        super().__init__()
        self.forms = []

    @staticmethod
    def _reviser():
        from nanoreviser_amd.engine import Reviser
        return Reviser

    @classmethod
    def with_device_merge(cls, *a, **kw):
        return cls._reviser().with_device_merge(*a, **kw)

    @classmethod
    def with_device_report(cls, *a, **kw):
        return cls._reviser().with_device_report(*a, **kw)

    @classmethod
    def with_device_edits(cls, *a, **kw):
        return cls._reviser().with_device_edits(*a, **kw)

    @classmethod
    def with_device_records(cls, *a, **kw):
        DeviceHash.records_used += 1
        return cls._reviser().with_device_records(*a, **kw)

    def run_packed_raw(self, packed):
        self.forms.append(len(packed))
        if len(packed) <= 9:
            return super().run_packed_raw(packed)
        self.packed_calls += 1
        p1, p2, a1, a2 = HashEngine.predict_read(self, None, packed[2])
        b, thr, descs, nr = packed[9], packed[10], packed[3], packed[4]
        el = [descs[r].ev_len for r in range(nr)]
        qc = cli.phred_chars(p1, p2, a1, a2) if thr is not None else None
        seq, qual, off = hs.emit_calls(b, el, a1, a2, qc, self.T)
        out = (seq, qual, off)
        if len(packed) >= 14:
            out += (hs.revision_report(b, el, a1, a2, p1, p2, qc, self.T, packed[12]) if packed[13] is not None else None,)
        if len(packed) >= 16:
            out += tuple(hs.revision_edits(b, el, a1, a2, p1, p2, qc, self.T)) if packed[15] is not None else (None, None)
        if len(packed) == 20:
            names = [packed[16][packed[17][r]:packed[17][r + 1]].tobytes() for r in range(nr)]
            out += tuple(hs.pack_records(names, seq, qual, off))
            if packed[11][0] is None:
                out = (None, None) + out[2:]
        return out

    def begin_packed_raw(self, packed):
        self.begun += 1
        self.packed_calls -= 1
        out = self.run_packed_raw(packed)
        return (self.begun, out, "merged") if len(packed) > 9 else (self.begun, out)


def _many(tmp_path, copies):
    d = tmp_path / "in"
    d.mkdir()
    for i in range(copies):
        shutil.copy(FAST5[i % 2], d / f"r{i:02d}_{'AB'[i % 2]} x.fast5")   # a blank in the name: `|||` in the record's
    return str(d)


def _per_read(out, fmt):
    """{record name: (seq, qual | None)} of a run's per-read files: the second line, and the text behind `+\\n`."""
    recs = {}
    for f in sorted(os.listdir(out)):
        if "_out." not in f:
            continue
        text = open(out + f, "rb").read()
        head, rest = text.split(b"\n", 1)
        assert head[:1] == (b"@" if fmt == "fastq" else b">") and rest.count(b"\n") == (1 if fmt == "fastq" else 0)
        if fmt == "fastq":
            seq, qual = rest.split(b"+\n", 1)
            recs[head[1:]] = (seq, qual)
        else:
            recs[head[1:]] = (rest, None)
    return recs


def _combined(path, fmt):
    """{record name: (seq, qual | None)} of FILE: every read once, every record addressed by FILE.fai, no parts left."""
    fastq = fmt == "fastq"
    blob = open(path, "rb").read()
    recs = parse_records(blob, fastq)
    names = [n for n, _, _ in recs]
    assert len(set(names)) == len(names), "a read has two records"
    off = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in recs])]).astype(np.int64)
    rec_off = np.concatenate([[0], np.cumsum([len(n) + (2 if fastq else 1) * len(s) + (6 if fastq else 3) for n, s, _ in recs])]).astype(np.int64)
    assert rec_off[-1] == len(blob)
    assert open(path + ".fai").read().split("\n") == fai_lines(names, off, rec_off, fastq) + [""]
    assert not glob.glob(glob.escape(path) + "*part*") and not glob.glob(glob.escape(path) + "*.tmp*")
    return {n: (s, q) for n, s, q in recs}


def _tree(d):
    return {os.path.relpath(os.path.join(r, f), d): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(d) for f in fs}


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_combined_holds_the_records_of_the_per_read_files(tmp_path, monkeypatch, fmt):
    import __graft_entry__ as g
    g.build_host()
    assert hostlib.load() is not None
    src = _many(tmp_path, 6)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                           # several device calls for these reads
    for k in ("NRV_COMBINED", "NRV_EDITS", "NRV_REPORT", "NRV_DEVICE_MERGE", "NRV_DEVICE_STATS", "NRV_CLI_ENGINES"):
        monkeypatch.delenv(k, raising=False)
    want_qual = fmt == "fastq"

    def run(tag, combined=True, extra=(), rc=0, **kw):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "-F", fmt, "--thread", "2", "--batch", "1024", "--split_reads_above", "0.2",
                "--report", out + "rep.tsv", "--edits", out + "ed"] + list(extra)
        assert cli.main(argv + (["--combined", out + "sub/all." + fmt] if combined else []), **kw) == rc
        assert not [f for f in os.listdir(out) if ".tmp" in f]
        assert bool([f for f in os.listdir(out) if "_out." in f]) == (not combined)
        return out

    # without --combined: no FILE, no parts, and the per-read files the writers have always written
    plain = run("plain", combined=False, worker_factory=hash_factory, world=1)
    assert not os.path.exists(plain + "sub") and sorted(f for f in os.listdir(plain) if "_out." not in f) == ["ed", "failed_reads.txt", "rep.tsv"]
    want = _per_read(plain, fmt)
    assert len(want) == 6 and all(b"|||" in n for n in want)
    names = sorted(os.listdir(src))
    for k in (0, 1):
        _, rd, rt = load_read("_".join(os.path.basename(FAST5[k]).split("_")[-3:-1]))
        seq, qual = cli._finish_read(T, rt, *HashEngine().predict_read(None, rt.feat_ev), want_qual=want_qual)
        text = hs.fastq_record(names[k], list(seq), list(qual)) if want_qual else hs.fasta_record(names[k], list(seq))
        assert open(cli.out_name(plain, names[k], fmt), "rb").read() == text.encode()
        assert want[hs.record_name(names[k])] == (seq.encode(), qual.encode() if want_qual else None)

    def same(out):
        assert _combined(out + "sub/all." + fmt, fmt) == want, out
        assert open(out + "rep.tsv", "rb").read() == open(plain + "rep.tsv", "rb").read(), out
        assert _tree(out + "ed") == _tree(plain + "ed"), out
        assert sorted(os.listdir(out)) == ["ed", "failed_reads.txt", "rep.tsv", "sub"] and sorted(os.listdir(out + "sub")) == ["all." + fmt, "all." + fmt + ".fai"]

    same(run("one", worker_factory=hash_factory, world=1))
    same(run("three", worker_factory=hash_factory, world=3))             # the fixture reads are split over the workers
    monkeypatch.setenv("NRV_CLI_PIPELINE", "1")
    eng_p = PackedHash()
    same(run("piped", reviser_factory=lambda a, dev: eng_p))
    monkeypatch.setenv("NRV_CLI_PIPELINE", "0")
    eng_s = PackedHash()
    same(run("staged", reviser_factory=lambda a, dev: eng_s))
    assert eng_p.begun >= 2 and eng_s.begun == 0 and eng_s.packed_calls >= 2
    # the device route with a stand-in for the engine's record calls: the blobs are appended as they come, no native writer runs
    monkeypatch.setenv("NRV_CLI_PIPELINE", "1")
    monkeypatch.setattr(cli, "_write_records_native", lambda *a, **kw: pytest.fail("a native writer ran"))
    monkeypatch.setattr(cli, "_finish_bundle_native", lambda *a, **kw: pytest.fail("a native writer ran"))
    eng_d, used = DeviceHash(), DeviceHash.records_used
    same(run("dev", extra=["--device_merge"], reviser_factory=lambda a, dev: eng_d))
    assert eng_d.forms and set(eng_d.forms) == {20} and DeviceHash.records_used - used == len(eng_d.forms)
    # reads whose window range is split over the workers: the parent forms the record from the merged slices
    gold = os.path.dirname(FAST5[0])
    whole, split = str(tmp_path / "whole") + "/", str(tmp_path / "split") + "/"
    assert cli.main(["-d", gold, "-o", whole, "-S", "ecoli", "-F", fmt, "--thread", "1", "--combined", whole + "all"],
                    reviser_factory=lambda a, dev: HashEngine()) == 0
    assert cli.main(["-d", gold, "-o", split, "-S", "ecoli", "-F", fmt, "--thread", "1", "--split_reads_above", "0.2", "--combined", split + "all"],
                    worker_factory=hash_factory, world=3) == 0
    assert _combined(split + "all", fmt) == _combined(whole + "all", fmt)
    assert sorted(_combined(whole + "all", fmt).values()) == sorted(want[hs.record_name(names[k])] for k in (0, 1))
    assert sorted(os.listdir(split)) == ["all", "all.fai", "failed_reads.txt"]


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_fallback_and_lost_workers_are_in_the_file_exactly_once(tmp_path, monkeypatch, fmt):
    src = _many(tmp_path, 6)
    monkeypatch.delenv("NRV_COMBINED", raising=False)
    _, rdA, rtA = load_read("_".join(os.path.basename(FAST5[0]).split("_")[-3:-1]))
    eng = HashEngine()

    def failing(sig_ev, feat_ev, real=eng.predict_read):
        if np.array_equal(feat_ev[0], rtA.feat_ev[0]):
            raise RuntimeError("injected engine failure")
        return real(sig_ev, feat_ev)
    runs = {}
    for tag, combined in (("files", False), ("one", True)):
        eng.predict_read = failing
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "-F", fmt, "--thread", "2", "-e", "bad.txt", "--report", out + "rep.tsv"]
        assert cli.main(argv + (["--combined", out + "all"] if combined else []), reviser_factory=lambda a, dev: eng) == 0
        runs[tag] = out
    failed = set(open(runs["one"] + "bad.txt").read().split("\n")) - {""}
    assert "r00_A x.fast5" in failed and failed == set(open(runs["files"] + "bad.txt").read().split("\n")) - {""}
    want = _per_read(runs["files"], fmt)
    got = _combined(runs["one"] + "all", fmt)
    assert got == want and len(got) == 6 and not [f for f in os.listdir(runs["one"]) if "_out." in f]
    orig = hostlib.bases_u8(rdA.bases).tobytes()
    seq = got[hs.record_name("r00_A x.fast5")][0]
    assert fmt == "fastq" or seq == orig                                 # the original basecalls (FASTQ: the fast5's own record, trimmed)
    assert open(runs["one"] + "rep.tsv", "rb").read() == open(runs["files"] + "rep.tsv", "rb").read()   # the unrevised row: what was written
    # a worker that dies inside its first call: the parent writes its reads unrevised, each read once
    for tag, combined in (("lost_files", False), ("lost_one", True)):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "-F", fmt, "--thread", "1", "--report", out + "rep.tsv"]
        assert cli.main(argv + (["--combined", out + "all"] if combined else []), worker_factory=dying_midway_factory, world=2) == 3
        runs[tag] = out
    lost = _combined(runs["lost_one"] + "all", fmt)
    assert lost == _per_read(runs["lost_files"], fmt) and len(lost) == 6
    assert open(runs["lost_one"] + "rep.tsv", "rb").read() == open(runs["lost_files"] + "rep.tsv", "rb").read()


def test_flag_parsing(monkeypatch, capsys):
    monkeypatch.delenv("NRV_COMBINED", raising=False)
    assert cli.get_args(["-d", "x"]).combined is None
    assert cli.get_args(["-d", "x", "--combined", "f.fa"]).combined == "f.fa"
    with pytest.raises(SystemExit) as e:
        cli.get_args(["-d", "x", "--combined", "f.fa", "--resume"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--resume" in err and "--combined" in err and err.count("\n") == 1
    monkeypatch.setenv("NRV_COMBINED", " envfile ")
    assert cli.get_args(["-d", "x"]).combined == "envfile"
    with pytest.raises(SystemExit) as e:
        cli.get_args(["-d", "x", "--resume"])
    assert e.value.code == 2
    # no per-read creates: nothing to probe, whatever the run's size
    monkeypatch.setenv("NRV_OUTPUT_PROBE", "1")
    monkeypatch.setattr(cli, "probe_rename_rate", lambda *a, **kw: pytest.fail("the output directory was probed"))
    assert cli.check_output_rate(cli.get_args(["-d", "x"]), 8, 10000) is None


# ---- (e) the parts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fastq", [True, False])
def test_merging_the_parts(tmp_path, fastq):
    rng = np.random.default_rng(4)

    def read(n):
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes().decode()
        return s, "".join(chr(c) for c in rng.integers(34, 74, n))
    reads = {f"r{i} a.fast5": read(n) for i, n in enumerate([5, 0, 17, 4, 9])}
    fns = sorted(reads)
    dst = str(tmp_path / "out" / "all")
    # part 0: three reads in one call, then a record cut short: its bytes without an index line, and half an index line
    p0 = cli.CombinedPart(cli.combined_part_path(dst, 0), fastq)
    seqs = "".join(reads[f][0] for f in fns[:3])
    off = np.concatenate([[0], np.cumsum([len(reads[f][0]) for f in fns[:3]])])
    p0.add(fns[:3], np.frombuffer(seqs.encode(), np.uint8), np.frombuffer("".join(reads[f][1] for f in fns[:3]).encode(), np.uint8) if fastq else None, off)
    p0.close()
    with open(cli.combined_part_path(dst, 0), "ab") as fp:
        fp.write(b">r3|||a.fast5\nAC")
    with open(cli.combined_index_part(cli.combined_part_path(dst, 0)), "ab") as fp:
        fp.write(b"r3|||a.fast5\t4\t")
    # part 1: one read; the parent's part: a read of part 0 again (as a lost worker's read is), and the last read
    p1 = cli.CombinedPart(cli.combined_part_path(dst, 1), fastq)
    p1.add_read(fns[3], *reads[fns[3]])
    p1.close()
    again = ("TTTT", "####")
    pp = cli.CombinedPart(cli.combined_part_path(dst, "parent"), fastq)
    pp.add_read(fns[1], *again)
    pp.add_read(fns[4], *reads[fns[4]])
    pp.close()
    assert sorted(os.listdir(tmp_path / "out")) == ["all.fai.part0", "all.fai.part1", "all.fai.partparent", "all.part0", "all.part1", "all.partparent"]
    cli.merge_combined(dst, fastq)
    assert sorted(os.listdir(tmp_path / "out")) == ["all", "all.fai"]
    blob = open(dst, "rb").read()
    recs = parse_records(blob, fastq)                                    # well-formed to the last byte: no stray bytes
    order = [fns[0], fns[2], fns[3], fns[1], fns[4]]                      # ascending rank, the parent's last; the earlier record of r1 is left out
    assert [n for n, _, _ in recs] == [hs.record_name(f) for f in order]
    want = dict(reads)
    want[fns[1]] = again
    for f, (n, s, q) in zip(order, recs):
        assert s.decode() == want[f][0] and (q is None if not fastq else q.decode() == want[f][1])
    off = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in recs])])
    rec_off = np.concatenate([[0], np.cumsum([len(n) + (2 if fastq else 1) * len(s) + (6 if fastq else 3) for n, s, _ in recs])])
    assert open(dst + ".fai").read().split("\n") == fai_lines([n for n, _, _ in recs], off, rec_off, fastq) + [""]
    # one part with nothing to drop: renamed
    one = str(tmp_path / "one" / "all")
    p = cli.CombinedPart(cli.combined_part_path(one, 0), fastq)
    for f in fns:
        p.add_read(f, *reads[f])
    p.close()
    ino = os.stat(cli.combined_part_path(one, 0)).st_ino
    cli.merge_combined(one, fastq)
    assert sorted(os.listdir(tmp_path / "one")) == ["all", "all.fai"] and os.stat(one).st_ino == ino
    assert [n for n, _, _ in parse_records(open(one, "rb").read(), fastq)] == [hs.record_name(f) for f in fns]
    # no part at all: an empty FILE and an empty index
    none = str(tmp_path / "none" / "all")
    cli.merge_combined(none, fastq)
    assert open(none, "rb").read() == b"" and open(none + ".fai", "rb").read() == b""


# ---- (f) routes --------------------------------------------------------------------------------------------------------------------
def test_route_batch_rows_of_combined():
    class Full:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = with_device_records = None

    class NoRecords:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_report = with_device_edits = None

    class NoReport:
        run_packed_raw = begin_packed_raw = with_device_merge = with_device_records = None

    bundle = {"bases": np.zeros(3, "S1"), "meta": np.array([[10, 3, 0., 1.]])}
    route = cli._route_batch
    # without --combined every row is what it was
    assert route(Full, bundle, 1, True, True, True, False) == (12, "pipelined")
    assert route(Full, bundle, 1, True, True, True, True) == (14, "pipelined")
    assert route(Full, bundle, 1, True, True, True, True, edits=True) == (16, "pipelined")
    assert route(Full, bundle, 1, True, True, True, False, combined=False) == (12, "pipelined")
    # with it: one form for the device route, whatever else the call carries
    for report in (False, True):
        for edits in (False, True):
            assert route(Full, bundle, 1, True, True, True, report, edits=edits, combined=True) == (20, "pipelined")
            want = 16 if edits else (14 if report else 12)
            assert route(NoRecords, bundle, 1, True, True, True, report, edits=edits, combined=True) == (want, "pipelined")
    assert route(NoReport, bundle, 1, True, True, True, True, combined=True)[0] == "host-merge"
    assert route(NoReport, bundle, 1, True, True, True, False, combined=True)[0] == 20
    # where --device_merge does not apply, --combined changes no form: the host forms the records
    assert route(Full, bundle, 1, True, True, False, False, combined=True) == (7, "pipelined")
    assert route(Full, {**bundle, "device_stats": 1}, 1, True, True, False, False, combined=True)[0] == 9
    assert route(Full, bundle, 1, False, True, True, False, combined=True) == (20, "packed+finish_bundle")   # taken back by `_host_merge_form`
    assert route(Full, None, 3, True, True, True, False, combined=True)[0] is None
    packed = tuple(range(9)) + (None,) * 11
    assert len(packed) == 20 and cli._host_merge_form(packed) == tuple(range(9))
    assert cli._host_merge_form(tuple(range(7)) + (None,) * 13) == tuple(range(7))
