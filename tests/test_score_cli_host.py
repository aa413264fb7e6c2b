"""--score on the command line, on stand-in engines (CPU): the score file is the same byte for byte on the host routes, on the
--device_merge route (form 36), for 1, 2 and 3 workers with split reads; reads without a labels file, with a stale one and reads
written unrevised get their status; the read files are a plain run's."""
import os

import numpy as np
import pytest

from echo_engine import EchoEngine, HashEngine, hash_factory
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from test_accuracy_host import FAST5, _clean_env, _files, _many
from test_infix_host import _memoised as _memoised_infix
from test_labels_host import LabelsHash, _want_labels

T = 11


class ScoreHash(LabelsHash):
    """LabelsHash with form 36: the call of the form the tuple extends, then the score block by the host definition from the
    same calls."""
    with_device_score = staticmethod(lambda *a, **k: LabelsHash._cls().with_device_score(*a, **k))

    def begin_packed_raw(self, packed):
        if len(packed) != 36:
            return super().begin_packed_raw(packed)
        base = next((size for size, at in ((33, 32), (31, 30), (30, 29), (27, 26), (22, 21), (20, 19), (16, 15), (14, 13)) if packed[at] is not None), 12)
        t, outs, merged = super().begin_packed_raw(tuple(packed[:base]))
        self.forms[-1] = 36
        p1, p2, a1, a2 = HashEngine.predict_read(self, None, packed[2])
        el = [int(d.ev_len) for d in packed[3]]
        block = hs.score_calls(packed[9], el, a1, a2, p1, p2, packed[33], packed[34], self.T)
        return t, tuple(outs) + (None,) * (13 - len(outs)) + (block,), merged


def _labels_dir(tmp_path, names, leave_out, stale):
    """A directory as an earlier --labels run left it: no file for `leave_out`, another read's bases in the file of `stale`."""
    d = str(tmp_path / "labels_from")
    os.makedirs(d)
    for f, body in _want_labels(names, leave_out).items():
        if f.split("_labels")[0] + ".fast5" in stale:
            lines = body.decode().split("\n")
            lines[1] = lines[1][:100] + ("A" if lines[1][100] != "A" else "C") + lines[1][101:]
            body = "\n".join(lines).encode()
        open(os.path.join(d, f), "wb").write(body)
    return d


def _check_structure(text, names, status_of, labels_dir):
    lines = text.decode().split("\n")
    assert lines[0] == cli.SCORE_HEADER and lines[-1] == "" and len(cli.SCORE_HEADER.split("\t")) == 31
    body = [ln.split("\t") for ln in lines[1:1 + len(names)]]
    assert [c[0] for c in body] == sorted(names)
    tot = [0] * 31
    for c in body:
        assert c[1] == status_of[c[0]], c[:2]
        v = [int(c[k]) for k in (2, 3, 4, 5)] + [int(x) for x in c[10:]]
        windows, labelled, ok1, ok2 = v[:4]
        if c[1] != "scored":
            assert labelled == 0 and c[6:10] == ["."] * 4 and not any(v[1:]) and (windows > 0) == (c[1] != "unrevised")
            continue
        lab_lines = open(cli.labels_file(labels_dir, c[0])).read().split("\n")
        head = lab_lines[0].split("\t")
        n, cs, ce = int(head[4]), int(head[9]), int(head[10])
        centre = np.arange(n)
        counted = (centre >= max(cs, 5)) & (centre < min(n - ce, 5 + n - T)) & (np.frombuffer(lab_lines[4].encode(), np.uint8) != ord("0"))
        assert windows == n - T and labelled == int(counted.sum()) and 0 < labelled <= windows
        assert sum(v[4:24]) == labelled and v[24] <= sum(v[8:12]) and ok1 <= labelled and ok2 <= labelled
        assert c[6] == f"{ok1 / labelled:.6f}" and c[7] == f"{ok2 / labelled:.6f}" and float(c[8]) > 0 and float(c[9]) > 0
        for k in (2, 3, 4, 5):
            tot[k] += int(c[k])
        for k in range(10, 31):
            tot[k] += int(c[k])
    t = lines[1 + len(names)].split("\t")
    assert t[:2] == ["#total", "scored"] and [int(t[k]) for k in (2, 3, 4, 5)] == tot[2:6] and [int(x) for x in t[10:]] == tot[10:]
    rest = lines[2 + len(names):-1]
    conf1 = [[int(x) for x in ln.split("\t")[2:]] for ln in rest if ln.startswith("#confusion1\t")]
    conf2 = [[int(x) for x in ln.split("\t")[2:]] for ln in rest if ln.startswith("#confusion2\t")]
    assert np.array(conf1).shape == (6, 6) and np.array(conf2).shape == (5, 5)
    assert np.sum(conf1) == np.sum(conf2) == tot[3] and np.trace(conf1) == tot[4] and np.trace(conf2) == tot[5]
    for tag, ok in (("#calibration1\t", tot[4]), ("#calibration2\t", tot[5])):
        cal = [ln.split("\t") for ln in rest if ln.startswith(tag)]
        assert cal and sum(int(c[2]) for c in cal) == tot[3] and sum(int(c[3]) for c in cal) == ok
        assert [int(c[1]) for c in cal] == sorted({int(c[1]) for c in cal}) and all(1 <= int(c[1]) <= 40 and int(c[2]) > 0 for c in cal)
        for c in cal:
            n, k = int(c[2]), int(c[3])
            assert c[4] == f"{-10.0 * np.log10((n - k + 0.5) / (n + 1)):.2f}"
    counts = [sum(1 for s in status_of.values() if s == k) for k in ("scored", "stale_labels", "no_labels", "unrevised")]
    assert rest[-1] == "#reads\t" + "\t".join(str(x) for x in counts)
    assert len(rest) == 6 + 5 + sum(1 for ln in rest if ln.startswith("#calibration")) + 1


def test_score_file_is_the_same_on_every_route(tmp_path, monkeypatch, capsys):
    import __graft_entry__ as g
    from nanoreviser_amd import hostlib
    g.build_host()
    _clean_env(monkeypatch)
    for k in ("NRV_ERROR_CLASSES", "NRV_INFIX", "NRV_LABELS", "NRV_SCORE", "NRV_LABELS_FROM"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib, "_lib", None)
    assert hostlib.load() is not None
    _memoised_infix(monkeypatch)
    src = _many(tmp_path, 6)
    names = sorted(os.listdir(src))
    lab = _labels_dir(tmp_path, names, (names[1],), (names[4],))
    status = {fn: "scored" for fn in names}
    status[names[1]], status[names[4]] = "no_labels", "stale_labels"
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                           # several device calls for these reads

    def run(tag, extra=(), score=True, **kw):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "--batch", "1024"] + list(extra)
        if score:
            argv += ["--score", out + "score.tsv", "--labels_from", lab]
        assert cli.main(argv, **kw) == 0
        files = _files(out)
        assert not [f for f in files if ".part" in f or ".tmp" in f]
        return files.pop("score.tsv", None), files

    eng_0 = ScoreHash()
    none, plain = run("plain", ["--device_merge"], score=False, reviser_factory=lambda a, dev: eng_0)
    assert none is None and set(eng_0.forms) == {12}                       # the switch off: as it was
    capsys.readouterr()
    eng_p = ScoreHash()
    piped, files = run("piped", reviser_factory=lambda a, dev: eng_p)
    assert files == plain and set(eng_p.forms) == {7}
    assert capsys.readouterr().out.count("--score:") == 1                  # the stale file is announced once
    _check_structure(piped, names, status, lab)
    eng_m = ScoreHash()
    merged, files = run("merged", ["--device_merge"], reviser_factory=lambda a, dev: eng_m)
    assert merged == piped and files == plain and set(eng_m.forms) == {36} and len(eng_m.forms) >= 2
    # an engine without the call: the host stage scores, the same file
    eng_o = LabelsHash()
    old, files = run("old", ["--device_merge"], reviser_factory=lambda a, dev: eng_o)
    assert old == piped and files == plain and set(eng_o.forms) == {7}
    seq_run, files = run("seq", ["--thread", "1"], reviser_factory=lambda a, dev: HashEngine())
    assert seq_run == piped and files == plain
    # the report, the summary and the trim in the same call change nothing of it
    eng_t = ScoreHash()
    more, _ = run("more", ["--device_merge", "--report", str(tmp_path / "rep.tsv"), "--summary", str(tmp_path / "sum.tsv"), "--trim_q", "3"],
                  reviser_factory=lambda a, dev: eng_t)
    assert more == piped and set(eng_t.forms) == {36}
    # FASTQ: the quality does not enter the score
    fq, _ = run("fastq", ["--device_merge", "-F", "fastq"], reviser_factory=lambda a, dev: ScoreHash())
    assert fq == piped


def test_score_file_for_1_2_and_3_workers_split_reads_and_unrevised_reads(tmp_path, monkeypatch):
    from conftest import load_read
    _clean_env(monkeypatch)
    for k in ("NRV_INFIX", "NRV_LABELS", "NRV_SCORE", "NRV_LABELS_FROM"):
        monkeypatch.delenv(k, raising=False)
    _memoised_infix(monkeypatch)
    src = _many(tmp_path, 4)
    names = sorted(os.listdir(src))
    lab = _labels_dir(tmp_path, names, (names[2],), ())
    status = {fn: "scored" for fn in names}
    status[names[2]] = "no_labels"
    outs = {}
    for world, extra in ((1, []), (2, []), (3, ["--split_reads_above", "0.2"])):   # ... the last one: reads split over the workers, merged in the parent
        out = str(tmp_path / f"w{world}") + "/"
        assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "--score", out + "score.tsv", "--labels_from", lab] + extra,
                        worker_factory=hash_factory, world=world) == 0
        outs[world] = open(out + "score.tsv", "rb").read()
        assert not [f for f in os.listdir(out) if ".part" in f]
    _check_structure(outs[1], names, status, lab)
    assert outs[2] == outs[1] and outs[3] == outs[1]
    # reads written unrevised
    _, rdA, rtA = load_read("_".join(os.path.basename(FAST5[0]).split("_")[-3:-1]))
    out = str(tmp_path / "o") + "/"
    eng = EchoEngine(fail_marker=rtA.feat_ev[0])                        # every call that STARTS with a read A fails
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "-e", "bad.txt", "--score", out + "score.tsv", "--labels_from", lab],
                    reviser_factory=lambda a, dev: eng) == 0
    failed = set(open(out + "bad.txt").read().split())
    assert failed and "r00_A.fast5" in failed
    st2 = {fn: ("unrevised" if fn in failed else status[fn]) for fn in names}
    _check_structure(open(out + "score.tsv", "rb").read(), names, st2, lab)
