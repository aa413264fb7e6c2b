"""Per-base training labels on the host (no GPU): hoststage.align_labels / align_columns / label_strings against the references of
tests/labels_cases.py and against the reference's own label code (tests/golden/labels_reference.json), the engine's marshalling of
nrv_align_labels, and the command line's --labels on stand-in engines."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLD
from echo_engine import HashEngine, hash_factory
from infix_cases import revcomp, strip
from infix_cases import reference as infix_reference
from labels_cases import SMALL, TINY, columns_to_labels, definition, enum_columns, loop_columns, planted_cases, reference, strand
from nanoreviser_amd import cli
from nanoreviser_amd import hoststage as hs
from test_accuracy_host import _Recorder, _clean_env, _files, _many
from test_infix_host import InfixHash, _expected_regions, _write_regions
from test_infix_host import _memoised as _memoised_infix


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def test_align_labels_equals_the_references_on_every_planted_pair():
    cases, ref, got = planted_cases(), reference(), definition()
    S = 64 * strip()
    assert len(cases) > 1400 and sum(v is None for v in ref.values()) <= 2
    assert sum(c[4] - c[3] > S for c in cases.values() if ref is not None) >= 30          # more than one stripe, with a reference
    bad = [k for k in cases if ref[k] is not None and ref[k] != got[k][:2]]
    assert not bad, (len(bad), [(k, ref[k][1], got[k][1]) for k in bad[:5]])
    # the tie-break: gaps land left-aligned
    assert got["repeat AAAA / AAA +"] == (bytes([5, 5, 5]), (3, 0, 0, 1, 0, 0, 1), "DMMM")
    assert got["repeat AAA / AAAA +"] == (bytes([1, 5, 5, 5]), (3, 0, 1, 0, 1, 0, 0), "IMMM")
    assert hs.align_columns(b"GAAAAT", b"GAAT", False, 0, 6) == "MDDMMM" and hs.align_columns(b"GAAT", b"GAAAAT", False, 0, 4) == "MIIMMM"
    assert hs.align_columns(b"ATTTTC", b"GAAT", True, 0, 6) == "MDDMMM"                   # the same u on the other strand
    # the sample of the rule text's enumeration form on random tiny pairs over A C G N
    rng = np.random.default_rng(5)
    al = np.frombuffer(b"ACGN", np.uint8)
    for _ in range(600):
        u, s = (al[rng.integers(0, 4, int(rng.integers(0, TINY + 1)))].tobytes() for _ in range(2))
        cols = enum_columns(u, s)
        assert cols == loop_columns(u, s) == loop_columns(u, s, max(len(u), len(s)))
        if u:
            lab, summ = hs.align_labels(u, s, False, 0, len(u))
            assert (lab.tobytes(), tuple(summ.tolist())) == columns_to_labels(u, s, cols), (u, s)
            assert hs.align_columns(u, s, False, 0, len(u)) == "".join("MID"[c] for c in cols)
    assert SMALL >= 300


def test_invariants_on_every_planted_pair():
    cases, got, inf = planted_cases(), definition(), infix_reference()
    seen_lead = seen_trail = 0
    for name, (t, s, rev, st, en) in cases.items():
        lab, summ = np.frombuffer(got[name][0], np.uint8), got[name][1]
        if not t:
            assert summ == (-1,) * 7 and not lab.any() and lab.size == len(s)
            continue
        u, cols = strand(t, rev)[st:en], got[name][2]
        L, n = len(u), len(s)
        match, sub, ins, dele, clip_s, clip_e, lead = summ
        # applying the columns to the read gives u: every M column holds u's next character, every D column is one of u's alone
        i = j = 0
        for c in cols:
            if c == "M":
                hit = u[i] == s[j] and u[i] in b"ACGT"
                assert (lab[j] & 7) == {65: 5, 71: 4, 84: 3, 67: 2}.get(u[i], 0) and bool(lab[j] & 8) == (not hit), (name, j)
                i, j = i + 1, j + 1
            elif c == "I":
                assert (lab[j] & 15) == 1, (name, j)
                j += 1
            else:
                i += 1
        assert (i, j) == (L, n) and cols.count("M") == match + sub and cols.count("I") == ins and cols.count("D") == dele, name
        # (d, M): the edit classes of (u, s) - and, where the bounds are the infix's, the infix line's dist and match
        d, M = hs.edit_classes(u, s)
        assert (match, sub + ins + dele) == (M, d), name
        if name in inf:
            assert inf[name][:2] == (d, M) and lead == 0 and not cols.endswith("D"), name
        # the counts of the bytes are the summary
        code = lab & 7
        assert int((code == 1).sum()) == ins and int(((lab & 8) != 0).sum()) == sub and int(((code != 1) & ((lab & 8) == 0)).sum()) == match
        assert n == match + sub + ins and L == match + sub + dele
        diag = np.flatnonzero(code != 1)
        assert (clip_s, clip_e) == ((int(diag[0]), n - 1 - int(diag[-1])) if diag.size else (n, 0)), name
        runs = [len(r) for r in cols.lstrip("D").replace("M", "I").split("I") if r]
        assert lead == len(cols) - len(cols.lstrip("D")) and int(((lab & 16) != 0).sum()) == len(runs) and sum(runs) + lead == dele, name
        seen_lead, seen_trail = seen_lead + (lead > 0), seen_trail + cols.endswith("D")
    assert seen_lead >= 10 and seen_trail >= 6


def test_degenerate_inputs_and_errors():
    lab, summ = hs.align_labels(b"ACGTACGT", b"", False, 2, 7)
    assert lab.size == 0 and lab.dtype == np.uint8 and summ.tolist() == [0, 0, 0, 5, 0, 0, 5] and summ.dtype == np.int64
    lab, summ = hs.align_labels(b"ACGTACGT", b"ACN", True, 3, 3)
    assert lab.tolist() == [1, 1, 1] and summ.tolist() == [0, 0, 3, 0, 3, 0, 0]
    lab, summ = hs.align_labels(b"", b"ACGT", False, 0, 0)
    assert lab.tolist() == [0, 0, 0, 0] and summ.tolist() == [-1] * 7 and hs.align_columns(b"", b"ACGT", False, 0, 0) == ""
    assert hs.align_labels("ACGT", np.frombuffer(b"ACGT", np.uint8), 0, 0, 4)[0].tolist() == [5, 2, 4, 3]
    # the reverse strand: the code is that of the complemented character; any other byte stays and has code 0
    lab, summ = hs.align_labels(b"ACNT", b"AGGT", True, 0, 4)
    assert lab.tolist() == [5, 0 | 8, 4, 3] and summ.tolist() == [3, 1, 0, 0, 0, 0, 0]
    for st, en in ((-1, 2), (3, 2), (0, 9), (9, 9)):
        with pytest.raises(ValueError, match="bounds"):
            hs.align_labels(b"ACGTACGT", b"ACGT", False, st, en)
    big = np.full(hs.LABELS_MAX_LEN + 1, ord("A"), np.uint8)
    assert hs.LABELS_MAX_LEN == 65536 and hs.LABEL_COLS == 7 == len(hs.LABEL_NAMES)
    with pytest.raises(ValueError, match="65536"):
        hs.align_labels(b"ACGT", big, False, 0, 4)
    with pytest.raises(ValueError, match="65536"):
        hs.align_labels(big, b"ACGT", False, 0, big.size)
    lab, summ = hs.align_labels(big, b"CAGT", False, 1, big.size)         # end - start at the limit: a band of one read's width
    assert summ.tolist() == [1, 3, 0, hs.LABELS_MAX_LEN - 4, 0, 0, hs.LABELS_MAX_LEN - 4] and lab.tolist() == [5 | 8, 5, 5 | 8, 5 | 8]    # the gap lands in front


def test_a_read_of_7000_needs_no_table_of_int64_cells():
    import tracemalloc
    rng = np.random.default_rng(9)
    from accuracy_cases import mutate, random_seq
    t = random_seq(rng, 7000)
    s = mutate(rng, t, 0.08)
    tracemalloc.start()
    lab, summ = hs.align_labels(t, s, False, 0, len(t))
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert peak < 7000 * 7000 * 8 / 8 and int(summ[0] + summ[1] + summ[3]) == 7000 and lab.size == len(s)
    assert summ[0] > 0.85 * 7000


def test_label_strings():
    b = np.array([5, 4, 3, 2, 0 | 8, 1, 5 | 8, 2 | 16, 1 | 16, 3 | 8 | 16, 0 | 8 | 16], np.uint8)
    assert hs.label_strings(b) == ("MMMMXIXDDDD", "54320150000", "54320152130")
    assert hs.label_strings(np.zeros(0, np.uint8)) == ("", "", "")
    assert hs.label_strings(np.frombuffer(bytes([5, 1]), np.uint8)) == ("MI", "51", "51")
    assert (hs.LABEL_SUB, hs.LABEL_DEL) == (8, 16)
    # the codes are the reference's classes (preprocessing.py get_base_label)
    assert [int(hs._LABEL_CODE[ord(c)]) for c in "ACGTN-acgt"] == [5, 2, 4, 3, 0, 0, 0, 0, 0, 0] and hs.BASE_LABEL["-"] == 1 and hs.BASE_LABEL["D"] == 0


# ---- the pin to the reference -----------------------------------------------------------------------------------------------------
def test_labels_equal_the_reference_on_its_own_sam_parsing():
    gold = json.load(open(os.path.join(GOLD, "labels_reference.json")))["cases"]
    assert 35 <= len(gold) <= 60
    seen = {"rev": 0, "D1": 0, "D3": 0, "I": 0, "clip_s": 0, "clip_e": 0, "N": 0}
    for c in gold:
        region, read = c["region"].encode(), c["read"].encode()
        lab, summ = hs.align_labels(region, read, bool(c["reverse"]), c["start"], c["end"])
        n, clip_s, clip_e = len(read), int(summ[4]), int(summ[5])
        mp, l1, l2 = (x[clip_s:n - clip_e] for x in hs.label_strings(lab))
        assert (mp, l1, l2) == (c["mapvals"], c["refvals"], c["refvals2"]), c["name"]
        assert (clip_s, clip_e) == (c["start_clipped_bases"], c["end_clipped_bases"]) and c["readvals"] == c["read"][clip_s:n - clip_e], c["name"]
        assert c["strand"] == "+-"[c["reverse"]] and (c["sam"]["seq"] == (revcomp(read) if c["reverse"] else read).decode())
        # data only, and no equal non-ACGT pair (the reference calls N / N a match)
        cols = hs.align_columns(region, read, bool(c["reverse"]), c["start"], c["end"])
        u = strand(region, c["reverse"])[c["start"]:c["end"]]
        seen["rev"] += c["reverse"]
        seen["D1"] += "MDM" in cols
        seen["D3"] += "DDD" in cols
        seen["I"] += "MIM" in cols or "MIIM" in cols
        seen["clip_s"] += clip_s > 0
        seen["clip_e"] += clip_e > 0
        seen["N"] += b"N" in u and "0" in l2 and "X" in mp
        assert b"N" not in read
    assert all(v >= 3 for v in seen.values()), seen


# ---- the engine's marshalling ------------------------------------------------------------------------------------------------------
def test_align_labels_marshalling():
    from nanoreviser_amd import engine
    from nanoreviser_amd.engine import Reviser
    assert "nrv_align_labels" in engine.SYMBOLS and engine.LABEL_COLS == hs.LABEL_COLS == 7 and engine.LABELS_MAX_LEN == hs.LABELS_MAX_LEN
    assert len(engine._ALIGN_LABELS_T) == 11
    rv = Reviser.__new__(Reviser)
    rv._lib, rv._h = _Recorder(), C.c_void_p(0)
    addr = lambda x: C.cast(x, C.c_void_p).value
    labs, summ = rv.align_labels_device([b"ACGTT", b"", b"AC"], [b"ACG", b"TT", b""], [0, 1, 0], [0, 0, 1], [5, 0, 2])
    (name, args), = rv._lib.calls
    assert name == "nrv_align_labels" and len(args) == 11 and args[5] == 3
    assert [len(x) for x in labs] == [3, 2, 0] and all(x.dtype == np.uint8 for x in labs) and summ.shape == (3, 7) and summ.dtype == np.int64
    as_i64 = lambda p, k: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int64)), (k,)).tolist()
    as_u8 = lambda p, k: bytes(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (k,)))
    assert as_i64(args[2], 4) == [0, 5, 5, 7] and as_i64(args[4], 4) == [0, 3, 5, 5] and as_u8(args[1], 7) == b"ACGTTAC" and as_u8(args[3], 5) == b"ACGTT"
    assert as_u8(args[6], 3) == bytes([0, 1, 0]) and as_i64(args[7], 3) == [0, 0, 1] and as_i64(args[8], 3) == [5, 0, 2]
    assert addr(args[9]) == labs[0].ctypes.data and addr(args[10]) == summ.ctypes.data
    lab, summ = rv.align_labels_arrays(np.zeros(0, np.uint8), [0], np.zeros(0, np.uint8), [0], [], [], [])
    assert lab.size == 0 and summ.shape == (0, 7) and rv._lib.calls[-1][1][5] == 0
    for bad in (lambda: rv.align_labels_device([b"A"], [], [0], [0], [1]), lambda: rv.align_labels_device([b"A"], [b"A"], [0, 1], [0], [1]),
                lambda: rv.align_labels_arrays(b"A", [0, 1], b"A", [0, 1], [0], [0, 0], [1])):
        with pytest.raises(ValueError):
            bad()
    rv._lib = _Recorder(without=("align_labels",))                       # a library without the entry point: found by presence
    for call in (lambda: rv.align_labels_device([b"A"], [b"A"], [0], [0], [1]), lambda: rv.align_labels_arrays(b"A", [0, 1], b"A", [0, 1], [0], [0], [1])):
        with pytest.raises(engine.NrvError, match="this build of libnanorev_hip.so has no nrv_align_labels"):
            call()
    rv._h = None


# ---- the command line --------------------------------------------------------------------------------------------------------------
def test_labels_flag_parsing(monkeypatch, capsys):
    for k in ("NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES", "NRV_INFIX", "NRV_LABELS", "NRV_TRIM_Q"):
        monkeypatch.delenv(k, raising=False)
    base = ["-d", "x", "-o", "y"]
    assert cli.get_args(base).labels is None
    a = cli.get_args(base + ["--truth", "t.fa", "--infix", "i.tsv", "--labels", "lab"])
    assert (a.truth, a.infix, a.labels, a.accuracy) == ("t.fa", "i.tsv", "lab", None)
    monkeypatch.setenv("NRV_LABELS", "envdir")
    assert cli.get_args(base + ["--truth", "t.fa", "--infix", "i.tsv"]).labels == "envdir"
    with pytest.raises(SystemExit) as e:                                  # the environment's switch is refused alone as well
        cli.get_args(base)
    assert e.value.code == 2 and "--labels goes with --truth and --infix" in capsys.readouterr().err
    monkeypatch.delenv("NRV_LABELS")
    for bad, msg in ((["--labels", "lab"], "--labels goes with --truth and --infix"),
                     (["--labels", "lab", "--truth", "t.fa", "--accuracy", "a.tsv"], "--labels goes with --truth and --infix"),
                     (["--labels", "lab", "--infix", "i.tsv"], "--labels goes with --truth and --infix"),
                     (["--labels", "lab", "--truth", "t.fa", "--infix", "i.tsv", "--resume"], "--resume cannot be used with --infix")):
        with pytest.raises(SystemExit) as e:
            cli.get_args(base + bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err, bad


def test_labels_plan_and_index_format():
    W = cli.ACC_WITH_TRUTH
    assert cli.LABELS_HEADER.split("\t") == ["name", "status", "strand", "start", "end", "len", "match", "sub", "ins", "del", "clip_start", "clip_end",
                                            "lead_del"] + [f"label1_{k}" for k in range(6)] + [f"label2_{k}" for k in range(6)]
    assert cli.LABELS_PART_COLS == 24 and cli.labels_file("d", "r01_A.fast5") == os.path.join("d", "r01_A_labels.txt")
    fwd = [100, 2, 97, 95, 12, 85, 2, 99, 60, 30, 0, 90, 3, 92, 1, 96, 50, 40, 5, 95, W]
    rev = [100, 2, 97, 95, 60, 30, 0, 90, 12, 85, 2, 99, 50, 40, 5, 95, 3, 92, 1, 96, W]
    assert cli.labels_plan(fwd, 97) == (W, 0, 2, 99) and cli.labels_plan(rev, 97) == (W, 1, 2, 99)     # the ORIGINAL read's bounds, on the strand picked
    assert cli.labels_plan(fwd, 65537)[0] == cli.ACC_TOO_LONG and cli.labels_plan(fwd, 65536)[0] == W
    wide = [200000, 1, 10, 10, 70000, 0, 5, 65542] + [0] * 12 + [W]
    assert cli.labels_plan(wide, 10)[0] == cli.ACC_TOO_LONG and cli.labels_plan(wide[:7] + [65541] + wide[8:], 10) == (W, 0, 5, 65541)
    for flag in (cli.ACC_NO_TRUTH, cli.ACC_TOO_LONG):
        assert cli.labels_plan([0, 0, 97, 101] + [0] * 16 + [flag], 97) == (flag, 0, 0, 0)


class LabelsHash(InfixHash):
    """InfixHash with nrv_align_labels by the host definition: the device route's plumbing without a device."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.label_calls = []

    def align_labels_arrays(self, a, a_off, b, b_off, reverse, start, end):
        n = len(a_off) - 1
        self.label_calls.append(n)
        a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
        out = [hs.align_labels(a[a_off[k]:a_off[k + 1]], b[b_off[k]:b_off[k + 1]], bool(reverse[k]), start[k], end[k]) for k in range(n)]
        return (np.concatenate([o[0] for o in out]) if out else np.zeros(0, np.uint8)), np.array([o[1] for o in out], np.int64).reshape(n, 7)


_WANT = {}


def _want_labels(names, leave_out=(), too_long=(), forward=False):
    """{file name: bytes} of the labels directory: the definition on the ORIGINAL read at the bounds of tests/test_infix_host.py's
    independent reference tuples, formatted here once more."""
    exp = _expected_regions()
    files, lines, tot, n_reads = {}, [cli.LABELS_HEADER], [0] * 20, [0, 0, 0]
    for i, fn in enumerate(sorted(names)):
        orig, _, region, g = exp[i % 2]
        if fn in leave_out or fn in too_long:
            lines.append("\t".join([fn, "too_long" if fn in too_long else "no_truth", ".", ".", ".", str(len(orig))] + ["."] * 19))
            n_reads[2 if fn in too_long else 1] += 1
            continue
        minus = not forward and (g[1][0], -g[1][1]) < (g[0][0], -g[0][1])
        d, M, st, en = g[1] if minus else g[0]
        key = (i % 2, minus)
        if key not in _WANT:
            _WANT[key] = hs.align_labels(region, orig, minus, st, en)
        lab, summ = _WANT[key]
        assert (int(summ[0]), int(summ[1] + summ[2] + summ[3])) == (M, d) and summ[6] == 0
        mp, l1, l2 = hs.label_strings(lab)
        m = len(region)
        lo, hi = (m - en, m - st) if minus else (st, en)
        v = ["-" if minus else "+", str(lo), str(hi), str(len(orig))] + [str(int(x)) for x in summ]
        files[fn.split(".")[0] + "_labels.txt"] = ("\n".join(["\t".join(["#" + fn] + v), orig.decode(), mp, l1, l2]) + "\n").encode()
        c = [l1.count(str(k)) for k in range(6)] + [l2.count(str(k)) for k in range(6)]
        lines.append("\t".join([fn, "with_truth"] + v + [str(x) for x in c]))
        tot = [a + b for a, b in zip(tot, [len(orig)] + [int(x) for x in summ] + c)]
        n_reads[0] += 1
    lines.append("\t".join(["#total", "with_truth", ".", ".", "."] + [str(x) for x in tot]))
    lines.append("#reads\t" + "\t".join(str(x) for x in n_reads))
    files["labels.tsv"] = ("\n".join(lines) + "\n").encode()
    return files


def test_label_files_are_the_same_on_every_route(tmp_path, monkeypatch, capsys):
    import __graft_entry__ as g
    from nanoreviser_amd import hostlib
    g.build_host()
    _clean_env(monkeypatch)
    for k in ("NRV_ERROR_CLASSES", "NRV_INFIX", "NRV_LABELS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(hostlib, "_tried", False)
    monkeypatch.setattr(hostlib, "_lib", None)
    assert hostlib.load() is not None
    _memoised_infix(monkeypatch)
    exp = _expected_regions()
    src = _many(tmp_path, 6)
    names = sorted(os.listdir(src))
    leave_out = (names[1], names[4])
    fa = _write_regions(str(tmp_path / "regions.fa"), names, leave_out)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                           # several device calls for these reads
    want = _want_labels(names, leave_out)
    assert len(want) == 5 and b"\t-\t" in want["labels.tsv"] and b"\t+\t" in want["labels.tsv"]
    for f, body in want.items():
        if f != "labels.tsv":
            head, bases, mp, l1, l2, last = body.decode().split("\n")
            assert last == "" and len(bases) == len(mp) == len(l1) == len(l2) > 5000 and set(mp) == set("MXID") and set(l1) <= set("012345")

    def run(tag, extra=(), labels=True, **kw):
        out = str(tmp_path / tag) + "/"
        argv = ["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "--batch", "1024", "--truth", fa, "--infix", out + "inf.tsv"] + list(extra)
        if labels:
            argv += ["--labels", out + "lab"]
        assert cli.main(argv, **kw) == 0
        f = _files(out + "lab/") if labels else None
        assert not labels or not [x for x in f if ".part" in x or ".tmp" in x]
        return _files_flat(out), f

    def _files_flat(out):
        return {f: open(out + f, "rb").read() for f in sorted(os.listdir(out)) if os.path.isfile(out + f)}

    eng_0 = LabelsHash()
    plain, none = run("plain", ["--device_merge"], labels=False, reviser_factory=lambda a, dev: eng_0)
    assert none is None and not eng_0.label_calls and not os.path.exists(str(tmp_path / "plain") + "/lab")    # the switch off: as it was
    capsys.readouterr()
    eng_p = LabelsHash()
    piped, lab_p = run("piped", reviser_factory=lambda a, dev: eng_p)
    assert capsys.readouterr().out.count("--labels: the reads are aligned to their truth regions by the host stage") == 1
    assert lab_p == want and piped == plain and not eng_p.label_calls and set(eng_p.forms) == {7}
    eng_m = LabelsHash()
    merged, lab_m = run("merged", ["--device_merge"], reviser_factory=lambda a, dev: eng_m)
    assert "--labels: the reads are aligned" not in capsys.readouterr().out
    assert lab_m == want and merged == plain and set(eng_m.forms) == {33}
    assert len(eng_m.label_calls) == len(eng_m.forms) >= 2 and sum(eng_m.label_calls) == 6             # ONE call per device call
    # an engine with the infix block and without nrv_align_labels: the host stage aligns, the same files
    eng_o = InfixHash()
    old, lab_o = run("old", ["--device_merge"], reviser_factory=lambda a, dev: eng_o)
    assert lab_o == want and old == plain and set(eng_o.forms) == {33}
    seq_run, lab_s = run("seq", ["--thread", "1"], reviser_factory=lambda a, dev: HashEngine())
    assert lab_s == want and seq_run == plain
    # --trim_q and the other truth files next to it change nothing of it
    eng_t = LabelsHash()
    _, lab_t = run("trim", ["--device_merge", "--trim_q", "3", "--accuracy", str(tmp_path / "acc.tsv"), "--error_classes", str(tmp_path / "ecl.tsv")],
                   reviser_factory=lambda a, dev: eng_t)
    assert lab_t == want and set(eng_t.forms) == {33}
    # --infix_strand forward: every read on +, on both routes
    want_f = _want_labels(names, leave_out, forward=True)
    assert b"\t-\t" not in want_f["labels.tsv"] and want_f != want
    for tag, extra in (("fwd_host", []), ("fwd_dev", ["--device_merge"])):
        assert run(tag, extra + ["--infix_strand", "forward"], reviser_factory=lambda a, dev: LabelsHash())[1] == want_f, tag
    # a read that is too long (--accuracy_max_len applies through the infix line): no file, counted too_long; a stale file goes
    lens = [max(len(exp[k][0]), len(exp[k][2])) for k in (0, 1)]
    long_kind = int(np.argmax(lens))
    too_long = [fn for i, fn in enumerate(names) if i % 2 == long_kind and fn not in leave_out]
    want_cut = _want_labels(names, leave_out, too_long)
    assert want_cut["labels.tsv"].decode().split("\n")[-2] == f"#reads\t{6 - 2 - len(too_long)}\t2\t{len(too_long)}"
    for tag, extra in (("cut_host", []), ("cut_dev", ["--device_merge"])):
        os.makedirs(str(tmp_path / tag / "lab"))
        stale = str(tmp_path / tag / "lab" / (too_long[0].split(".")[0] + "_labels.txt"))
        open(stale, "w").write("stale\n")
        assert run(tag, extra + ["--accuracy_max_len", str(min(lens))], reviser_factory=lambda a, dev: LabelsHash())[1] == want_cut, tag
        assert not os.path.exists(stale)


def test_label_files_for_1_2_and_3_workers_split_reads_and_unrevised_reads(tmp_path, monkeypatch):
    from conftest import load_read
    from echo_engine import EchoEngine
    from test_accuracy_host import FAST5
    _clean_env(monkeypatch)
    for k in ("NRV_INFIX", "NRV_LABELS"):
        monkeypatch.delenv(k, raising=False)
    _memoised_infix(monkeypatch)
    src = _many(tmp_path, 4)
    names = sorted(os.listdir(src))
    fa = _write_regions(str(tmp_path / "regions.fa"), names, (names[2],))
    want = _want_labels(names, (names[2],))
    for world, extra in ((1, []), (2, []), (3, ["--split_reads_above", "0.2"])):   # ... the last one: reads split over the workers, merged in the parent
        out = str(tmp_path / f"w{world}") + "/"
        assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "--truth", fa, "--infix", out + "inf.tsv", "--labels", out + "lab"] + extra,
                        worker_factory=hash_factory, world=world) == 0
        assert _files(out + "lab/") == want, world
    # a read written unrevised: its ORIGINAL bases are what was written - the same file
    _, rdA, rtA = load_read("_".join(os.path.basename(FAST5[0]).split("_")[-3:-1]))
    fa = _write_regions(str(tmp_path / "regions2.fa"), names)
    out = str(tmp_path / "o") + "/"
    eng = EchoEngine(fail_marker=rtA.feat_ev[0])                        # every call that STARTS with a read A fails
    assert cli.main(["-d", src, "-o", out, "-S", "ecoli", "--thread", "2", "-e", "bad.txt", "--truth", fa, "--infix", out + "inf.tsv", "--labels", out + "lab"],
                    reviser_factory=lambda a, dev: eng) == 0
    failed = set(open(out + "bad.txt").read().split())
    assert failed and "r00_A.fast5" in failed
    assert _files(out + "lab/") == _want_labels(names)
