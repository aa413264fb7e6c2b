"""Per-base training labels on the device (MI355X only, -m gpu): csrc/nrv_labels.h through nrv_align_labels and the command line's
--labels.

Everything is compared BIT FOR BIT - label bytes and seven integers per pair, nothing here has a tolerance.
hoststage.align_labels is the definition (tests/test_labels_host.py holds it to two references that share no code with it and to
the reference's own label code through tests/golden/labels_reference.json).  The shipped E. coli weights:
  1. nrv_align_labels on tests/labels_cases.py's planted pairs in ONE call with mixed strands - the infix pairs with the bounds
     the infix found (region lengths on both sides of a strip and of a stripe, up to three stripes, reads across the boundaries,
     empty regions first, in the middle and last) and the label-specific ones (homopolymers, D and I runs across strip, stripe
     and feed-chunk boundaries, bounds that leave leading and trailing D, start == end, n = 0 / 1, L = 1, N and lower case) -
     two passes over one handle; single pairs of one stripe, two stripes, n = 0, no truth;
  2. the same pairs under NRV_LABELS_BUDGET = 300 000 bytes: several batches, the long pairs alone, the same bytes;
  3. null arguments, offsets that do not ascend from 0, a reverse byte of 2, bounds outside the region and a read or an
     end - start above the limit are refused under the entry point's name and the handle stays usable;
  4. handles under NRV_POISON, both patterns, two passes, the pairs of more than one stripe included, with and without batches;
  5. a call in flight: nrv_reads_raw_begin on the two shortest fixture reads, nrv_align_labels, then _end - both results are
     those obtained alone;
  6. the command line: --device_merge --truth --infix --labels on the fixture reads, the regions the seeded mutation between
     flanks of tests/test_gpu_infix.py; the host route's files and index byte for byte; --infix_strand forward.
"""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLD
from labels_cases import definition, planted_cases
from nanoreviser_amd import cli
from test_gpu_device_accuracy import FAST5, PATTERNS, _engine, _eq, _same, short_reads  # noqa: F401
from test_gpu_infix import mutate, random_seq, revcomp, strip     # the regions of the command-line test: that module's own helpers

pytestmark = pytest.mark.gpu

BUDGET = 300000


@pytest.fixture(scope="module")
def planted():
    """(names, regions, reads, reverse, start, end, the definition's bytes joined, its summaries int64[n][7]): computed once."""
    cases, want = planted_cases(), definition()
    names = list(cases)
    cols = list(zip(*(cases[k] for k in names)))
    return (names, list(cols[0]), list(cols[1]), np.array(cols[2], np.uint8), np.array(cols[3], np.int64), np.array(cols[4], np.int64),
            [np.frombuffer(want[k][0], np.uint8) for k in names], np.array([want[k][1] for k in names], np.int64))


def _check(rv, planted, what, pick=None):
    names, regions, rds, rev, st, en, want_l, want_s = planted
    pick = range(len(names)) if pick is None else pick
    got_l, got_s = rv.align_labels_device([regions[k] for k in pick], [rds[k] for k in pick], rev[pick], st[pick], en[pick])
    assert got_s.dtype == np.int64 and got_s.shape == (len(pick), 7) and len(got_l) == len(pick), what
    bad = [(names[k], got_s[q].tolist(), want_s[k].tolist()) for q, k in enumerate(pick)
           if got_s[q].tolist() != want_s[k].tolist() or got_l[q].dtype != np.uint8 or got_l[q].tobytes() != want_l[k].tobytes()]
    assert not bad, (what, len(bad), bad[:6])


# ---- 1. the kernels on planted pairs ------------------------------------------------------------------------------------------------
def test_align_labels_on_planted_pairs(species_models, planted, monkeypatch):
    monkeypatch.delenv("NRV_LABELS_BUDGET", raising=False)
    names, regions, rds, rev, st, en, want_l, want_s = planted
    S = 64 * strip()
    # the planted set is what it says: both strands, no truth first / in the middle / last, leading and trailing D, several stripes
    assert len(names) > 1400 and 0 < rev.sum() < len(names) and (want_s[0] == -1).all() and (want_s[-1] == -1).all()
    assert ((want_s == -1).all(1)).sum() >= 6 and (want_s[:, 6] > 0).sum() >= 10 and sum(e - s > 2 * S for s, e in zip(st, en)) >= 4
    assert sum(bool(len(l)) and bool(l[-1] & 16) for l in want_l) >= 6
    rv = _engine(monkeypatch, *species_models["ecoli"])
    for p in range(2):                                                   # a second pass over the same handle: the same pairs
        _check(rv, planted, ("one call", p))
    for name in ("m=65 cut 1:64 +", f"m={S + 1} cut {S - 20}:{S + 1} +", f"m={2 * S + 1} cut {S - 20}:{S + 20} -", "m=64 empty read +",
                 "empty region last -", "a leading D run of a stripe and more -", "repeat AAAA / AAA +", "start == end == 17 +"):
        _check(rv, planted, name, [names.index(name)])                   # one pair at a time: a grid of one wave and one thread
    k = names.index("repeat AAAA / AAA +")
    assert want_l[k].tolist() == [5, 5, 5] and want_s[k].tolist() == [3, 0, 0, 1, 0, 0, 1]       # the gap lands left-aligned
    k = names.index("repeat AAA / AAAA +")
    assert want_l[k].tolist() == [1, 5, 5, 5] and want_s[k].tolist() == [3, 0, 1, 0, 1, 0, 0]
    got_l, got_s = rv.align_labels_device([], [], [], [], [])
    assert got_l == [] and got_s.shape == (0, 7)
    rv.close()


# ---- 2. batches -----------------------------------------------------------------------------------------------------------------------
def test_batches_give_the_same_bytes(species_models, planted, monkeypatch):
    names, regions, rds, rev, st, en, want_l, want_s = planted
    need = [-(-(e - s) // (64 * strip())) * (len(r) + 63) * 256 for r, s, e in zip(rds, st, en)]
    assert sum(need) > 20 * BUDGET and max(need) > 3 * BUDGET            # several batches, and pairs that run alone
    monkeypatch.setenv("NRV_LABELS_BUDGET", str(BUDGET))
    rv = _engine(monkeypatch, *species_models["ecoli"])
    monkeypatch.delenv("NRV_LABELS_BUDGET")
    for p in range(2):
        _check(rv, planted, ("batches", p))
    rv.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_refused_by_name(species_models, planted, monkeypatch):
    from nanoreviser_amd import engine as E
    monkeypatch.delenv("NRV_LABELS_BUDGET", raising=False)
    rv = _engine(monkeypatch, *species_models["ecoli"])
    a = np.frombuffer(b"ACGTACGT", np.uint8)
    ok = dict(a=a, a_off=[0, 4, 8], b=a, b_off=[0, 3, 8], reverse=[0, 1], start=[0, 1], end=[4, 4])
    for k, v in (("a_off", [1, 4, 8]), ("a_off", [0, 5, 4]), ("b_off", [0, 9, 8]), ("b_off", [2, 4, 8]),
                 ("start", [-1, 1]), ("start", [0, 5]), ("end", [5, 4]), ("end", [4, 0])):
        with pytest.raises(E.NrvError, match="nrv_align_labels"):       # refused under the entry point's name
            rv.align_labels_arrays(**dict(ok, **{k: v}))
    with pytest.raises(E.NrvError, match="nrv_align_labels: reverse"):
        rv.align_labels_arrays(**dict(ok, reverse=[0, 2]))
    with pytest.raises(E.NrvError, match="nrv_align_labels: bounds"):
        rv.align_labels_arrays(**dict(ok, end=[4, 5]))
    big = np.full(E.LABELS_MAX_LEN + 1, ord("A"), np.uint8)
    with pytest.raises(E.NrvError, match="nrv_align_labels.*NRV_LABELS_MAX_LEN"):
        rv.align_labels_arrays(a, [0, 8], big, [0, big.size], [0], [0], [8])
    with pytest.raises(E.NrvError, match="nrv_align_labels.*NRV_LABELS_MAX_LEN"):
        rv.align_labels_arrays(big, [0, big.size], a, [0, 8], [0], [0], [big.size])
    good = (rv._h, a, np.array([0, 8], np.int64), a, np.array([0, 8], np.int64), 1, np.zeros(1, np.uint8), np.zeros(1, np.int64),
            np.full(1, 8, np.int64), np.zeros(8, np.uint8), np.zeros(7, np.int64))
    for k in (1, 2, 3, 4, 6, 7, 8, 9, 10):                               # a null argument, one at a time
        with pytest.raises(E.NrvError, match="nrv_align_labels"):
            rv._check(rv._lib.nrv_align_labels(*E._marshal(good[:k] + (None,) + good[k + 1:], E._ALIGN_LABELS_T)))
    # a region above the limit with bounds inside it is fine, and the handle is usable after the refusals
    lab, summ = rv.align_labels_arrays(big, [0, big.size], a, [0, 8], [0], [3], [7])
    assert lab.tolist() == [5, 1, 1, 1, 5, 1, 13, 13] and summ.tolist() == [[2, 2, 4, 0, 0, 0, 0]]
    lab, summ = rv.align_labels_arrays(**ok)
    assert lab.tolist() == [5, 2, 20, 1, 1, 2, 4, 3] and summ.tolist() == [[3, 0, 0, 1, 0, 0, 0], [3, 0, 2, 0, 2, 0, 0]]
    _check(rv, planted, "after the refusals", list(range(0, len(planted[0]), 37)))
    rv.close()


# ---- 4. NRV_POISON --------------------------------------------------------------------------------------------------------------------
def test_poisoned_workspace_gives_the_same_bytes(species_models, planted, monkeypatch):
    names, regions, rds, rev, st, en, want_l, want_s = planted
    S = 64 * strip()
    carry = [k for k in range(len(names)) if en[k] - st[k] > S and len(rds[k])]      # more than one stripe: they read the carry words
    assert len(carry) >= 30
    some = sorted(set(carry) | set(range(0, len(names), 9)))
    for poison in PATTERNS:
        for budget in (None, BUDGET):
            if budget is None:
                monkeypatch.delenv("NRV_LABELS_BUDGET", raising=False)
            else:
                monkeypatch.setenv("NRV_LABELS_BUDGET", str(budget))
            rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)
            for p in range(2):
                _check(rv, planted, (poison, budget, p), some)
            rv.close()
    monkeypatch.delenv("NRV_LABELS_BUDGET", raising=False)


# ---- 5. a call in flight --------------------------------------------------------------------------------------------------------------
def test_labels_while_a_raw_call_is_in_flight(species_models, short_reads, planted, monkeypatch):
    monkeypatch.delenv("NRV_LABELS_BUDGET", raising=False)
    rv = _engine(monkeypatch, *species_models["ecoli"])
    rrs = [r for r, _ in short_reads]
    args = ([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs], [r.shift for r in rrs], [r.scale for r in rrs])
    alone = rv.run_packed_raw(rv.pack_reads_raw(*args, rv.T))
    pick = list(range(0, len(planted[0]), 5))
    _check(rv, planted, "alone", pick)
    t = rv.begin_packed_raw(rv.pack_reads_raw(*args, rv.T))
    _check(rv, planted, "between _begin and _end", pick)
    got = rv.end_packed_raw(t)
    assert len(got) == len(alone) == 4
    for k, (g, w) in enumerate(zip(got, alone)):
        _same(g, w, ("the raw call", k))
    rv.close()


# ---- 6. command line ------------------------------------------------------------------------------------------------------------------
def test_command_line_labels_are_the_same_on_the_device_route(tmp_path, monkeypatch):
    from nanoreviser_amd.engine import Reviser
    for k in ("NRV_DEVICE_STATS", "NRV_DEVICE_MERGE", "NRV_CLI_PIPELINE", "NRV_CLI_ENGINES", "NRV_REPORT", "NRV_EDITS", "NRV_COMBINED", "NRV_SUMMARY",
              "NRV_TRIM_Q", "NRV_TRUTH", "NRV_ACCURACY", "NRV_ERROR_CLASSES", "NRV_INFIX", "NRV_LABELS", "NRV_LABELS_BUDGET"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NRV_CLI_GROUPS", "2")                               # several device calls, one in flight behind the other
    d = tmp_path / "in"
    d.mkdir()
    src = sorted(glob.glob(os.path.join(FAST5, "*.fast5")) + glob.glob(os.path.join(GOLD, "fast5_more", "*.fast5")))
    n = 4
    for i in range(n):
        shutil.copy(src[i % len(src)], d / f"s{i:02d}.fast5")
    calls, forms = [], []
    real, real_begin = Reviser.align_labels_arrays, Reviser.begin_packed_raw
    monkeypatch.setattr(Reviser, "align_labels_arrays", lambda self, *a: calls.append(len(a[1]) - 1) or real(self, *a))
    monkeypatch.setattr(Reviser, "begin_packed_raw", lambda self, packed: forms.append(len(packed)) or real_begin(self, packed))
    fa = str(tmp_path / "regions.fa")
    outs, labs = {}, {}
    for tag, extra in (("plain", []), ("host", ["truth"]), ("device", ["--device_merge", "truth"]),
                       ("forward_host", ["--infix_strand", "forward", "truth"]), ("forward", ["--device_merge", "--infix_strand", "forward", "truth"])):
        del calls[:], forms[:]
        out = str(tmp_path / tag) + "/"
        ldir = tmp_path / (tag + "_labels")
        argv = ["-d", str(d), "-o", out, "-S", "ecoli", "--gpus", "1", "--thread", "4"]
        argv += [x for e in extra for x in (["--truth", fa, "--infix", str(tmp_path / (tag + ".inf")), "--labels", str(ldir)] if e == "truth" else [e])]
        assert cli.main(argv) == 0
        outs[tag] = {f: open(out + f, "rb").read() for f in sorted(os.listdir(out))}
        assert outs[tag]["failed_reads.txt"] == b""
        if "truth" in extra:
            labs[tag] = {f: open(ldir / f, "rb").read() for f in sorted(os.listdir(ldir))}
            assert sorted(labs[tag]) == ["labels.tsv"] + [f"s{i:02d}_labels.txt" for i in range(n) if i != 2], (tag, sorted(labs[tag]))
            # ONE nrv_align_labels call per device call on the device route, none on the host route
            assert (len(calls) == len(forms) >= 2 and sum(calls) == n and set(forms) == {33}) if "--device_merge" in extra else not calls, (tag, calls, forms)
        if tag == "plain":                          # the regions: a seeded 5 % mutation of what the plain run wrote, between flanks
            rng = np.random.default_rng(8)
            with open(fa, "w") as fp:
                for i in range(n):
                    if i != 2:                                              # one read left out; every second region on the other strand
                        t = random_seq(rng, 64 + i) + mutate(rng, outs[tag][f"s{i:02d}_out.fasta"].split(b"\n")[1], 0.05) + random_seq(rng, 80)
                        t = (revcomp(t) if i % 2 else t).decode()
                        fp.write(f">s{i:02d}{'.fast5' if i % 2 else ''}\n" + "".join(t[k:k + 70] + "\n" for k in range(0, len(t), 70)))
    assert labs["device"] == labs["host"] and labs["forward"] == labs["forward_host"]
    assert outs["host"] == outs["device"] == outs["forward"] == outs["plain"]
    idx = [ln.split("\t") for ln in labs["host"]["labels.tsv"].decode().split("\n")]
    assert idx[0] == cli.LABELS_HEADER.split("\t") and idx[-2] == ["#reads", str(n - 1), "1", "0"] and idx[-3][0] == "#total" and idx[-1] == [""]
    for i, c in enumerate(idx[1:n + 1]):
        assert c[0] == f"s{i:02d}.fast5" and c[1] == ("no_truth" if i == 2 else "with_truth")
        if i == 2:
            continue
        head, bases, mp, l1, l2, last = labs["host"][f"s{i:02d}_labels.txt"].decode().split("\n")
        assert last == "" and head.split("\t") == ["#" + c[0]] + c[2:13] and c[2] == "+-"[i % 2]
        ln, (match, sub, ins, dele, clip_s, clip_e, lead) = int(c[5]), map(int, c[6:13])
        assert len(bases) == len(mp) == len(l1) == len(l2) == ln > 1000 and match + sub + ins == ln
        # the read lies inside the flanks: the infix bounds leave no leading D, and a 5 % mutation of the REVISED read is mostly matches
        assert lead == 0 and not mp.endswith("D") and match > 0.7 * ln and 0 < sub and 0 < ins and 0 < dele
        assert [int(x) for x in c[13:19]] == [l1.count(str(k)) for k in range(6)] and [int(x) for x in c[19:25]] == [l2.count(str(k)) for k in range(6)]
        assert set(mp) == set("MXID") and l1.count("0") >= mp.count("D")
    tot = idx[-3]
    assert [int(x) for x in tot[5:25]] == [sum(int(c[k]) for c in idx[1:n + 1] if c[1] == "with_truth") for k in range(5, 25)]
    fwd = [ln.split("\t") for ln in labs["forward"]["labels.tsv"].decode().split("\n")]
    assert [c[2] for c in fwd[1:n + 1]] == ["+", "+", ".", "+"] and fwd[1] == idx[1] and fwd[2] != idx[2]
