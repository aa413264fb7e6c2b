"""Inputs and the reference (d, M) pairs shared by tests/test_errclass_host.py and tests/test_gpu_errclass.py (no test here).

d is the unit-cost edit distance of a truth and a read, M the largest number of matched columns among the alignments with d edits
(include/nanorev.h, nrv_revise_reads_raw_errclass_begin).  Three references, none of which shares code with hoststage:
  `loop_classes`      the recurrence of the rule text over Python tuples (d, -M), for pairs of up to ~300 characters;
  `all_alignments`    every global alignment of a pair enumerated, for up to 5 characters: no recurrence at all;
  `diagonal_classes`  the SCALAR form of the rule, cost K edits - matches with K = min(m, n) + 1, filled one anti-diagonal at a
                      time in NumPy (the host definition works row-wise on (d << 32) - M inside a band), for the long pairs;
                      `reference` asserts it equal to the loop wherever both run.

`planted_cases()` holds the smallest shapes at which a wave of 64 lanes with R truth characters each can go wrong (R is read from
engine.ERRCLASS_R, the mirror of the kernel's constant): truth lengths on both sides of a lane's strip (R - 1, R, R + 1) and of
a stripe (64 R - 1, 64 R, 64 R + 1), one stripe and one strip (64 R + R), two stripes and one character, and 0, 1, 2, 63, 64, 65;
per truth the reads of `reads_for`; read lengths on both sides of lane 0's feed chunks; a read of 3 characters against more than
one stripe (pipeline fill and drain); AC / CA, the smallest pair where the tie matters; a few hundred pairs of 3 to 5 characters
over A C G N; N and lower case; homopolymer runs across strip and stripe boundaries; empty truths first, in the middle and
last.  The pairs with a truth of 64 R - 1 and more are thinned so that the references stay below ten seconds over all."""
import itertools

import numpy as np

from accuracy_cases import mutate, random_seq

SMALL = 300                                                          # `loop_classes` up to here
TINY = 5                                                             # `all_alignments` up to here
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def strip():
    from nanoreviser_amd.engine import ERRCLASS_R
    return int(ERRCLASS_R)


def loop_classes(t, s):
    t, s = bytes(t), bytes(s)
    prev = [(j, 0) for j in range(len(s) + 1)]
    for i in range(1, len(t) + 1):
        cur = [(i, 0)]
        for j in range(1, len(s) + 1):
            dg = prev[j - 1]
            dg = (dg[0], dg[1] - 1) if (t[i - 1] == s[j - 1] and t[i - 1] in b"ACGT") else (dg[0] + 1, dg[1])
            cur.append(min((prev[j][0] + 1, prev[j][1]), (cur[j - 1][0] + 1, cur[j - 1][1]), dg))
        prev = cur
    return prev[-1][0], -prev[-1][1]


def all_alignments(t, s):
    """(d, M) by enumeration: an alignment is a choice of k columns that pair a truth character with a read character (in order),
    every other character stands alone."""
    t, s = bytes(t), bytes(s)
    m, n = len(t), len(s)
    best = None
    for k in range(min(m, n) + 1):
        for ti in itertools.combinations(range(m), k):
            for si in itertools.combinations(range(n), k):
                match = sum(t[a] == s[b] and t[a] in b"ACGT" for a, b in zip(ti, si))
                key = ((m - k) + (n - k) + (k - match), -match)
                best = key if best is None or key < best else best
    return best[0], -best[1]


def diagonal_classes(t, s):
    t, s = np.frombuffer(bytes(t), np.uint8), np.frombuffer(bytes(s), np.uint8)
    m, n = t.size, s.size
    K, INF = min(m, n) + 1, 1 << 60
    tb = np.isin(t, _ACGT)
    p2, p1 = np.full(m + 1, INF, np.int64), np.full(m + 1, INF, np.int64)
    p1[0] = 0                                                        # the anti-diagonal i + j = 0
    for k in range(1, m + n + 1):
        cur = np.full(m + 1, INF, np.int64)
        i = np.arange(max(k - n, 1), min(m, k - 1) + 1)              # the cells with i >= 1 and j = k - i >= 1
        if i.size:
            hit = tb[i - 1] & (t[i - 1] == s[k - i - 1])
            cur[i] = np.minimum(np.minimum(p1[i - 1], p1[i]) + K, p2[i - 1] + np.where(hit, -1, K))
        if k <= n:
            cur[0] = K * k
        if k <= m:
            cur[k] = K * k
        p2, p1 = p1, cur
    cost = int(p1[m])
    d = -(-cost // K)
    return d, K * d - cost


def reads_for(rng, t, full):
    """name -> read for one truth; full: every shape (the thinned set of a long truth keeps the ones marked *)."""
    r = {"itself*": t, "empty*": b"", "one character*": b"G", "mutated 10 %*": mutate(rng, t, 0.1)}
    if full:
        r.update({"mutated 50 %": mutate(rng, t, 0.5), "unrelated": random_seq(rng, len(t) + 7)})
    return r


def lengths():
    R = strip()
    return (0, 1, 2, R - 1, R, R + 1, 63, 64, 65, 64 * R - 1, 64 * R, 64 * R + 1, 64 * R + R, 2 * 64 * R + 1)


def planted_cases(seed=3110):
    """(cases: name -> (truth, read), known: name -> (d, M))."""
    R = strip()
    S = 64 * R
    rng = np.random.default_rng(seed)
    cases, known = {}, {}
    for m in lengths():
        t = random_seq(rng, m)
        for name, s in reads_for(rng, t, m < S - 1 or m in (S + 1, 2 * S + 1)).items():
            cases[f"m={m} {name}"] = (t, s)
        if m:
            known[f"m={m} itself*"], known[f"m={m} empty*"] = (0, m), (m, 0)
    # lane 0's feed chunks: read lengths on both sides of 64 and 128, against a short truth and against one of several strips
    for m in (R + 1, 3 * R + 5):
        t = random_seq(rng, m)
        for n in (63, 64, 65, 128, 129):
            cases[f"m={m} read of {n}"] = (t, random_seq(rng, n))
    t = random_seq(rng, 140)
    for n in (63, 64, 65, 128, 129):
        cases[f"m=140 its first {n}"] = (t, t[:n])
        known[f"m=140 its first {n}"] = (140 - n, n)
    # pipeline fill and drain beyond one stripe
    for m in (S + 1, 2 * S + 1):
        t = random_seq(rng, m)
        cases[f"m={m} 3 characters"] = (t, b"ACG")
    # the tie: one deletion and one insertion keep a match, two substitutions keep none
    cases["AC / CA"], known["AC / CA"] = (b"AC", b"CA"), (2, 1)
    cases["ACGT / CGTA"], known["ACGT / CGTA"] = (b"ACGT", b"CGTA"), (2, 3)
    alphabet = np.frombuffer(b"ACGN", np.uint8)
    for k in range(400):
        m, n = int(rng.integers(3, 6)), int(rng.integers(3, 6))
        cases[f"short #{k}"] = (alphabet[rng.integers(0, 4, m)].tobytes(), alphabet[rng.integers(0, 4, n)].tobytes())
    # N at equal positions and lower case match nothing
    t = bytearray(random_seq(rng, 260))
    for p in (0, R - 1, R, 63, 64, 259):
        t[p] = ord("N")
    cases["N at equal positions"], known["N at equal positions"] = (bytes(t), bytes(t)), (6, 254)
    cases["lower case matches nothing"], known["lower case matches nothing"] = (b"acgtACGT", b"acgtACGT"), (4, 4)
    # homopolymer runs across strip boundaries and across the stripe boundary: a shorter run is so many deletions, a longer one so
    # many insertions, and every other column matches
    for m, at, run in ((3 * R, R - 3, 10), (5 * R, 2 * R - 1, R + 2), (S + 40, S - 9, 20)):
        body = np.frombuffer(b"CGT", np.uint8)[rng.integers(0, 3, m)].tobytes()
        t = body[:at] + b"A" * run + body[at:]
        for k in (-3, 4):
            name = f"m={len(t)} run of {run} at {at} {'shorter' if k < 0 else 'longer'} by {abs(k)}"
            cases[name], known[name] = (t, body[:at] + b"A" * (run + k) + body[at:]), (abs(k), len(t) + min(k, 0))
    # pairs with an empty truth first, in the middle and last
    order = list(cases)
    out = {"empty truth first": (b"", b"ACGT")}
    for i, name in enumerate(order):
        out[name] = cases[name]
        if i == len(order) // 2:
            out["empty truth in the middle"] = (b"", b"")
    out["empty truth last"] = (b"", b"ACGTACGT")
    return out, known


_REFERENCE = {}


def reference(seed=3110):
    """name -> the reference (d, M) of every planted pair, computed once per process: `diagonal_classes`, equal to `loop_classes`
    up to SMALL characters and to `all_alignments` up to TINY."""
    if seed not in _REFERENCE:
        cases, _ = planted_cases(seed)
        ref = {}
        for name, (t, s) in cases.items():
            w = diagonal_classes(t, s)
            if len(t) <= SMALL and len(s) <= SMALL:
                assert loop_classes(t, s) == w, name
            if len(t) <= TINY and len(s) <= TINY:
                assert all_alignments(t, s) == w, name
            ref[name] = w
        _REFERENCE[seed] = ref
    return _REFERENCE[seed]


def counts(m, n, d, M):
    """(S, I, D) of a pair, written out once more for the tests: substitutions, insertions, deletions."""
    return m + n - 2 * M - d, d - (m - M), d - (n - M)
