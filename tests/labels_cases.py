"""Inputs and the reference (labels, summary) pairs shared by tests/test_labels_host.py and tests/test_gpu_labels.py (no test here).

A read s is aligned against u = strand(t)[start:end] of its truth region t (include/nanorev.h, nrv_align_labels;
hoststage.align_labels is the definition): the global recurrence on (d, -M) with the candidates in the order diagonal, I (the
read character alone), D (the truth character alone), the FIRST that attains the minimum is the cell's direction, and the path
walks back from (L, n).  Two references, neither of which shares code with hoststage:
  `enum_columns`   every alignment enumerated as a string of columns (up to 5 characters a side): among those with the optimal
                   (d, M) the one whose columns, read from the END backwards, are lexicographically smallest under
                   diagonal < I < D - no recurrence at all;
  `loop_columns`   the recurrence of the rule text over Python tuples with a direction per cell and the walk, on the full table
                   (up to SMALL characters a side) or, for the long pairs, on the cells within `band` of the main diagonal -
                   band = accuracy_cases.row_distance(u, s), a path with that many edits never leaves it; `reference` asserts
                   the banded form equal to the full one, and both to the enumeration, wherever two of them run.
Both give the alignment as columns in reading order; `columns_to_labels` turns them into the bytes and the seven figures going
FORWARD (the definition and the device form them on the walk back).

`planted_cases()`: infix_cases.planted_cases() with the bounds its reference found - region lengths on both sides of a lane's
strip and of a stripe, up to three stripes and a character, reads cut across strip and stripe boundaries, read lengths
63 / 64 / 65 / 128 / 129, N and lower case, both strands in turn, empty regions first, in the middle and last - and the
label-specific pairs: homopolymers and dinucleotide repeats (the tie-break decides where the gap lands), D runs and I runs of
1, 2 and 17 across a strip boundary, a stripe boundary and lane 0's feed chunk, bounds that are NOT the infix's (leading and
trailing D), start == end, n = 0 and 1, L = 1, N and lower case on both sides.  The references stay below ten seconds over all."""
import numpy as np

import infix_cases
from accuracy_cases import mutate, random_seq, row_distance
from infix_cases import revcomp, strip

SMALL = 300                                                          # the full `loop_columns` up to here
TINY = 5                                                             # `enum_columns` up to here
BAND_CELLS = 450000                                                 # the banded `loop_columns` up to this many cells
CODE = {ord("A"): 5, ord("G"): 4, ord("T"): 3, ord("C"): 2}
_INF = (1 << 40, 0)


def hit(a, b):
    return a == b and a in b"ACGT"


def columns_to_labels(u, s, cols):
    """(labels bytes, (match, sub, ins, del, clip_start, clip_end, lead_del)) of an alignment given as columns in reading order:
    0 a truth character opposite a read character, 1 the read character alone, 2 the truth character alone."""
    u, s = bytes(u), bytes(s)
    lab = bytearray(len(s))
    i = j = match = sub = ins = dele = lead = 0
    diag_at = []                                                     # read positions of the diagonal columns
    for c in cols:
        if c == 2:
            dele += 1
            if j == 0:
                lead += 1
            else:
                lab[j - 1] |= 16
            i += 1
        elif c == 1:
            lab[j] = 1
            ins, j = ins + 1, j + 1
        else:
            ok = hit(u[i], s[j])
            lab[j] = CODE.get(u[i], 0) | (0 if ok else 8)
            match, sub = match + ok, sub + (not ok)
            diag_at.append(j)
            i, j = i + 1, j + 1
    assert i == len(u) and j == len(s)
    clip = (diag_at[0], len(s) - 1 - diag_at[-1]) if diag_at else (len(s), 0)
    return bytes(lab), (match, sub, ins, dele, clip[0], clip[1], lead)


def enum_columns(u, s):
    u, s = bytes(u), bytes(s)
    best = None

    def go(i, j, cols, d, M):
        nonlocal best
        if i == len(u) and j == len(s):
            key = (d, -M, cols[::-1])
            best = key if best is None or key < best else best
            return
        if i < len(u) and j < len(s):
            ok = hit(u[i], s[j])
            go(i + 1, j + 1, cols + (0,), d + (not ok), M + ok)
        if j < len(s):
            go(i, j + 1, cols + (1,), d + 1, M)
        if i < len(u):
            go(i + 1, j, cols + (2,), d + 1, M)

    go(0, 0, (), 0, 0)
    return best[2][::-1]


def loop_columns(u, s, band=None):
    u, s = bytes(u), bytes(s)
    L, n = len(u), len(s)
    inside = (lambda i, j: True) if band is None else (lambda i, j: abs(i - j) <= band)
    dirs = [None] * (L + 1)
    prev = {j: (j, 0) for j in range(n + 1) if inside(0, j)}
    for i in range(1, L + 1):
        cur, dr = {}, {}
        if inside(i, 0):
            cur[0] = (i, 0)
        for j in range(max(1, 0 if band is None else i - band), min(n, n if band is None else i + band) + 1):
            d, M = prev.get(j - 1, _INF)
            cand = [(d, M - 1) if hit(u[i - 1], s[j - 1]) else (d + 1, M)]
            for d, M in (cur.get(j - 1, _INF), prev.get(j, _INF)):
                cand.append((d + 1, M))
            cur[j] = min(cand)
            dr[j] = cand.index(cur[j])                               # the first candidate that attains it
        dirs[i], prev = dr, cur
    i, j, cols = L, n, []
    while i > 0 or j > 0:
        mv = 1 if i == 0 else 2 if j == 0 else dirs[i][j]
        cols.append(mv)
        i, j = i - (mv != 1), j - (mv != 2)
    return tuple(cols[::-1])


def strand(t, reverse):
    return revcomp(t) if reverse else bytes(t)


def reference_pair(t, s, reverse, start, end):
    """(labels, summary) by the references, or None where the pair is too long for them."""
    if len(t) == 0:
        return bytes(len(s)), (-1,) * 7
    u = strand(t, reverse)[start:end]
    L, n = len(u), len(s)
    cols = []
    if L <= TINY and n <= TINY:
        cols.append(enum_columns(u, s))
    if L <= SMALL and n <= SMALL:
        cols.append(loop_columns(u, s))
    band = row_distance(u, s) if L and n else max(L, n)
    if L * min(n + 1, 2 * band + 1) <= BAND_CELLS and (not cols or L * n <= 2500):
        cols.append(loop_columns(u, s, band))
    if not cols:
        return None
    assert all(c == cols[0] for c in cols), (u, s, cols)
    return columns_to_labels(u, s, cols[0])


def planted_cases(seed=3410):
    """name -> (region, read, reverse, start, end)."""
    R = strip()
    S = 64 * R
    rng = np.random.default_rng(seed)
    inf, _ = infix_cases.planted_cases()
    ref = infix_cases.reference()
    cases = {}
    for name, (t, s, rev) in inf.items():
        _, _, st, en = ref[name] if t else (0, 0, 0, 0)
        cases[name] = (t, s, rev, st, en)

    def both(name, t, s, st=0, en=None):
        en = len(t) if en is None else en
        m = len(t)
        assert name + " +" not in cases and name + " -" not in cases, name
        cases[name + " +"] = (t, s, 0, st, en)
        cases[name + " -"] = (revcomp(t), s, 1, st, en)               # the same u on the other strand
        assert strand(revcomp(t), 1)[st:en] == t[st:en] and m == len(t)

    # the tie-break decides where the gap lands: homopolymers and dinucleotide repeats
    for t, s in ((b"AAAA", b"AAA"), (b"AAA", b"AAAA"), (b"ACACAC", b"ACAC"), (b"ACAC", b"ACACAC"), (b"GAAAAT", b"GAAT"), (b"GAAT", b"GAAAAT"),
                 (b"CACACACAG", b"CACAG"), (b"TTTTTTTTTTTTTTTTTTTT", b"TTTTTTTTTTTTTTTTT"), (b"A" * 40, b"A" * 17), (b"AC" * 20, b"AC" * 30)):
        both(f"repeat {t.decode()} / {s.decode()}", t, s)
    # D runs and I runs of 1, 2 and 17 across a strip boundary (row R), a stripe boundary (row S) and lane 0's feed chunk (column 64)
    for at, m in ((R, 3 * R + 5), (64, 140), (S, S + 90)):
        t = random_seq(rng, m)
        for run in (1, 2, 17):
            for lo in sorted({at - run + 1, at - run // 2, at}):     # the run ends at, lies across and starts at the boundary
                if run == 1 and lo != at:
                    continue
                both(f"m={m} D run of {run} at {lo}", t, t[:lo] + t[lo + run:])
                both(f"m={m} I run of {run} at {lo}", t, t[:lo] + random_seq(rng, run) + t[lo:])
    t = random_seq(rng, S + R + 3)
    both("mutated 10 % across the stripe", t, mutate(rng, t, 0.1))
    both("mutated 10 %, bounds inside", t, mutate(rng, t[40:S + 5], 0.1), 40, S + 5)
    t = random_seq(rng, 2 * S + 40)                                  # three stripes of u: the carry words are written and read twice
    both("three stripes, mutated 5 %", t, mutate(rng, t, 0.05))
    both("three stripes, a short read at the end", t, t[2 * S - 30:2 * S + 20], 5, 2 * S + 40)
    # bounds that are NOT the infix's: the region's characters in front of and behind the read are deleted, or the read's hang over
    t = random_seq(rng, 120)
    both("bounds wider than the read", t, t[30:90], 22, 97)
    both("bounds wider, mutated", t, mutate(rng, t[30:90], 0.1), 25, 95)
    both("bounds narrower than the read", t, t[30:90], 35, 80)
    both("bounds beside the read", t, t[30:60], 70, 100)
    t = random_seq(rng, S + 40)
    both("a leading D run of a stripe and more", t, t[S + 5:], 0, S + 40)
    both("a trailing D run across the stripe", t, t[:S - 9], 0, S + 40)
    # start == end, n = 0 and 1, L = 1
    t = random_seq(rng, 50)
    for st in (0, 17, 50):
        both(f"start == end == {st}", t, b"ACGTT", st, st)
        both(f"start == end == {st}, no read", t, b"", st, st)
    both("n = 0", t, b"", 3, 40)
    both("n = 1, a match", t, t[20:21], 10, 30)
    both("n = 1, no match", t, b"N", 10, 30)
    both("L = 1, a match", t, b"GG" + t[9:10] + b"CC", 9, 10)
    both("L = 1, no match", t, b"NNN", 9, 10)
    both("L = 1, n = 1", t, t[9:10], 9, 10)
    both("L = 1, n = 0", t, b"", 9, 10)
    # N and lower case on both sides: they match nothing, their code is 0
    t = bytearray(random_seq(rng, 90))
    for p in (0, R - 1, R, 40, 89):
        t[p] = ord("N")
    for p in (20, 21, 60):
        t[p] = ord("acgt"[p % 4])
    t = bytes(t)
    both("labels: N and lower case, the region itself", t, t)
    both("labels: N and lower case, upper-cased", t, t.upper())
    s = bytearray(random_seq(rng, 90))
    s[5], s[50], s[51] = ord("N"), ord("a"), ord("n")
    both("N and lower case in the read", random_seq(rng, 90), bytes(s))
    both("N opposite another base", b"ACGTNACGT", b"ACGTGACGT")
    both("N opposite N", b"ACGTNACGT", b"ACGTNACGT")
    for name in [k for k in cases if k.startswith("empty region last")]:         # ... and they stay last
        cases[name] = cases.pop(name)
    return cases


_REFERENCE = {}


def reference(seed=3410):
    """name -> (labels, summary) by the references, None where the pair is too long for them; computed once per process."""
    if seed not in _REFERENCE:
        _REFERENCE[seed] = {name: reference_pair(*c) for name, c in planted_cases(seed).items()}
    return _REFERENCE[seed]


_DEFINITION = {}


def definition(seed=3410):
    """name -> (labels bytes, summary tuple, columns) by hoststage.align_labels / align_columns, computed once per process: what
    the device is held to."""
    if seed not in _DEFINITION:
        from nanoreviser_amd import hoststage as hs
        out = {}
        for name, (t, s, rev, st, en) in planted_cases(seed).items():
            lab, summ = hs.align_labels(t, s, rev, st, en)
            out[name] = (lab.tobytes(), tuple(int(x) for x in summ), hs.align_columns(t, s, rev, st, en))
        _DEFINITION[seed] = out
    return _DEFINITION[seed]
