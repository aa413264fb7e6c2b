"""Inputs and the reference (d, M, start, end) tuples shared by tests/test_infix_host.py and tests/test_gpu_infix.py (no test here).

A read s is placed inside a truth REGION t with free ends on the region (include/nanorev.h, nrv_revise_reads_raw_infix_begin):
among all substrings t[start:end] the fewest edits d of a global alignment with s, then the most matched columns M, then the
largest start, then the smallest end; with `reverse` the region is first replaced by its reverse complement.  Three references,
none of which shares code with hoststage:
  `loop_infix`       the recurrence of the rule text over Python tuples (d, -M, -start), for pairs of up to ~300 characters;
  `substring_infix`  every substring enumerated under errclass_cases.all_alignments (up to 5 characters a side) / loop_classes,
                     for pairs of up to 8 characters: no free-end recurrence at all;
  `diagonal_infix`   a SCALAR form, cost d K2 - M K1 - start with K1 = m + 1 and K2 = (min(m, n) + 1) K1, filled one
                     anti-diagonal at a time in NumPy (the host definition works row-wise on d 2^42 - M 2^21 - start), for the
                     long pairs; `reference` asserts it equal to the loop wherever both run.

`planted_cases()` holds the smallest shapes at which a wave of 64 lanes with R region characters each can go wrong (R is read
from engine.INFIX_R, the mirror of the kernel's constant): region lengths on both sides of a lane's strip and of a stripe, one,
two and three stripes and a character; reads CUT OUT of the region with either end on both sides of a strip and of a stripe
boundary, from stripe 0 into stripe 1, ending in stripe 0 of three (the running minimum over later, worse stripes) and ending
exactly at m - the answer is known, (0, b - a, a, b), wherever the cut occurs once; the same reads reverse-complemented on the
reverse strand, (0, b - a, m - b, m - a); the same reads mutated 10 %; a read of Ns; a read that occurs twice (the later copy
wins); AC / CA; 400 pairs of 3 to 6 characters over A C G N on both strands; N and lower case in the region; read lengths on both
sides of lane 0's feed chunks; 3 characters against more than one stripe; reads longer than their region; empty regions first,
in the middle and last on either strand.  Most reads against a long region are short, a few are long: the references stay
below ten seconds over all."""
import numpy as np

from accuracy_cases import mutate, random_seq
from errclass_cases import all_alignments, loop_classes

SMALL = 300                                                          # `loop_infix` up to here
TINY = 8                                                             # `substring_infix` up to here
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def strip():
    from nanoreviser_amd.engine import INFIX_R
    return int(INFIX_R)


def revcomp(t):
    """The reverse complement: A<->T, C<->G, every other byte as it is."""
    return bytes(t).translate(_COMP)[::-1]


def loop_infix(t, s, reverse=False):
    t, s = (revcomp(t) if reverse else bytes(t)), bytes(s)
    n = len(s)
    prev = [(j, 0, 0) for j in range(n + 1)]
    best = prev[n] + (0,)
    for i in range(1, len(t) + 1):
        cur = [(0, 0, -i)]
        for j in range(1, n + 1):
            d, M, st = prev[j - 1]
            dg = (d, M - 1, st) if (t[i - 1] == s[j - 1] and t[i - 1] in b"ACGT") else (d + 1, M, st)
            up, left = prev[j], cur[j - 1]
            cur.append(min((up[0] + 1, up[1], up[2]), (left[0] + 1, left[1], left[2]), dg))
        prev = cur
        best = min(best, cur[n] + (i,))
    return best[0], -best[1], -best[2], best[3]


def substring_infix(t, s, reverse=False):
    """By enumeration of every substring; (d, M) of a substring and the read by every alignment enumerated (up to 5 characters a
    side) or by errclass_cases.loop_classes."""
    t, s = (revcomp(t) if reverse else bytes(t)), bytes(s)
    best = None
    for a in range(len(t) + 1):
        for b in range(a, len(t) + 1):
            d, M = all_alignments(t[a:b], s) if b - a <= 5 and len(s) <= 5 else loop_classes(t[a:b], s)
            key = (d, -M, -a, b)
            best = key if best is None or key < best else best
    return best[0], -best[1], -best[2], best[3]


def diagonal_infix(t, s, reverse=False):
    t = np.frombuffer(revcomp(t) if reverse else bytes(t), np.uint8)
    s = np.frombuffer(bytes(s), np.uint8)
    m, n = t.size, s.size
    K1 = m + 1
    K2, INF = (min(m, n) + 1) * K1, 1 << 60
    tb = np.isin(t, _ACGT)
    sr = s[::-1]
    last = np.full(m + 1, INF, np.int64)                             # W[i][n], met on the anti-diagonal i + n
    # three buffers in turn, never cleared: a cell reads its three neighbours on the two anti-diagonals before, all of them written
    p2, p1, cur = (np.full(m + 1, INF, np.int64) for _ in range(3))
    p1[0] = 0                                                        # the anti-diagonal i + j = 0
    if n == 0:
        last[0] = 0
    for k in range(1, m + n + 1):
        lo, hi = max(k - n, 1), min(m, k - 1)                        # the cells with i >= 1 and j = k - i >= 1: i = lo .. hi
        if lo <= hi:
            hit = tb[lo - 1:hi] & (t[lo - 1:hi] == sr[n - k + lo:n - k + hi + 1])
            cur[lo:hi + 1] = np.minimum(np.minimum(p1[lo - 1:hi], p1[lo:hi + 1]) + K2, p2[lo - 1:hi] + np.where(hit, -K1, K2))
        if k <= n:
            cur[0] = K2 * k                                          # the first row: k edits
        if k <= m:
            cur[k] = -k                                              # column 0: the substring starts at k for nothing
        if 0 <= k - n <= m:
            last[k - n] = cur[k - n]
        p2, p1, cur = p1, cur, p2
    end = int(np.argmin(last))
    cost = int(last[end])
    d = -(-cost // K2)
    rest = K2 * d - cost
    return d, rest // K1, rest % K1, end


def lengths():
    R = strip()
    S = 64 * R
    return (0, 1, 2, R - 1, R, R + 1, 63, 64, 65, S - 1, S, S + 1, S + R, 2 * S + 1, 3 * S + 1)


def _cuts(m):
    """(a, b) of the reads cut out of a region of m characters."""
    R = strip()
    S = 64 * R
    c = [(1, m - 1), (0, m - 1), (1, m), (0, m)]
    if m >= 3 * R:                                                   # either end on both sides of a strip boundary
        c += [(R - 1, R + 25), (R, R + 24), (R + 1, R + 30), (3, 2 * R - 1), (3, 2 * R), (3, 2 * R + 1)]
    if m >= S - 1:                                                   # the best end exactly m, and one strip before it
        c = [(m - 30, m), (m - 30 - R, m - R)] + c[4:]
    for k in (1, 2, 3):                                              # ... and of a stripe boundary; from one stripe into the next
        B = k * S
        if m > B:
            c += [(B - 1, min(B + 30, m)), (B - 20, min(B + 20, m))]
            if k == 1:
                c += [(B, min(B + 30, m)), (B - 30, B - 1), (B - 30, B), (B - 30, B + 1)]
                if m > B + R:
                    c += [(B + 1, B + R)]
    if m > 3 * S:                                                    # the best end in stripe 0 of three
        c += [(100, 140), (S + 200, S + 240)]
    return sorted({(a, b) for a, b in c if 0 <= a < b <= m})


def planted_cases(seed=3310):
    """(cases: name -> (region, read, reverse), known: name -> (d, M, start, end))."""
    R = strip()
    S = 64 * R
    rng = np.random.default_rng(seed)
    cases, known = {}, {}

    def cut(t, a, b, tag=""):
        m, s = len(t), t[a:b]
        once = t.find(s) == t.rfind(s)
        name = f"m={m} cut {a}:{b}{tag}"
        cases[name + " +"] = (t, s, 0)
        cases[name + " -"] = (t, revcomp(s), 1)
        if once:                                                     # the cut occurs once: no other substring has no edit
            known[name + " +"], known[name + " -"] = (0, b - a, a, b), (0, b - a, m - b, m - a)
        if b - a >= 10:                                              # (a long region: the strands take turns, to keep the references quick)
            turn = len(cases) // 2 % 2
            if m < S - 1 or turn == 0:
                cases[name + " mutated 10 % +"] = (t, mutate(rng, s, 0.1), 0)
            if m < S - 1 or turn == 1:
                cases[name + " mutated 10 % -"] = (t, revcomp(mutate(rng, s, 0.1)), 1)

    for m in lengths():
        t = random_seq(rng, m)
        for rev in (0, 1):
            cases[f"m={m} empty read {'+-'[rev]}"] = (t, b"", rev)
            if m:
                known[f"m={m} empty read {'+-'[rev]}"] = (0, 0, m, m)
        for a, b in _cuts(m):
            cut(t, a, b)
    # a few LONG reads against more than one stripe: every column's carry word is written and read
    t = random_seq(rng, S + 1)
    cut(t, R + 1, S + 1, " long")
    t = random_seq(rng, 2 * S + 1)
    cut(t, 5, 2 * S - 3, " long")
    t = random_seq(rng, 3 * S + 1)
    cases["m=3S+1 a mutated middle stripe +"] = (t, mutate(rng, t[S - 7:2 * S + 9], 0.1), 0)
    # lane 0's feed chunks: read lengths on both sides of 64 and 128, against a short region and against one of several strips
    for m in (R + 1, 3 * R + 5):
        t = random_seq(rng, m)
        for n in (63, 64, 65, 128, 129):
            cases[f"m={m} read of {n} +"] = (t, random_seq(rng, n), 0)
            cases[f"m={m} read of {n} -"] = (t, random_seq(rng, n), 1)
    t = random_seq(rng, 140)
    for n in (63, 64, 65, 128, 129):
        cut(t, 0, n, f" its first {n}")
        cut(t, 140 - n, 140, f" its last {n}")
    # pipeline fill and drain beyond one stripe
    for m in (S + 1, 2 * S + 1):
        t = random_seq(rng, m)
        for rev in (0, 1):
            cases[f"m={m} 3 characters {'+-'[rev]}"] = (t, b"ACG", rev)
    # a read longer than its region
    t = random_seq(rng, 40)
    cases["region of 40 inside a read of 60 +"] = (t, random_seq(rng, 9) + t + random_seq(rng, 11), 0)
    cases["region of 40 inside a read of 60 -"] = (t, random_seq(rng, 9) + revcomp(t) + random_seq(rng, 11), 1)
    cases["region of 20, read of 300 +"] = (t[:20], random_seq(rng, 300), 0)
    # a read of Ns matches nothing: n edits, and the largest start there is
    for m in (200, S + 5):
        t = random_seq(rng, m)
        for rev in (0, 1):
            name = f"m={m} a read of Ns {'+-'[rev]}"
            cases[name], known[name] = (t, b"N" * 10, rev), (10, 0, m, m)
    # a read that occurs twice: the later copy wins - inside one strip's reach, and with the later copy across the stripe boundary
    r = random_seq(rng, 20)
    body = np.frombuffer(b"CGT", np.uint8)
    for m, at1, at2 in ((200, 30, 120), (S + 200, 50, S - 10)):
        f = [body[rng.integers(0, 3, k)].tobytes() for k in (at1, at2 - at1 - 20, m - at2 - 20)]
        t = f[0] + b"A" + r[1:] + f[1] + b"A" + r[1:] + f[2]             # (the copies start with the one A of the region's alphabet)
        rr = b"A" + r[1:]
        if t.rfind(rr) == at2 and t.find(rr) == at1:
            known[f"m={m} twice +"], known[f"m={m} twice -"] = (0, 20, at2, at2 + 20), (0, 20, m - at1 - 20, m - at1)
        cases[f"m={m} twice +"], cases[f"m={m} twice -"] = (t, rr, 0), (t, revcomp(rr), 1)
    # the tie: AC holds CA with one edit and one match from position 1 on
    cases["AC / CA"], known["AC / CA"] = (b"AC", b"CA", 0), (1, 1, 1, 2)
    cases["sample of the header +"], known["sample of the header +"] = (b"TTTTACGTACGTTTTT", b"ACGTACG", 0), (0, 7, 4, 11)
    alphabet = np.frombuffer(b"ACGN", np.uint8)
    for k in range(400):
        m, n = int(rng.integers(3, 7)), int(rng.integers(3, 7))
        t, s = alphabet[rng.integers(0, 4, m)].tobytes(), alphabet[rng.integers(0, 4, n)].tobytes()
        cases[f"short #{k} +"], cases[f"short #{k} -"] = (t, s, 0), (t, s, 1)
    # N and lower case in the region match nothing, under the complement too (n stays n, a stays a)
    t = bytearray(random_seq(rng, 260))
    for p in (0, R - 1, R, 63, 64, 259):
        t[p] = ord("N")
    for p in (100, 101, 200):
        t[p] = ord("acgt"[p % 4])
    t = bytes(t)
    cases["N and lower case, the region itself +"] = (t, t, 0)
    cases["N and lower case, its reverse complement -"] = (t, revcomp(t), 1)
    cases["N and lower case, upper-cased +"] = (t, t.upper(), 0)
    cases["N and lower case, upper-cased -"] = (t, revcomp(t.upper()), 1)
    cases["lower case matches nothing +"], known["lower case matches nothing +"] = (b"acgtACGT", b"acgtACGT", 0), (4, 4, 4, 8)
    cases["lower case matches nothing -"] = (b"acgtACGT", b"ACGTacgt", 1)
    # pairs with an empty region first, in the middle and last, on either strand
    order = list(cases)
    out = {"empty region first +": (b"", b"ACGT", 0), "empty region first -": (b"", b"ACGT", 1)}
    for i, name in enumerate(order):
        out[name] = cases[name]
        if i == len(order) // 2:
            out["empty region in the middle +"], out["empty region in the middle -"] = (b"", b"", 0), (b"", b"", 1)
    out["empty region last +"], out["empty region last -"] = (b"", b"ACGTACGT", 0), (b"", b"ACGTACGT", 1)
    return out, known


_REFERENCE = {}


def reference(seed=3310):
    """name -> the reference (d, M, start, end) of every planted pair, computed once per process: `diagonal_infix`, equal to
    `loop_infix` up to SMALL characters and to `substring_infix` up to TINY."""
    if seed not in _REFERENCE:
        cases, _ = planted_cases(seed)
        ref = {}
        for name, (t, s, rev) in cases.items():
            w = diagonal_infix(t, s, rev)
            if len(t) <= SMALL and len(s) <= SMALL:
                assert loop_infix(t, s, rev) == w, name
            if len(t) <= TINY and len(s) <= TINY:
                assert substring_infix(t, s, rev) == w, name
            ref[name] = w
        _REFERENCE[seed] = ref
    return _REFERENCE[seed]


def by_strand(seed=3310):
    """{reverse: (names, regions, reads, the references' tuples as int64[n][4] with -1 in all four for an empty region)}: the
    planted pairs as the unit door takes them, one strand per call."""
    cases, _ = planted_cases(seed)
    ref = reference(seed)
    out = {}
    for rev in (0, 1):
        names = [k for k, c in cases.items() if c[2] == rev]
        want = np.array([ref[k] if cases[k][0] else (-1,) * 4 for k in names], np.int64)
        out[rev] = (names, [cases[k][0] for k in names], [cases[k][1] for k in names], want)
    return out
