"""Inputs and the two reference distances shared by tests/test_accuracy_host.py and tests/test_gpu_device_accuracy.py (no test here).

`loop_distance` is the table of the rule text of include/nanorev.h in plain Python, for pairs of up to ~300 characters;
`row_distance` fills the same table one row at a time in NumPy - the minimum along a row, D[i][j] = min(c[j], D[i][j-1] + 1), is
`np.minimum.accumulate(c - arange) + arange` - for the long pairs.  Neither shares code with hoststage (no Myers recurrence).

`planted_cases()` holds the smallest shapes at which a wave of 64 lanes with one 64-bit (or 32-bit) word of the truth each can
go wrong: truth lengths on both sides of every block boundary (32, 64, 128) and stripe boundary (2048, 4096) of both block
forms, 4160 = one stripe and one whole block, 8193 = two stripes and one character; per truth length the reads named in
`reads_for`.  The pairs with m >= 4095 are thinned - three reads per length, one of them empty, and a few chunk and run pairs: about a dozen
that cost a full table - so that `row_distance` stays below ten seconds over all.
Every case is (truth bytes, read bytes); `known` carries the distances that are known without any reference."""
import numpy as np

LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4095, 4096, 4097, 4160, 8193)
SMALL = 300                                                          # `loop_distance` up to here


def loop_distance(t, s):
    t, s = bytes(t), bytes(s)
    prev = list(range(len(s) + 1))
    for i in range(1, len(t) + 1):
        cur = [i] + [0] * len(s)
        for j in range(1, len(s) + 1):
            c = 0 if (t[i - 1] == s[j - 1] and t[i - 1] in b"ACGT") else 1
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + c)
        prev = cur
    return prev[len(s)]


def row_distance(t, s):
    t, s = np.frombuffer(bytes(t), np.uint8), np.frombuffer(bytes(s), np.uint8)
    n = s.size
    ar = np.arange(n + 1, dtype=np.int64)
    base = np.isin(s, np.frombuffer(b"ACGT", np.uint8))
    prev = ar.copy()
    cur = np.empty(n + 1, np.int64)
    for i in range(1, t.size + 1):
        cur[0] = i
        np.minimum(prev[1:] + 1, prev[:-1] + np.where(base & (s == t[i - 1]), 0, 1), out=cur[1:])
        prev = np.minimum.accumulate(cur - ar) + ar
    return int(prev[n])


def random_seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def mutate(rng, seq, rate):
    """A seeded mutation of `seq`: each character is, with probability `rate`, substituted, deleted or followed by an insertion."""
    out = bytearray()
    kind = rng.random(len(seq))
    pick = rng.integers(0, 4, len(seq))
    for c, k, p in zip(bytes(seq), kind, pick):
        if k >= rate:
            out.append(c)
        elif k < rate / 3:
            out.append(b"ACGT"[(b"ACGT".find(bytes([c])) + 1 + p % 3) % 4] if c in b"ACGT" else b"ACGT"[p])
        elif k < 2 * rate / 3:
            pass
        else:
            out.append(c)
            out.append(b"ACGT"[p])
    return bytes(out)


def reads_for(rng, t, full):
    """name -> read for one truth; full: every shape (the thinned set of a long truth keeps the ones marked *)."""
    m = len(t)
    r = {"itself*": t, "empty*": b"", "mutated 10 %*": mutate(rng, t, 0.1)}
    if full:
        r.update({"one character": b"G", "3 characters": b"ACG", "mutated 50 %": mutate(rng, t, 0.5), "unrelated": random_seq(rng, m + 7)})
    return r


def planted_cases(seed=3010):
    """(cases: name -> (truth, read), known: name -> distance)."""
    rng = np.random.default_rng(seed)
    cases, known = {}, {}
    for m in LENGTHS:
        t = random_seq(rng, m)
        for name, s in reads_for(rng, t, m < 4095).items():
            cases[f"m={m} {name}"] = (t, s)
        if m:
            known[f"m={m} itself*"], known[f"m={m} empty*"] = 0, m
        if m and m < 4095:
            cases[f"m={m} A against C"] = (b"A" * m, b"C" * (m + 5))
            known[f"m={m} A against C"] = m + 5
            cases[f"m={m} C against longer A"] = (b"A" * m, b"C" * max(m - 5, 1))
            known[f"m={m} C against longer A"] = m
    # pipeline fill and drain beyond one stripe, and an unrelated read across two stripes
    t = random_seq(rng, 4097)
    cases["m=4097 3 characters"], cases["m=4097 unrelated 500"] = (t, b"ACG"), (t, random_seq(rng, 500))
    # chunks removed from / inserted into the truth at a block boundary and mid-block (a random chunk: its removal costs exactly
    # its length only when no cheaper alignment exists, so the known answer is an upper bound there and the reference decides)
    for m, at in ((129, 64), (300, 128), (300, 100), (2049, 1024), (2049, 1000)):
        t = random_seq(rng, m)
        for k in (64, 100):
            if at + k <= m:
                cases[f"m={m} {k} removed at {at}"] = (t, t[:at] + t[at + k:])
            cases[f"m={m} {k} inserted at {at}"] = (t, t[:at] + random_seq(rng, k) + t[at:])
    # 'G' chunks in an 'A' / 'C' / 'T' truth: here the chunk length IS the answer
    t = np.frombuffer(b"ACT", np.uint8)[rng.integers(0, 3, 4160)].tobytes()
    for k, at, inserted in ((64, 64, True), (100, 130, False), (64, 4096, False), (100, 2000, True)):
        name = f"m=4160 G x {k} {'inserted' if inserted else 'removed'} at {at}"
        longer = t[:at] + b"G" * k + t[at:]
        cases[name], known[name] = ((t, longer) if inserted else (longer, t)), k
    # a match run across every block boundary: the carry of the addition runs through every word (a homopolymer, one
    # substitution in front so that the run starts inside block 0)
    for m in (129, 300, 4097):
        cases[f"m={m} match run"] = (b"C" + b"A" * (m - 1), b"G" + b"A" * (m - 1))
        known[f"m={m} match run"] = 1
    # Ns at equal positions in both: each costs 1
    t = bytearray(random_seq(rng, 260))
    for p in (0, 63, 64, 65, 128, 259):
        t[p] = ord("N")
    cases["N at equal positions"], known["N at equal positions"] = (bytes(t), bytes(t)), 6
    cases["lower case matches nothing"], known["lower case matches nothing"] = (b"acgtACGT", b"acgtACGT"), 4
    # 300 pairs of 3 characters
    for k in range(300):
        cases[f"3 characters #{k}"] = (random_seq(rng, 3), random_seq(rng, 3))
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


def reference(seed=3010):
    """name -> the reference distance of every planted pair, computed once per process: `loop_distance` up to SMALL characters
    (and `row_distance` equal to it there), `row_distance` beyond."""
    if seed not in _REFERENCE:
        cases, _ = planted_cases(seed)
        ref = {}
        for name, (t, s) in cases.items():
            d = row_distance(t, s)
            if len(t) <= SMALL and len(s) <= SMALL:
                assert loop_distance(t, s) == d, name
            ref[name] = d
        _REFERENCE[seed] = ref
    return _REFERENCE[seed]


def truth_for_reads(rng, seq, off, rate, without=()):
    """(truth uint8[], truth_off int64[R + 1]): seeded mutations of the reads seq[off[r]:off[r + 1]], none for the reads in
    `without` (and none for an empty read's mutation that came out empty)."""
    seq = np.asarray(seq, np.uint8)
    parts = [b"" if r in without else mutate(rng, seq[int(off[r]):int(off[r + 1])].tobytes(), rate) for r in range(len(off) - 1)]
    toff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), toff
