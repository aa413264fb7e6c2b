"""Inputs and the reference loops shared by tests/test_trim_host.py and tests/test_gpu_device_trim.py (no test here).

`loop_trim` is the per-read, per-position transcription of the rule text of include/nanorev.h (nrv_revise_reads_raw_trim_begin) in
plain Python: it shares no code with hoststage (no trim_bounds, no prefix sum).  `loop_trimmed_records` cuts the reads by hand
and lays the records out with `records_cases.loop_records`.  `planted_cases(W)` are the smallest shapes at which a window kernel
that works in tiles of 256 characters with a halo of W - 1 can go wrong: read lengths around W and around the tile, many reads in
one tile, one read over more than 256 tiles, the only good window at either end of a read and across a tile edge, a window that is
good only by reaching into the next read, sums exactly at and one below the bar."""
import numpy as np

from records_cases import loop_records

TILE = 256                                                      # characters per workgroup of trim_window_kernel
WINDOWS = (1, 2, 10, 64)


def loop_trim(qual, off, Q, W):
    """int64[R][2] by the rule text, one read and one position at a time."""
    out = []
    for r in range(len(off) - 1):
        q = [max(int(c) - 33, 0) for c in qual[int(off[r]):int(off[r + 1])]]
        L = len(q)
        good = [i for i in range(L) if i + W <= L and sum(q[i:i + W]) >= Q * W]
        out.append((good[0], good[-1] + W) if good else (0, 0))
    return np.array(out, np.int64).reshape(-1, 2)


def loop_trimmed_records(names, seq, qual, off, trim, min_len):
    """(blob bytes, rec_off list) of the trimmed reads, by slicing by hand: a dropped read has no record."""
    blob, rec_off = b"", [0]
    for r, name in enumerate(names):
        lo, hi = int(trim[r][0]), int(trim[r][1])
        if hi - lo >= min_len:
            a = int(off[r]) + lo
            rec, _ = loop_records([name], seq[a:a + hi - lo], None if qual is None else qual[a:a + hi - lo], [0, hi - lo])
            blob += rec
        rec_off.append(len(blob))
    return blob, rec_off


def _join(reads):
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    q = np.concatenate([np.asarray(r, np.int64) for r in reads] + [np.zeros(0, np.int64)])
    return (q + 33).astype(np.uint8), off


def planted_cases(W, Q=20):
    """{name: (qual uint8[], off int64[R + 1], Q)}: quality CHARACTERS.  `bad` is Phred 2.  The cases with ONE good window carry
    Q = 40: only a window of W characters of Phred 40 reaches the bar, one that overlaps the planted one does not."""
    bad, hi = 2, 40
    cases = {}

    def read(L, good_at=(), fill=bad):
        """L characters of `fill` with windows of Phred 40 planted at the given positions."""
        q = np.full(L, fill, np.int64)
        for i in good_at:
            q[i:i + W] = hi
        return q

    # read lengths around W and around the tile, all good and all bad; an empty read first, in the middle and last
    lens = [0, W - 1, W, W + 1, 255, 256, 257, 256 + W - 1, 0, 513, 0]
    cases["lengths, all 40"] = _join([read(L, fill=hi) for L in lens]) + (Q,)
    cases["lengths, all bad"] = _join([read(L) for L in lens]) + (Q,)
    rng = np.random.default_rng(7 + W)
    cases["lengths, random"] = _join([rng.integers(0, 41, L) for L in lens]) + (Q,)
    # many reads per tile
    cases["300 reads of 3"] = _join([rng.integers(0, 41, 3) for _ in range(300)]) + (Q,)
    # more than 256 tiles in one read, a short read on either side
    long = rng.integers(0, 41, 70000)
    long[:W + 5] = bad
    long[-(W + 7):] = bad
    cases["70000 in one read"] = _join([rng.integers(0, 41, 5), long, rng.integers(0, 41, 300)]) + (Q,)
    # the only good window at position 0, at L - W, and with its first character the last of a tile (the halo)
    L = 2 * TILE + 77
    pre = 100                                                   # characters of the read in front: the read starts inside a tile
    cases["only window at 0"] = _join([read(pre), read(L, [0]), read(50)]) + (40,)
    cases["only window at L - W"] = _join([read(pre), read(L, [L - W]), read(50)]) + (40,)
    cases["only window across a tile edge"] = _join([read(pre), read(L, [TILE - 1 - pre]), read(50)]) + (40,)
    cases["only window ends at a tile edge"] = _join([read(pre), read(L, [2 * TILE - pre - W]), read(50)]) + (40,)
    # a window that would be good ONLY by reaching into the next read: the last W - 1 characters of a read are 40 and so are the
    # first of the next, whose own first whole window is spoiled further in - and the same across a tile edge
    if W > 1:
        a = read(pre + 30)
        a[-(W - 1):] = hi
        b = read(L)
        b[:W - 1] = hi
        cases["window reaching into the next read"] = _join([a, b]) + (40,)
        a = read(TILE)
        a[-(W - 1):] = hi
        cases["window reaching into the next read over a tile edge"] = _join([a, b]) + (40,)
    # sums exactly Q * W and Q * W - 1
    exact = np.full(W, Q, np.int64)
    below = exact.copy()
    below[W // 2] -= 1
    lead = read(7, fill=0)
    cases["sum exactly Q W"] = _join([np.concatenate([lead, exact, lead]), np.concatenate([lead, below, lead])]) + (Q,)
    cases["characters below '!'"] = (np.concatenate([np.full(W + 3, 10, np.uint8), np.full(W, 33 + Q, np.uint8)]),
                                    np.array([0, 2 * W + 3], np.int64), Q)
    cases["no reads"] = (np.zeros(0, np.uint8), np.zeros(1, np.int64), Q)
    cases["Q 1 and Q 40"] = _join([rng.integers(0, 3, 400), rng.integers(38, 41, 400)]) + (1,)
    return cases
