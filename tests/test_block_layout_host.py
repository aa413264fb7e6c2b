"""The device blocks of the one-shot entry points, laid out on the host (CPU only): csrc/nrv_block.h.

A region that is too small, or two that overlap, is an out-of-bounds store on the device that no CPU test of the results would
notice.  tests/block_layout_main.cpp - plain C++ with a main of its own - includes the header and prints the offsets and the total
of every layout for the shapes below; it is built with AddressSanitizer + UndefinedBehaviorSanitizer and run directly.  For every
shape of every layout:
  * every offset is a multiple of 256;
  * the regions lie in the order they are named, and each one ends - at the size the kernels index and the entry point copies -
    no later than the next one starts (the last one: than the block ends);
  * the total is the formula the entry point summed by hand before there was a header, written out below as plain arithmetic.
The shapes: one pair with an empty a, an empty b or both; lengths 255 / 256 / 257 (and offset arrays of 256 and 264 bytes); a
pair of two stripes (ta = 4097, tb = 1025); FASTA and FASTQ records, with and without a trim."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "block_layout_main.cpp")
LABEL_COLS = 7                                 # NRV_LABEL_COLS
DESC = 48                                      # sizeof(nrv_read_desc)


def up(x):
    return (x + 255) & ~255


def _compiler():
    if shutil.which("g++"):
        return "g++"
    clang = "/opt/rocm/llvm/bin/clang++"
    return clang if os.path.exists(clang) else None


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """ask(requests) -> one {name: value} per request, in the program's order of printing (dicts keep it)."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler in this image")
    exe = str(tmp_path_factory.mktemp("block_layout") / "block_layout_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def ask(requests):
        text = "".join(" ".join(str(int(x)) if not isinstance(x, str) else x for x in q) + "\n" for q in requests)
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-4000:])
        lines = p.stdout.splitlines()
        assert len(lines) == len(requests)
        return [{k: int(v) for k, v in (f.split("=") for f in ln.split())} for ln in lines]

    return ask


def _check(got, regions, total, what):
    """regions: [(name, bytes the kernels index / the entry point copies)] in the block's order."""
    assert list(got) == [n for n, _ in regions] + ["bytes"], (what, got)
    for name, _ in regions:
        assert got[name] % 256 == 0, (what, name, got)
    assert got["bytes"] % 256 == 0, (what, got)
    assert got[regions[0][0]] == 0, (what, got)
    ends = [got[n] for n, _ in regions[1:]] + [got["bytes"]]
    for (name, size), end in zip(regions, ends):
        assert got[name] + size <= end, (what, name, size, got)       # in order, disjoint, large enough
    assert got["bytes"] == total, (what, got, total)


PAIR_SHAPES = [(1, 0, 0), (1, 0, 5), (1, 5, 0), (1, 1, 1), (1, 255, 255), (1, 256, 256), (1, 257, 257), (1, 255, 257), (1, 4097, 1025),
               (3, 4097 + 7, 1025 + 300), (31, 255, 256), (32, 256, 257), (33, 1000, 999), (64, 64 * 4097, 64 * 4097), (800, 3600, 3601)]


@pytest.mark.parametrize("door,carry,k", [("nrv_edit_distance", 1, 1), ("nrv_edit_classes", 8, 2), ("nrv_infix_classes", 8, 4)])
def test_pair_doors(layout, door, carry, k):
    got = layout([("pair", n, ta, tb, carry, k) for n, ta, tb in PAIR_SHAPES])
    for (n, ta, tb), g in zip(PAIR_SHAPES, got):
        nb = (n + 1) * 8
        # align_kernel: a carry byte per character of b; errclass_kernel and infix_kernel: a 64-bit word
        regions = [("a_off", nb), ("b_off", nb), ("a", ta), ("b", tb), ("hc", tb if door == "nrv_edit_distance" else 8 * tb)]
        regions += [(f"out{q}", 8 * n) for q in range(k)]
        o_bo = up(nb); o_a = o_bo + up(nb); o_b = o_a + up(ta); o_hc = o_b + up(tb)                     # noqa: E702
        if door == "nrv_edit_distance":
            o_d = o_hc + up(tb)
            total = o_d + up(n * 8)
        elif door == "nrv_edit_classes":
            o_d = o_hc + up(tb * 8)
            total = o_d + 2 * up(n * 8)
        else:
            o_d = o_hc + up(tb * 8)
            total = o_d + 4 * up(n * 8)
        _check(g, regions, total, (door, n, ta, tb))
        assert g["hc"] == o_hc and [g[f"out{q}"] for q in range(k)] == [o_d + q * up(n * 8) for q in range(k)]


def test_trim_door(layout):
    shapes = [(1, 0), (1, 1), (1, 255), (1, 256), (1, 257), (15, 4000), (16, 4096), (17, 4097), (31, 1), (32, 100000), (1000, 123457)]
    for (n, total_q), g in zip(shapes, layout([("trim", n, t) for n, t in shapes])):
        nb, tb = (n + 1) * 8, n * 16                                     # two 64-bit words per read: the accumulators, the bounds
        o_q = up(nb); o_acc = o_q + up(total_q); o_trim = o_acc + up(tb)                                # noqa: E702
        _check(g, [("off", nb), ("qual", total_q), ("acc", 16 * n), ("trim", 16 * n)], o_trim + up(tb), ("nrv_trim_reads", n, total_q))


def test_record_door(layout):
    shapes = []
    for n, name_bytes, total in [(1, 0, 0), (1, 1, 0), (1, 0, 1), (2, 255, 255), (2, 256, 256), (3, 257, 257), (31, 500, 4097), (32, 16, 100001),
                                 (33, 4096, 1)]:
        for fastq in (0, 1):
            for trim in (0, 1):
                q = 2 if fastq else 1
                shapes.append((n, name_bytes, total, fastq, name_bytes + q * total + 3 * q * n, trim))      # blob_capacity
    for (n, name_bytes, total, fastq, cap, trim), g in zip(shapes, layout([("record",) + s for s in shapes])):
        nb = (n + 1) * 8
        o_noff = up(nb); o_names = o_noff + up(nb); o_seq = o_names + up(name_bytes); o_qual = o_seq + up(total)   # noqa: E702
        o_roff = o_qual + (up(total) if fastq else 0); o_blob = o_roff + up(nb); o_trim = o_blob + up(cap)         # noqa: E702
        want = o_trim + (up(n * 16) if trim else 0)
        regions = [("off", nb), ("name_off", nb), ("names", name_bytes), ("seq", total), ("qual", total if fastq else 0), ("rec_off", nb),
                   ("blob", cap), ("trim", 16 * n if trim else 0)]
        _check(g, regions, want, ("nrv_pack_records_trim", n, name_bytes, total, fastq, trim))
        assert (g["qual"], g["rec_off"], g["blob"], g["trim"]) == (o_qual, o_roff, o_blob, o_trim)


def test_labels_door(layout):
    shapes = [(1, 0, 0, 0), (1, 0, 5, 0), (1, 5, 0, 0), (1, 1, 1, 64 * 64), (1, 255, 255, 1), (1, 256, 256, 63), (1, 257, 257, 65),
              (1, 4097, 1025, 5 * (1025 + 63) * 64), (31, 2000, 2001, 1 << 20), (32, 3000, 2999, 12345), (33, 70000, 65536, 1 << 24)]
    for (n, ta, tb, words), g in zip(shapes, layout([("labels", n, ta, tb, LABEL_COLS, w) for n, ta, tb, w in shapes])):
        nb, np8 = (n + 1) * 8, up(n * 8)
        o_bo = up(nb); o_st = o_bo + up(nb); o_en = o_st + np8; o_do = o_en + np8; o_rv = o_do + np8; o_a = o_rv + up(n)     # noqa: E702
        o_b = o_a + up(ta); o_hc = o_b + up(tb); o_lab = o_hc + up(tb * 8); o_sum = o_lab + up(tb)                           # noqa: E702
        o_dir = o_sum + up(n * LABEL_COLS * 8)
        regions = [("a_off", nb), ("b_off", nb), ("start", 8 * n), ("end", 8 * n), ("dir_off", 8 * n), ("reverse", n), ("a", ta), ("b", tb),
                   ("hc", 8 * tb), ("labels", tb), ("summary", n * LABEL_COLS * 8), ("dir", 4 * words)]
        _check(g, regions, o_dir + up(words * 4), ("nrv_align_labels", n, ta, tb, words))


def test_merge_calls_inputs(layout):
    shapes = []
    for n_reads, N, T in [(1, 12, 11), (1, 256 + 11, 11), (2, 255, 1), (3, 257, 2), (7, 4097, 32), (40, 100000, 11)]:
        n = N - T
        for have_p, records, truth in [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1)]:
            for name_bytes, truth_bytes in [(0, 0), (255, 257), (4096, N + 300)]:
                shapes.append((n_reads, DESC, N, n, have_p, records, name_bytes, truth, truth_bytes, 256 * (n_reads + 5)))
    for s, g in zip(shapes, layout([("merge_in",) + s for s in shapes])):
        n_reads, _, N, n, have_p, records, name_bytes, truth, truth_bytes, merged = s
        nb = (n_reads + 1) * 8
        nm, tr = (name_bytes if records else 0), (truth_bytes if truth else 0)          # the entry point reads them only then
        o_b = up(n_reads * DESC); o_a1 = o_b + up(N); o_a2 = o_a1 + up(n)                                    # noqa: E702
        o_p1 = o_a2 + up(n); o_p2 = o_p1 + (up(n * 24) if have_p else 0); o_no = o_p2 + (up(n * 20) if have_p else 0)   # noqa: E702
        o_nm = o_no + (up(nb) if records else 0); o_to = o_nm + (up(nm) if records else 0)                   # noqa: E702
        o_tr = o_to + (up(nb) if truth else 0); o_m = o_tr + (up(tr) if truth else 0)                        # noqa: E702
        regions = [("reads", n_reads * DESC), ("bases", N), ("a1", n), ("a2", n), ("p1", 24 * n if have_p else 0), ("p2", 20 * n if have_p else 0),
                   ("name_off", nb if records else 0), ("names", nm), ("truth_off", nb if truth else 0), ("truth", tr), ("merged", merged)]
        _check(g, regions, o_m + merged, ("nrv_merge_calls", s))
        assert g["merged"] == o_m


def test_merged_carries(layout):
    """The stripe carries inside a merged block: per kind `sets` of one word per character, the original reads' in front."""
    shapes = [(N, N + max(N - T, 0)) for N, T in [(12, 11), (255, 1), (256, 2), (257, 11), (4097, 32), (100000, 11)]]
    kernels = [("align_kernel", 1, 1), ("errclass_kernel", 8, 1), ("infix_kernel", 8, 2)]
    reqs = [("carry", N, cap, word, sets) for N, cap in shapes for _, word, sets in kernels]
    got = iter(layout(reqs))
    for N, cap in shapes:
        for name, word, sets in kernels:
            g = next(got)
            want = {"align_kernel": up(N) + up(cap), "errclass_kernel": up(N * 8) + up(cap * 8),
                    "infix_kernel": 2 * up(N * 8) + 2 * up(cap * 8)}[name]
            assert g["bytes"] == want and g["hc1"] == sets * up(N * word), (name, N, cap, g)
            assert g["hs0"] % 256 == 0 and g["hs1"] % 256 == 0 and g["hs0"] >= N * word and g["hs1"] >= cap * word, (name, N, cap, g)
            assert sets * g["hs0"] <= g["hc1"] and g["hc1"] + sets * g["hs1"] <= g["bytes"], (name, N, cap, g)


def test_up256(layout):
    xs = [0, 1, 255, 256, 257, 511, 512, (1 << 32) - 1, 1 << 32, (1 << 40) + 1]
    assert [g["up256"] for g in layout([("up256", x) for x in xs])] == [up(x) for x in xs]
