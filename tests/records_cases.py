"""Inputs and the reference loop shared by tests/test_combined_records_host.py and tests/test_gpu_combined_records.py (no test here).

`loop_records` is the per-read restatement of the rule text of include/nanorev.h (nrv_revise_reads_raw_records_begin) in plain
Python: it shares no code with hoststage (no pack_records).  `fai_lines` states the samtools faidx columns of a record the same
way.  The name sets are chosen around the device kernel's store width of 4 bytes (csrc/nrv_pack.h): 1, 3, 4, 5 bytes, 15 / 16 / 17
(a multiple of the width and its neighbours), 255, and one with the `|||` that stands for a blank.  The case builders put merged
reads (seq, qual, off) on top of `report_cases.report_case()` and `edits_cases.carry_case()`; `tiny_reads_case` is 600 reads of
0 - 40 bases in one call: the smallest shape at which the scan over the READS carries across its 256-wide passes."""
import numpy as np

from edits_cases import carry_case
from report_cases import T, report_case

NAME_LENS = (1, 3, 4, 5, 15, 16, 17, 255)


def names_for(R, seed=5):
    """R names whose lengths cycle through NAME_LENS (the first has ONE byte: the first sequence then starts at byte 3 of the blob,
    an odd offset), some of them carrying `|||`."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789_.-", np.uint8)
    out = []
    for r in range(R):
        n = NAME_LENS[r % len(NAME_LENS)]
        nm = alpha[rng.integers(0, alpha.size, n)].tobytes()
        if r % 5 == 4 and n >= 5:
            nm = nm[:1] + b"|||" + nm[4:]
        out.append(nm)
    return out


def loop_records(names, seq, qual, off):
    """(blob bytes, rec_off list) by the rule text, one read at a time."""
    blob, rec_off = b"", [0]
    for r, name in enumerate(names):
        lo, hi = int(off[r]), int(off[r + 1])
        s = bytes(bytearray(int(x) for x in seq[lo:hi]))
        if qual is None:
            rec = b">" + bytes(name) + b"\n" + s + b"\n"
            assert len(rec) == len(name) + (hi - lo) + 3
        else:
            q = bytes(bytearray(int(x) for x in qual[lo:hi]))
            rec = b"@" + bytes(name) + b"\n" + s + b"\n+\n" + q + b"\n"
            assert len(rec) == len(name) + 2 * (hi - lo) + 6
        blob += rec
        rec_off.append(len(blob))
    return blob, rec_off


def fai_lines(names, off, rec_off, fastq, base=0):
    """One samtools faidx line per record: name, length, offset of the first base, linebases, linewidth[, qualoffset]."""
    lines = []
    for r, name in enumerate(names):
        L = int(off[r + 1]) - int(off[r])
        o = base + int(rec_off[r]) + 1 + len(name) + 1
        cols = [bytes(name).decode(), str(L), str(o), str(L), str(L + 1)] + ([str(o + L + 3)] if fastq else [])
        lines.append("\t".join(cols))
    return lines


def parse_records(blob, fastq):
    """A blob of well-formed records -> [(name, seq, qual | None)] by splitting at newlines; raises when it is not well-formed."""
    lines = bytes(blob).split(b"\n")
    assert lines[-1] == b"", "the blob does not end with a newline"
    lines = lines[:-1]
    per = 4 if fastq else 2
    assert len(lines) % per == 0, len(lines)
    out = []
    for k in range(0, len(lines), per):
        head = lines[k]
        assert head[:1] == (b"@" if fastq else b">"), head[:20]
        if fastq:
            assert lines[k + 2] == b"+" and len(lines[k + 3]) == len(lines[k + 1])
        out.append((head[1:], lines[k + 1], lines[k + 3] if fastq else None))
    return out


def merged_of(c, fastq, T=T):
    """The merged reads of a calls case (report_case / carry_case at window length T): (seq, qual | None, off), by the host
    definition of the merge."""
    from nanoreviser_amd import hoststage as hs
    return hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], c["qc"] if fastq else None, T)


def report_records_case(fastq, T=T):
    """`report_case(T)` merged: a read boundary on a tile edge, empty reads first, in the middle and last."""
    c = report_case(T=T)
    seq, qual, off = merged_of(c, fastq, T)
    return {"names": names_for(len(c["ev_len"])), "seq": seq, "qual": qual, "off": off, "calls": c}


def carry_records_case(fastq, T=T):
    """`carry_case(T)` merged: 257 * 256 + 3 events in four reads, one record spanning many workgroups of the copy."""
    c = carry_case(False, T=T)
    seq, qual, off = merged_of(c, fastq, T)
    return {"names": names_for(len(c["ev_len"]), seed=6), "seq": seq, "qual": qual, "off": off, "calls": c}


def tiny_reads_case(fastq, R=600, seed=8):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 41, R)
    L[[0, 255, 256, 257, R - 1]] = [0, 40, 0, 1, 0]
    off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(off[-1]))].copy()
    qual = rng.integers(34, 74, int(off[-1])).astype(np.uint8) if fastq else None
    return {"names": names_for(R, seed=seed), "seq": seq, "qual": qual, "off": off}


def empty_reads_case(fastq, R=5):
    z = np.zeros(0, np.uint8)
    return {"names": names_for(R), "seq": z, "qual": z if fastq else None, "off": np.zeros(R + 1, np.int64)}


def no_reads_case(fastq):
    z = np.zeros(0, np.uint8)
    return {"names": [], "seq": z, "qual": z if fastq else None, "off": np.zeros(1, np.int64)}


def name_lengths_case(fastq, seed=3):
    """One read per name length, read lengths around the store width as well (0 .. 9 bases)."""
    rng = np.random.default_rng(seed)
    names = names_for(2 * len(NAME_LENS) + 2, seed=seed)
    L = np.array([(3 * r + 1) % 10 for r in range(len(names))], np.int64)
    off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(off[-1]))].copy()
    qual = rng.integers(34, 74, int(off[-1])).astype(np.uint8) if fastq else None
    return {"names": names, "seq": seq, "qual": qual, "off": off}


EDGE_CASES = {"no reads": no_reads_case, "empty reads": empty_reads_case, "name lengths": name_lengths_case, "600 tiny reads": tiny_reads_case}
