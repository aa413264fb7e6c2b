#!/usr/bin/env python3
"""Pin hoststage.align_labels / label_strings to the reference's own label code: tests/golden/labels_reference.json.

The reference derives a read's training labels from an external mapper's SAM record (NanoReviser_train.py ->
nanorevutils/nanorevtrainutils.py): `parse_sam_record` (nanorevutils/alignutils.py) turns the record and the genome into the
aligned read / reference / column-type lists and the clipped bases at both ends, `clean_read_map_ref`
(nanorevutils/preprocessing.py) folds the deleted reference characters into the read base in front of them, and
`get_base_label` gives the class numbers - `refvals` (model1's six classes), `refvals2` (model2's five), `mapvals`.

    python tools/make_label_goldens.py --reference /path/to/nanoreviser

For every case below - a region, a read, a strand and bounds - this script takes OUR alignment (hoststage.align_columns),
writes it as the SAM record a mapper would have emitted, and records what the reference's three functions make of it:
  * leading and trailing I runs become S clips (the reference cannot take a CIGAR that begins with I), diagonal columns M;
  * on the reverse strand the CIGAR is reversed, the flag is 16, seq is the reverse complement of the read and
    pos = m - end + 1 (1-based on the region as given); on the forward strand pos = start + 1.
The reference is imported only here, when the script runs; only data is written - no reference source is copied into the repo.
tests/test_labels_host.py consumes the file: `label_strings(align_labels(...))` cut to [clip_start : n - clip_end] must equal the
recorded mapvals / refvals / refvals2, and the clipped bases must equal clip_start / clip_end.

Kept out of the cases: equal non-ACGT pairs (the reference calls N / N a match, this project does not), paths that begin or end
with D and a D next to a clip (the reference mishandles both; the infix placement never produces them)."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "labels_reference.json")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(t):
    return bytes(t).translate(_COMP)[::-1]


def _load(ref_root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cigar_of(cols):
    out, k = [], 0
    while k < len(cols):
        e = k
        while e < len(cols) and cols[e] == cols[k]:
            e += 1
        out.append((e - k, cols[k]))
        k = e
    return out


def cases(rng):
    """(name, region, read, reverse, start, end): small, both strands, D runs of 1 and of 3 and more, I runs, clips at both ends,
    an N in the truth opposite a different read base."""
    def rnd(n):
        return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()

    def other(c):                                                      # a base that is not c: a clipped base must not match its neighbour
        return b"A" if c != b"A" else b"C"
    out = []
    core = [rnd(24) for _ in range(13)]
    edits = [
        ("exact", lambda t: t),
        ("one substitution", lambda t: t[:9] + (b"A" if t[9:10] != b"A" else b"C") + t[10:]),
        ("D run of 1", lambda t: t[:8] + t[9:]),
        ("D run of 3", lambda t: t[:10] + t[13:]),
        ("D run of 5", lambda t: t[:7] + t[12:]),
        ("I run of 1", lambda t: t[:11] + (b"G" if t[11:12] != b"G" else b"T") + t[11:]),
        ("I run of 4", lambda t: t[:6] + b"ACGT" + t[6:]),
        ("D run of 1 and D run of 3", lambda t: t[:4] + t[5:14] + t[17:]),
        ("I run and D run", lambda t: t[:5] + b"TT" + t[5:15] + t[18:]),
        ("clip at the start", lambda t: other(t[:1]) * 3 + t),
        ("clip at the end", lambda t: t + other(t[-1:]) * 3),
        ("clips at both ends and a D run of 3", lambda t: other(t[:1]) * 2 + t[:12] + t[15:] + other(t[-1:]) * 4),
        ("clips at both ends, I run and D run of 1", lambda t: other(t[:1]) + t[:6] + other(t[6:7]) * 2 + t[6:16] + t[17:] + other(t[-1:]) * 2),
    ]
    for k, ((what, f), t) in enumerate(zip(edits, core)):
        for rev in (0, 1):
            flank_a, flank_b = rnd(5 + k % 3), rnd(4 + k % 2)
            region = flank_a + t + flank_b
            region_given = revcomp(region) if rev else region
            out.append((f"{what} {'+-'[rev]}", region_given, f(t), rev, len(flank_a), len(flank_a) + len(t)))
    # an N in the truth opposite a different read base (never opposite an N: the reference would call that a match)
    t = rnd(20)
    tn = t[:7] + b"N" + t[8:]
    for rev in (0, 1):
        out.append((f"N in the truth {'+-'[rev]}", revcomp(b"AC" + tn + b"GT") if rev else b"AC" + tn + b"GT", t, rev, 2, 22))
    tn2 = t[:3] + b"N" + t[4:12] + b"N" + t[13:]
    out.append(("two N in the truth and a D run of 1 +", b"T" + tn2 + b"A", t[:16] + t[17:], 0, 1, 21))
    out.append(("two N in the truth and a D run of 1 -", revcomp(b"T" + tn2 + b"A"), t[:16] + t[17:], 1, 1, 21))
    # longer, mutated
    for k in range(10):
        t = rnd(40 + 3 * k)
        s = bytearray()
        for c in t:
            r = rng.random()
            if r < 0.05:
                continue
            s.append(c if r > 0.10 else b"ACGT"[rng.integers(0, 4)])
            if r > 0.95:
                s.append(b"ACGT"[rng.integers(0, 4)])
        rev = k % 2
        fa, fb = rnd(6), rnd(7)
        region = fa + t + fb
        out.append((f"mutated #{k} {'+-'[rev]}", revcomp(region) if rev else region, bytes(s), rev, 6, 6 + len(t)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of pkubioinformatics/nanoreviser")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from nanoreviser_amd import hoststage as hs
    au = _load(args.reference, "nanorevutils/alignutils.py", "_ref_alignutils")
    pp = _load(args.reference, "nanorevutils/preprocessing.py", "_ref_preprocessing")
    rng = np.random.default_rng(20260)
    rows, skipped = [], []
    for name, region, read, rev, start, end in cases(rng):
        cols = hs.align_columns(region, read, rev, start, end)
        core = cols.strip("I")
        if not core or core[0] == "D" or core[-1] == "D":             # the reference cannot take these: not a case
            skipped.append(name)
            continue
        lead, trail = len(cols) - len(cols.lstrip("I")), len(cols) - len(cols.rstrip("I"))
        cg = ([(lead, "S")] if lead else []) + cigar_of(list(core)) + ([(trail, "S")] if trail else [])
        m = len(region)
        if rev:
            cg = cg[::-1]
        rec = {"qName": name.replace(" ", "_"), "flag": "16" if rev else "0", "rName": "region", "pos": str(m - end + 1 if rev else start + 1),
               "mapq": "60", "cigar": "".join(f"{k}{c}" for k, c in cg), "rNext": "*", "pNext": "0", "tLen": "0",
               "seq": (revcomp(read) if rev else read).decode(), "qual": "*"}
        readVals, refVals, mapVals, loc, clip_s, clip_e = au.parse_sam_record(rec, {"region": region.decode()})
        c_read, c_map, c_ref, c_ref2 = pp.clean_read_map_ref(readVals, mapVals, refVals)
        rows.append({"name": name, "region": region.decode(), "read": read.decode(), "reverse": int(rev), "start": int(start), "end": int(end),
                     "sam": {k: rec[k] for k in ("flag", "pos", "cigar", "seq")},
                     "mapvals": "".join(c_map), "refvals": "".join(str(pp.get_base_label(c)) for c in c_ref),
                     "refvals2": "".join(str(pp.get_base_label(c)) for c in c_ref2), "readvals": "".join(c_read),
                     "start_clipped_bases": int(clip_s), "end_clipped_bases": int(clip_e), "strand": loc["Strand"]})
    with open(args.out, "w") as fp:
        json.dump({"source": "nanorevutils/alignutils.py parse_sam_record, nanorevutils/preprocessing.py clean_read_map_ref, get_base_label",
                   "cases": rows}, fp, indent=1)
        fp.write("\n")
    print("wrote", args.out, len(rows), "cases;", len(skipped), "skipped:", skipped)
    return 0


if __name__ == "__main__":
    sys.exit(main())
