"""Command line of the MI355X reviser: the reference's `NanoReviser.py` contract, fast5 in,
`<read>_out.fasta` / `_out.fastq` out.

Kept from the reference (NanoReviser.py:42-95, 105-236):
  * the flag surface  -d -o -F -S --thread -t -e -g -s --test_mode --model1_predict_dir
    --model2_predict_dir -v ;
  * weight path convention ./model/<S>/<S>_win13_50ep_model{1,2}.h5 (:191-193);
  * one output file per read, `<output_dir><stem>_out.<fmt>` with stem = name up to the first '.'
    (:137, :163) and the record layout of output_handeler.py:26-62;
  * the failure contract: any error while revising a read writes the ORIGINAL basecalls instead
    (:146-152 fasta, :173-179 fastq via extract_fastq) - and, which the reference parses but never
    does (:63-65), the read is listed in the --failed_read file.
Changed on purpose:
  * the network is actually executed (the reference shells out to a missing Guppy binary,
    SURVEY.md F1): per read  events -> bases -> signal windows/features (hoststage) ->
    nrv_predict_read on the GPU -> merge (hoststage.revise_read);
  * no tmp-dir copies (the -t flag is accepted and ignored; the reference's per-slot tmp dirs race,
    :111) and no file is dropped when the count is not a multiple of the pool size (:212);
  * reads are sharded over the visible GPUs, one worker process per GPU, no collectives
    (--gpus, default all); --thread bounds the host-stage worker processes per GPU worker;
  * explicitly given --model{1,2}_predict_dir win over -S (in the reference -S always overrides
    them, which makes those flags dead, :191-193);
  * --resume: a rerun skips the reads whose output file exists, EXCEPT those the earlier run listed in its
    failed-reads file (their output is the unrevised fallback: they are revised again and replaced; the
    reference clears temp_dir and re-revises / overwrites every read, :196-201; SURVEY.md 5
    "skip-if-exists is a free resume"); --resume_keep_failed leaves those files alone and returns 3;
  * each GPU worker is pinned to the cores of its GPU's NUMA node (`worker_cpus`), and a very long
    read (BASELINE config 5) is split over the GPU workers by window range with a T-1-event halo
    (`shard.split_read_windows`, `plan_splits`): still no device-to-device exchange.
FASTQ qualities: the reviser has no Guppy qualities; each revised base gets
Phred = -10 log10(1 - min(p_model1, p_model2)) of its call (capped 1..40), unrevised edge bases '#'.
"""
from __future__ import annotations

import argparse
import math
import os
import queue
import sys
import threading
import time
from collections import deque
from concurrent.futures import Future, ProcessPoolExecutor, ThreadPoolExecutor
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import h5lite
from . import hostlib
from . import hoststage as hs
from .shard import shard_reads, split_read_windows
from .weights import load_model

VERSION = "1.0"


def get_args(argv: Optional[Sequence[str]] = None):
    p = argparse.ArgumentParser(
        prog="NanoReviser.py", usage="%(prog)s [-d] [-o]",
        description="An Error-correction Tool for Nanopore Sequencing Based on a Deep Learning Algorithm "
                    "(MI355X engine)")
    p.add_argument("-d", "--fast5_base_dir", dest="fast5_base_dir", help="path to the fast5 files")
    p.add_argument("-o", "--output_dir", dest="output_dir", default="./unitest/nanorev_output/",
                   help="path to store the output files")
    p.add_argument("-F", "--output_format", dest="output_format", default="fasta",
                   help="format of the output files, default is fasta")
    p.add_argument("-S", "--species", dest="species", default="human", help="ecoli or human")
    p.add_argument("--thread", dest="thread", type=int, default=100,
                   help="host parsing threads per GPU worker (capped at the core count)")
    p.add_argument("-t", "--tmp_dir", dest="temp_dir", default="./unitest/tmp/", help="accepted, unused")
    p.add_argument("-e", "--failed_read", dest="failed_reads_filename", default="failed_reads.txt",
                   help="document to log the failed reads")
    p.add_argument("-g", "--basecall_group", dest="basecall_group", default="Basecall_1D_000")
    p.add_argument("-s", "--basecall_subgroup", dest="basecall_subgroup", default="BaseCalled_template")
    p.add_argument("--test_mode", action="store_true", default=False, help="just for unitest")
    p.add_argument("--model1_predict_dir", dest="model1_predict_dir", default=None)
    p.add_argument("--model2_predict_dir", dest="model2_predict_dir", default=None)
    p.add_argument("-v", "--virsion", action="store_true", dest="virsion", help="version of NanoReviser")
    p.add_argument("--gpus", type=int, default=0, help="GPUs to use (0 = all visible)")
    p.add_argument("--batch", type=int, default=4096, help="windows per device launch group")
    p.add_argument("--model_dir", default=None, help="root of model/<species>/ (default: next to the package)")
    p.add_argument("--resume", action="store_true", default=False,
                   help="skip every read whose <stem>_out.<format> already exists and is not empty (outputs are written "
                        "through a temporary + rename, so an existing file is a complete one) - except the reads the earlier "
                        "run listed in its failed-reads file: their output holds the ORIGINAL basecalls (a GPU worker died, "
                        "the engine failed), so they are revised again and the file is replaced")
    p.add_argument("--resume_keep_failed", action="store_true", default=False,
                   help="with --resume: do not redo the reads of the failed-reads file either; they stay listed there and "
                        "the exit code is 3 while any of them is left")
    p.add_argument("--split_reads_above", type=float, default=float(os.environ.get("NRV_SPLIT_READS_MB", "4")),
                   help="with more than one GPU: a fast5 file above this many MB (~10 MB per 100 k events) AND above a GPU "
                        "worker's fair share of the input has its window range split over the workers, T-1 events of halo "
                        "per slice (0 = never)")
    p.add_argument("--device_stats", action="store_true", default=False,
                   help="compute the read statistics (median / MAD of a read, per-base mean / std, feature columns 1 - 2) on the "
                        "GPU instead of in the host stage: a third less host work per read, the same output byte for byte "
                        "(also NRV_DEVICE_STATS=1).  Off by default.  Applies to the pipelined native-bundle path; these stay "
                        "host-fed: the Python fallback reader (libnanorev_host.so not built, or a file it declines), "
                        "NRV_CLI_PIPELINE=0, several engines per device (NRV_CLI_ENGINES), reads whose window range is split "
                        "over GPU workers (a slice needs the whole read's median), and any read with a base of more than "
                        "16384 samples")
    p.add_argument("--device_merge", action="store_true", default=False,
                   help="merge the two models' calls, compute the per-base quality and pack the revised reads on the GPU instead "
                        "of in the host stage: 2 - 4 bytes per base come back instead of 46 and a device call's reads are "
                        "written by one native task, the same output byte for byte (also NRV_DEVICE_MERGE=1).  Off by default.  "
                        "Applies where --device_stats applies (the pipelined native-bundle path) and composes with it; the "
                        "Python fallback reader, NRV_CLI_PIPELINE=0, several engines per device, reads whose window range is "
                        "split over GPU workers, a library without the new entry points and the per-read retry after a failed "
                        "call keep the host merge")
    p.add_argument("--report", dest="report", default=None, metavar="FILE",
                   help="write a per-read revision report to FILE (also NRV_REPORT=FILE): a TSV with one header line, one line "
                        "per input read sorted by file name - name, status (revised / unrevised), bases in / out, edge bases, "
                        "windows confirmed / substituted / inserted / deleted / undecided, the class histograms of both models, "
                        "how often model 2 agrees with the basecaller, calls on a softmax near-tie, the sum of the qualities - "
                        "and a last line #total with the sums over the revised reads.  With --device_merge the numbers are "
                        "counted on the GPU behind the merge, everywhere else by the host stage from the calls it holds: the "
                        "same file byte for byte.  Off by default; without it nothing changes")
    p.add_argument("--report_tie_eps", dest="report_tie_eps", type=float, default=hs.REPORT_TIE_EPS,
                   help="a call is a near-tie when top1 - top2 of either model's softmax row is below this (default 4e-4: what two "
                        "precision modes that both meet the parity bar can differ by)")
    p.add_argument("--edits", dest="edits", default=None, metavar="DIR",
                   help="write a per-read edit list into DIR (also NRV_EDITS=DIR): for every read that is written a file "
                        "<stem>_edits.tsv with one header line and one line per base the revision substituted (S), inserted (I) or "
                        "deleted (D) - position in the original read, position in the revised read, kind, original base, new base "
                        "('-' for a deletion), the call's quality character ('.' in FASTA runs) and the confidence the quality is "
                        "computed from.  A read written unrevised gets the header alone.  With --device_merge the list is compacted on "
                        "the GPU behind the merge, everywhere else it is formed by the host stage from the calls it holds: the same "
                        "files byte for byte.  Off by default; without it nothing changes and DIR is not created")
    p.add_argument("--combined", dest="combined", default=None, metavar="FILE",
                   help="write every read's record into ONE file, FILE, instead of one <stem>_out.<format> per read (also "
                        "NRV_COMBINED=FILE): well-formed FASTA / FASTQ records without line wrapping (in FASTQ a newline in front of "
                        "'+' and one at the end, which the per-read files leave out), sequence and quality lines exactly those of the "
                        "per-read files, plus FILE.fai in samtools faidx layout.  With --device_merge the records are laid out on the "
                        "GPU behind the merge and a device call's reads are appended with one write; everywhere else the host stage "
                        "forms them from the reads it holds: the same records.  Their order is not specified beyond the reads of one "
                        "device call staying together.  --report and --edits work unchanged next to it; --resume does not.  Off by "
                        "default; without it nothing changes and FILE is not created")
    p.add_argument("--summary", dest="summary", default=None, metavar="FILE",
                   help="write a per-read sequencing summary to FILE (also NRV_SUMMARY=FILE): a TSV with one header line, one line "
                        "per input read sorted by file name - name, status (revised / unrevised), bases, mean and median quality "
                        "(the mean is that of the error probabilities, as Guppy and NanoStat define it), bases of Q10 / Q20 / Q30 and "
                        "more, GC content, the counts of A / C / G / T / other - then a line #total over the revised reads and a "
                        "line #reads with the revised and unrevised reads and the N50 of the revised ones.  The qualities are those "
                        "of the FASTQ form of the run, in FASTA runs too; a read written unrevised has its base counts and no "
                        "quality.  With --device_merge the counts are made on the GPU behind the merge, everywhere else by the host "
                        "stage from the calls it holds: the same file byte for byte.  Off by default; without it nothing changes")
    p.add_argument("--trim_q", dest="trim_q", type=int, default=None, metavar="Q",
                   help="cut every revised read down to the part a sliding quality window keeps (also NRV_TRIM_Q=Q): the read is "
                        "written from the first to the last window of --trim_window bases whose mean quality is at least Q "
                        "(1 .. 40; integers: the window's Phred values add up to Q x W or more), and a read whose kept part is "
                        "shorter than --min_len is DROPPED - no output file, no record in --combined, not a failed read.  The "
                        "qualities are those of the FASTQ form of the run, in FASTA runs too; the first and last bases of a read "
                        "have no window and Phred 2, so any Q above 2 cuts them off.  A read written unrevised is written whole.  "
                        "--report, --edits and --summary keep describing the UNTRIMMED revision (positions, counts): their bytes "
                        "are what they are without the trim.  With --device_merge the bounds are found on the GPU behind the merge "
                        "and the records of --combined are cut there, everywhere else the host stage applies them: the same files "
                        "byte for byte.  --resume does not work with it.  Off by default; without it nothing changes")
    p.add_argument("--trim_window", dest="trim_window", type=int, default=10, metavar="W",
                   help="with --trim_q: bases per window, 1 .. 64 (default 10)")
    p.add_argument("--min_len", dest="min_len", type=int, default=1, metavar="L",
                   help="with --trim_q: a read with fewer than L bases left is dropped (default 1; 0 keeps empty reads)")
    p.add_argument("--trim_log", dest="trim_log", default=None, metavar="FILE",
                   help="with --trim_q: write what the trim did to FILE, a TSV with one header line, one line per input read sorted "
                        "by file name - name, status (revised / unrevised), bases of the untrimmed read, lo, hi, kept (1 / 0) - "
                        "and a last line #total with the sums over the revised reads.  The same file on every route")
    p.add_argument("--truth", dest="truth", default=None, metavar="FASTA",
                   help="the true sequence of the reads, for --accuracy (also NRV_TRUTH=FASTA): a FASTA file whose records may be "
                        "wrapped and are upper-cased on load; the first word of a header is the read's name, matched against the "
                        "fast5 file name with or without .fast5.  A name that occurs twice is an error.  A read without a record "
                        "has no truth")
    p.add_argument("--accuracy", dest="accuracy", default=None, metavar="FILE",
                   help="with --truth: write to FILE (also NRV_ACCURACY=FILE) how far every read is from its truth before and "
                        "after the revision, a TSV with one header line, one line per input read sorted by file name - name, "
                        "status (revised / unrevised), truth_len, len_in, dist_in, len_out, dist_out, id_in, id_out - then a line "
                        "#total with the sums over the reads with a truth and the pooled identities and a line #reads with the "
                        "reads with a truth, without one and too long.  dist is the global unit-cost edit distance (only equal "
                        "A / C / G / T match), id = 1 - dist / max(len, truth_len); the revised read is the untrimmed one.  "
                        "With --device_merge the distances are found on the GPU behind the merge, everywhere else by the host "
                        "stage at about 0.1 s per read: the same file byte for byte.  --resume does not work with it.  Off by "
                        "default; without it nothing changes")
    p.add_argument("--accuracy_max_len", dest="accuracy_max_len", type=int, default=65536, metavar="L",
                   help="with --accuracy: a read whose truth or original length exceeds L is treated as having no truth and "
                        "counted as too_long (default 65536)")
    p.add_argument("--error_classes", dest="error_classes", default=None, metavar="FILE",
                   help="with --truth and --accuracy: write to FILE (also NRV_ERROR_CLASSES=FILE) which errors separate every read "
                        "from its truth before and after the revision, a TSV with one header line, one line per input read sorted "
                        "by file name - name, status, truth_len, then for the original and for the revised (untrimmed) read its "
                        "length and the matched, substituted, inserted (absent from the truth) and deleted (absent from the read) "
                        "characters of the alignments with the fewest edits that match the most characters - then a line #total "
                        "with the sums over the reads with a truth and the pooled substitution / insertion / deletion rates per "
                        "truth base before and after, and a line #reads as in --accuracy.  It shares --accuracy_max_len.  With "
                        "--device_merge the counts are found on the GPU behind the merge, everywhere else by the host stage at "
                        "about 0.3 s per read: the same file byte for byte.  Off by default; without it nothing changes")
    p.add_argument("--infix", dest="infix", default=None, metavar="FILE",
                   help="with --truth (--accuracy is not needed): treat every truth as a REGION that holds the read somewhere, on "
                        "either strand, and write to FILE (also NRV_INFIX=FILE) where the original and the revised (untrimmed) "
                        "read lie in it, a TSV with one header line, one line per input read sorted by file name - name, status, "
                        "truth_len, strand, then for both forms of the read its length, dist, match, start, end and id - then a "
                        "line #total with the summed integers and the pooled identities and a line #reads as in --accuracy.  "
                        "Among all substrings of the region the one with the fewest edits, then the most matched columns, then "
                        "the largest start, then the smallest end; strand is - when the ORIGINAL read fits the reverse complement "
                        "strictly better, and both forms are reported on that strand; start / end are 0-based half-open on the "
                        "region as given; id = match / (match + dist).  --accuracy_max_len applies, capped at 2097151.  With "
                        "--device_merge the figures are found on the GPU behind the merge, everywhere else by the host stage at "
                        "about 2 s per read: the same file byte for byte.  --resume does not work with it.  Off by default; "
                        "without it nothing changes")
    p.add_argument("--infix_strand", dest="infix_strand", default="both", choices=("both", "forward"),
                   help="with --infix: try both strands of a region (default) or the forward strand alone")
    p.add_argument("--labels", dest="labels", default=None, metavar="DIR",
                   help="with --truth and --infix: write the per-base training labels of every read into DIR (also "
                        "NRV_LABELS=DIR).  The ORIGINAL bases of a read whose --infix line is with_truth are aligned against its "
                        "region on that line's strand at start_in:end_in - revised or written unrevised alike - and "
                        "DIR/<stem>_labels.txt gets five lines: #name, strand, start, end, len, match, sub, ins, del, clip_start, "
                        "clip_end, lead_del (tab separated); the bases; per base M / X / I, or D where deleted truth characters "
                        "follow; label1 (0 D, 1 -, 2 C, 3 T, 4 G, 5 A: the truth character opposite the base, 0 where a deletion "
                        "follows); label2 (the same without the deletions).  A read without a truth, or whose length or "
                        "end - start exceeds 65536, gets no file.  DIR/labels.tsv has a header, one line per input read sorted by "
                        "file name - name, status (with_truth / no_truth / too_long), strand, start, end, len, the seven figures, "
                        "the counts of label1 = 0 .. 5 and of label2 = 0 .. 5 -, a line #total with the sums (the class balance) "
                        "and a line #reads.  With --device_merge the labels of a device call's reads are found on the GPU by one "
                        "call while the next is in flight (not timed yet), everywhere else by the host stage: the same files "
                        "byte for byte.  Off by default; without it nothing changes")
    p.add_argument("--score", dest="score", default=None, metavar="FILE",
                   help="with --labels_from: score both classifiers against the per-base labels an earlier --labels run wrote and "
                        "write the result to FILE (also NRV_SCORE=FILE): what Keras' model.evaluate gives for this pair of models.  "
                        "Neither --truth nor --infix is needed.  A window counts when the base it revises has a label (clipped ends "
                        "and bases opposite no A / C / G / T have none).  One header line, one line per input read sorted by file "
                        "name - name, status (scored; stale_labels: the labels file holds other bases; no_labels: no file; "
                        "unrevised), windows, labelled, correct1, correct2, acc1, acc2, loss1, loss2 (categorical cross-entropy in "
                        "nats, from an integer -log2 in units of 2^-16 bit), the twenty counts decision x kind (confirmed, "
                        "substituted, inserted, deleted, undecided x M, X, I, D: what the merge did to a base that matches, "
                        "mismatches, is an insertion, is followed by a deletion) and sub_right (substitutions to the truth's base) - "
                        "then #total, #confusion1 (6 lines: true class x answer), #confusion2 (5 lines), #calibration1 / "
                        "#calibration2 - per non-empty confidence bin the Phred the quality rule gives it, n, ok and the empirical "
                        "Phred -10 log10((n - ok + 0.5) / (n + 1)) - and #reads scored / stale_labels / no_labels / unrevised.  With "
                        "--device_merge the counts are found on the GPU behind the merge (not timed yet), everywhere else by the "
                        "host stage: the same file byte for byte.  --resume does not work with it.  Off by default; without it "
                        "nothing changes")
    p.add_argument("--labels_from", dest="labels_from", default=None, metavar="DIR",
                   help="with --score: the directory an earlier run's --labels wrote (also NRV_LABELS_FROM=DIR); never this run's own")
    a = p.parse_args(argv)
    a.score = a.score or (os.environ.get("NRV_SCORE", "").strip() or None)
    a.labels_from = a.labels_from or (os.environ.get("NRV_LABELS_FROM", "").strip() or None)
    a.infix = a.infix or (os.environ.get("NRV_INFIX", "").strip() or None)
    a.labels = a.labels or (os.environ.get("NRV_LABELS", "").strip() or None)
    a.error_classes = a.error_classes or (os.environ.get("NRV_ERROR_CLASSES", "").strip() or None)
    a.truth = a.truth or (os.environ.get("NRV_TRUTH", "").strip() or None)
    a.accuracy = a.accuracy or (os.environ.get("NRV_ACCURACY", "").strip() or None)
    if a.labels and not (a.truth and a.infix):
        print("[！！！Error] --labels goes with --truth and --infix", file=sys.stderr)
        raise SystemExit(2)
    if (a.score is None) != (a.labels_from is None):
        print("[！！！Error] --score goes with --labels_from", file=sys.stderr)
        raise SystemExit(2)
    if a.score and a.labels and os.path.abspath(a.labels_from) == os.path.abspath(a.labels):
        print("[！！！Error] --labels_from cannot be the directory this run's --labels writes: the labels of a read are formed "
              "after the call that would score it", file=sys.stderr)
        raise SystemExit(2)
    if a.score and a.resume:
        print("[！！！Error] --resume cannot be used with --score: a skipped read's calls are not at hand", file=sys.stderr)
        raise SystemExit(2)
    if a.infix and not a.truth:
        print("[！！！Error] --infix goes with --truth", file=sys.stderr)
        raise SystemExit(2)
    if (a.truth is None) != (a.accuracy is None) and not (a.infix and a.truth):
        print("[！！！Error] --truth and --accuracy go together", file=sys.stderr)
        raise SystemExit(2)
    if a.infix and a.resume:
        print("[！！！Error] --resume cannot be used with --infix: a skipped read's written form is not at hand", file=sys.stderr)
        raise SystemExit(2)
    if a.accuracy and a.resume:
        print("[！！！Error] --resume cannot be used with --accuracy: a skipped read's written form is not at hand", file=sys.stderr)
        raise SystemExit(2)
    if a.error_classes and not (a.truth and a.accuracy):
        print("[！！！Error] --error_classes goes with --truth and --accuracy", file=sys.stderr)
        raise SystemExit(2)
    if (a.accuracy or a.infix) and a.accuracy_max_len < 0:
        print("[！！！Error] --accuracy_max_len must be 0 or more", file=sys.stderr)
        raise SystemExit(2)
    if a.infix:                           # a packed cell of the infix recurrence holds lengths up to NRV_INFIX_MAX_LEN
        a.accuracy_max_len = min(a.accuracy_max_len, hs.INFIX_MAX_LEN)
    if a.trim_q is None and os.environ.get("NRV_TRIM_Q", "").strip():
        try:
            a.trim_q = int(os.environ["NRV_TRIM_Q"].strip())
        except ValueError:
            print("[！！！Error] NRV_TRIM_Q must be an integer", file=sys.stderr)
            raise SystemExit(2)
    if a.trim_q is not None:
        if not (1 <= a.trim_q <= 40 and 1 <= a.trim_window <= 64 and a.min_len >= 0):
            print("[！！！Error] --trim_q must be in 1 .. 40, --trim_window in 1 .. 64 and --min_len 0 or more", file=sys.stderr)
            raise SystemExit(2)
        if a.resume:
            print("[！！！Error] --resume cannot be used with --trim_q: a dropped read has no output to resume from", file=sys.stderr)
            raise SystemExit(2)
    elif a.trim_log:
        print("[！！！Error] --trim_log needs --trim_q", file=sys.stderr)
        raise SystemExit(2)
    a.summary = a.summary or (os.environ.get("NRV_SUMMARY", "").strip() or None)
    a.combined = a.combined or (os.environ.get("NRV_COMBINED", "").strip() or None)
    if a.combined and a.resume:
        print("[！！！Error] --resume cannot be used with --combined: a combined run cannot be resumed", file=sys.stderr)
        raise SystemExit(2)
    a.edits = a.edits or (os.environ.get("NRV_EDITS", "").strip() or None)
    a.device_stats = bool(a.device_stats) or device_stats_env()
    a.device_merge = bool(a.device_merge) or device_merge_env()
    a.report = a.report or (os.environ.get("NRV_REPORT", "").strip() or None)
    if a.virsion:
        print(f"The virsion of NanoReviser : {VERSION} ")
        raise SystemExit(0)
    if not (a.fast5_base_dir and a.output_dir):
        p.print_help()
        raise SystemExit(0)
    return a


def device_stats_env() -> bool:
    """NRV_DEVICE_STATS=1 (anything but empty / 0): the environment form of --device_stats."""
    return os.environ.get("NRV_DEVICE_STATS", "0").strip() not in ("", "0")


def device_merge_env() -> bool:
    """NRV_DEVICE_MERGE=1 (anything but empty / 0): the environment form of --device_merge."""
    return os.environ.get("NRV_DEVICE_MERGE", "0").strip() not in ("", "0")


def model_paths(args):
    """NanoReviser.py:188-194."""
    root = args.model_dir or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "model")
    sp = "ecoli" if (args.test_mode and not args.species) else args.species
    p1 = args.model1_predict_dir or os.path.join(root, sp, f"{sp}_win13_50ep_model1.h5")
    p2 = args.model2_predict_dir or os.path.join(root, sp, f"{sp}_win13_50ep_model2.h5")
    ok = all(os.path.exists(p) or os.path.exists(os.path.splitext(p)[0] + ".f32") for p in (p1, p2))
    if not ok:
        raise RuntimeError("！！！[Error] model file: Please check the dir of models file!!")
    return p1, p2


def out_name(output_dir: str, fast5_fn: str, fmt: str) -> str:
    # NanoReviser.py:137/163: plain string concatenation with output_dir, stem = up to the first '.'
    return output_dir + fast5_fn.split(".")[0] + "_out." + fmt


def parse_read(path: str, group: str, subgroup: str):
    """fast5 -> (ReadData, fastq text or None).  nanorev_fast5_handeler.py:58-150."""
    d = h5lite.read_fast5(path, group, subgroup)
    ev = d["events"]
    start, length = ev["start"], ev["length"]
    try:
        old = tuple(int(x) for x in d["version"].split(".")[:2]) <= (0, 0)
    except ValueError:
        old = False
    if old:                                   # pre-versioned Albacore: times in seconds (:66-71)
        start = start * 4000 - d["raw_attrs"]["start_time"]
        length = length * 4000
    rd = hs.collapse_events(start, ev["mean"], ev["stdv"], ev["model_state"], ev["move"], d["signal"])
    fq = d["fastq"]                           # bytes (fixed-length string dataset) or str (variable-length)
    if isinstance(fq, (bytes, np.bytes_)):
        fq = bytes(fq).decode("utf8", "replace")
    elif fq is not None:
        fq = str(fq)
    return rd, fq


def phred_chars(p1: np.ndarray, p2: np.ndarray, a1=None, a2=None) -> np.ndarray:
    """Per-window quality from the smaller of the two models' top probabilities.  With the argmax
    arrays the top probability is a gather (p.max(-1) over a 6-wide axis is 10x slower in NumPy)."""
    if a1 is not None and a2 is not None and len(a1) == len(p1):
        idx = np.arange(len(a1))
        conf = np.minimum(p1[idx, a1], p2[idx, a2]).astype(np.float64)
    else:
        conf = np.minimum(p1.max(-1), p2.max(-1)).astype(np.float64)
    q = np.clip(np.round(-10.0 * np.log10(np.maximum(1.0 - conf, 1e-4))), 1, 40).astype(np.int64)
    return (q + 33).astype(np.uint8)


_PHRED_THR = None


def phred_thresholds() -> np.ndarray:
    """float32[39]: entry k - 2 is the smallest f32 confidence for which `phred_chars` yields Phred >= k, k = 2 .. 40.
    `phred_chars` is a monotone step function of the f32 confidence on [0, 1] (checked on the CPU: 5 M random values and
    +-2000 ulps around every step), so 33 + 1 + searchsorted(thr, conf, 'right') reproduces its characters exactly - which is
    how the device merge (csrc/nrv_merge.h) gives the host's quality bytes without a log10.  Found by bisection over the f32 bit
    patterns (ascending with the value on [0, 1]) of `phred_chars` ITSELF, once per process."""
    global _PHRED_THR
    if _PHRED_THR is None:
        def q(bits):
            c = bits.astype(np.uint32).view(np.float32).reshape(-1, 1)
            return phred_chars(c, c).astype(np.int64) - 33
        k = np.arange(2, 41, dtype=np.int64)
        lo, hi = np.zeros(39, np.int64), np.full(39, 0x3F800000, np.int64)        # q(0.0) = 1 < k <= 40 = q(1.0)
        assert (q(lo) < k).all() and (q(hi) >= k).all()
        while (hi - lo > 1).any():
            mid = lo + (hi - lo) // 2
            up = q(mid) >= k
            hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
        thr = hi.astype(np.uint32).view(np.float32).copy()
        thr.flags.writeable = False
        _PHRED_THR = thr
    return _PHRED_THR


def phred_lookup(conf) -> np.ndarray:
    """`phred_chars` through the table: uint8 characters for f32 confidences (what the device computes per window)."""
    return (33 + 1 + np.searchsorted(phred_thresholds(), np.asarray(conf, np.float32), "right")).astype(np.uint8)


def _merge_read(T: int, bases, a1, a2, qc):
    """Original bases of one read + its calls -> (revised sequence, per-base quality string or None); qc: per-window Phred
    characters (FASTQ) or None (FASTA)."""
    codes = np.frombuffer(np.asarray(bases, dtype="S1").tobytes(), dtype=np.uint8)
    off, n = (T - 1) // 2, len(a1)
    if n == 0:
        return codes.tobytes().decode("ascii"), "#" * len(codes)
    first, second, count = hs.merge_calls(codes[off:off + n], a1, a2)
    z = qc if qc is not None else np.zeros(n, np.uint8)
    seq_mid, q_mid = hs.expand_calls(first, second, count, z, z)
    seq = (codes[:off].tobytes() + seq_mid.tobytes() + codes[off + n:].tobytes()).decode("ascii")
    if qc is None:
        return seq, None
    edge = np.full(1, ord("#"), np.uint8)
    qual = np.repeat(edge, off).tobytes() + q_mid.tobytes() + np.repeat(edge, len(codes) - off - n).tobytes()
    return seq, qual.decode("ascii")


def _finish_read(T: int, rt, p1, p2, a1, a2, want_qual: bool = True):
    """Calls of one read -> (revised sequence, per-base quality string or None)."""
    return _merge_read(T, rt.bases, a1, a2, phred_chars(p1, p2, a1, a2) if want_qual and len(a1) else None)


def predict_one(reviser, rt):
    """Device side of one read -> (p1, p2, a1, a2) over its N-T windows."""
    if isinstance(rt, hs.RawReadTensors):
        return reviser.predict_reads_raw([rt.raw], [rt.starts], [rt.feat_ev], [rt.shift], [rt.scale])
    return reviser.predict_read(rt.sig_ev, rt.feat_ev)


def prepare_many(reviser_cls, rts, T):
    """The NumPy half of `predict_many` for raw reads (concatenation, descriptors, output arrays), done outside the
    engine thread; None when the batch cannot take the packed path (mixed tensor kinds, an engine without it)."""
    pack = getattr(reviser_cls, "pack_reads_raw", None)
    if pack is None or not all(isinstance(rt, hs.RawReadTensors) for rt in rts):
        return None
    return pack([rt.raw for rt in rts], [rt.starts for rt in rts], [rt.feat_ev for rt in rts],
                [rt.shift for rt in rts], [rt.scale for rt in rts], T)


def predict_many(reviser, rts, packed=None):
    """Several reads in ONE device call: their per-event arrays are concatenated, the engine forms
    every sliding window of the concatenation, and the T windows that straddle each read boundary
    are simply not used (0.2 % extra work; full launch groups, one host<->device round trip).
    Returns one (p1, p2, a1, a2) per read."""
    if len(rts) == 1 and packed is None:
        return [predict_one(reviser, rts[0])]
    T = reviser.T
    if packed is not None:
        p1, p2, a1, a2 = reviser.run_packed_raw(packed)
    elif all(isinstance(rt, hs.RawReadTensors) for rt in rts):
        # raw samples + event starts cross PCIe; the (N,50) windows are cut on the device
        p1, p2, a1, a2 = reviser.predict_reads_raw([rt.raw for rt in rts], [rt.starts for rt in rts],
                                                   [rt.feat_ev for rt in rts], [rt.shift for rt in rts],
                                                   [rt.scale for rt in rts])
    else:
        sig = np.concatenate([rt.sig_ev for rt in rts])
        feat = np.concatenate([rt.feat_ev for rt in rts])
        p1, p2, a1, a2 = reviser.predict_read(sig, feat)
    return _slice_calls((p1, p2, a1, a2), [len(rt.feat_ev) for rt in rts], T)


def _slice_calls(outs, ev_lens, T):
    """The outputs of one call over concatenated reads -> one (p1, p2, a1, a2) per read."""
    p1, p2, a1, a2 = outs
    calls, e0 = [], 0
    for N in ev_lens:
        sl = slice(e0, e0 + max(int(N) - T, 0))    # window i of the read == window e0+i of the call
        calls.append((p1[sl], p2[sl], a1[sl], a2[sl]))
        e0 += int(N)
    return calls


def _predict_each(reviser, rts):
    """Read by read, after a call over all of them failed: each read's calls, or its exception."""
    calls = []
    for rt in rts:
        try:
            calls.append(predict_one(reviser, rt))
        except Exception as e:
            calls.append(e)
    return calls


def revise_one(reviser, rt, want_qual: bool = True):
    """One read through the engine -> (revised sequence, per-base quality string)."""
    return _finish_read(reviser.T, rt, *predict_one(reviser, rt), want_qual=want_qual)


def revise_many(reviser, rts, want_qual: bool = True):
    return [_finish_read(reviser.T, rt, *c, want_qual=want_qual) for rt, c in zip(rts, predict_many(reviser, rts))]


def _load_one(job, native: bool = True):
    """Worker side of the host stage: fast5 -> per-event device inputs (picklable).  The file goes through the native
    reader (libnanorev_host.so: nrvh_load_fast5, one C call with the GIL released) when that is built and knows the
    file's HDF5 subset; anything else - and every failure - through the Python host stage, which is the definition of
    the numbers and words the errors."""
    path, fn, group, subgroup = job[:4]
    t0 = time.perf_counter()
    if native:
        rc, o = hostlib.load_fast5(path, group, subgroup, want_fastq=(job[4] if len(job) > 4 else True))
        if rc == hostlib.OK:
            rt = hs.RawReadTensors(o["raw"], o["starts"], o["feat"], o["bases"], o["shift"], o["scale"])
            return fn, rt, o["fastq"], None, time.perf_counter() - t0
    try:
        rd, fq = parse_read(path, group, subgroup)
    except Exception as e:                           # broken file: nothing to fall back to
        return fn, None, None, repr(e), time.perf_counter() - t0
    try:
        # int16 samples + starts + features (46 B/base through the pipe and over PCIe); the signal
        # windows are cut on the device.  Non-int16 signals (never seen in fast5) take the host path.
        rt = hs.read_tensors_raw(rd) if np.asarray(rd.signal).dtype == np.int16 else hs.read_tensors(rd)
        return fn, rt, fq, None, time.perf_counter() - t0
    except Exception as e:                           # host stage failed: originals can still be written
        return fn, hs.ReadTensors(None, None, rd.bases, 0.0, 0.0), fq, repr(e), time.perf_counter() - t0


class _LightRead:
    """What the finisher needs of a read whose arrays travel inside a bundle: the original bases."""
    __slots__ = ("bases", "n_ev")

    def __init__(self, bases, n_ev):
        self.bases, self.n_ev = bases, n_ev


def _load_bundle(jobs, device_stats: bool = False):
    """Worker-process side of the host stage for SEVERAL files: every read through `_load_one`, and the raw reads
    among them concatenated here into the arrays of ONE device call (samples, event starts, event features, one row
    of (raw_len, ev_len, shift, scale) per read), so that the main process neither unpickles thousands of small
    arrays nor concatenates them: a bundle is four big arrays.  Returns (entries, bundle): entries are
    `_load_one`'s tuples, with the tensors of bundled reads replaced by a `_LightRead`; bundle is None when no read
    qualified.  device_stats (--device_stats): the native loader leaves the read statistics to the device; the bundle then
    carries `last_dur` and `device_stats` per read, and shift / scale / feature columns 1 - 2 of the flagged reads are zeros."""
    t0 = time.perf_counter()
    # (device_stats is passed only when set: a stand-in for hostlib.load_bundle without that keyword keeps working)
    nb = hostlib.load_bundle([j[0] for j in jobs], jobs[0][2], jobs[0][3], want_fastq=(jobs[0][4] if len(jobs[0]) > 4 else True),
                             **({"device_stats": True} if device_stats else {})) \
        if jobs and all(j[2:] == jobs[0][2:] for j in jobs) else None
    n_ok = int((nb["status"] == hostlib.OK).sum()) if nb is not None else 0
    if device_stats and not 0 < n_ok == len(jobs):
        return _load_bundle(jobs)                     # no library, or a file for the Python reader among them: host-fed as ever
    if n_ok > 0:
        # ONE native call for the whole task: the reads it took are already concatenated; the others (a layout the native
        # reader does not know, a broken file) go through the Python host stage one by one
        dt = (time.perf_counter() - t0) / len(jobs)
        entries, good, eo = [], [], 0
        for i, j in enumerate(jobs):
            if nb["status"][i] == hostlib.OK:
                el = int(nb["meta"][i, 1])
                entries.append((j[1], _LightRead(nb["bases"][eo:eo + el], el), nb["fastq"][i], None, dt))
                good.append(i)
                eo += el
            else:
                entries.append(tuple(_load_one(j, native=False)))
        if any(isinstance(e[1], hs.RawReadTensors) for e in entries):
            # a Python-path read would have to be spliced into the middle of the concatenation: rare enough to give up
            # the bundle's shortcut for this task (each read then travels on its own, as without a pool)
            out, eo, ro = [], 0, 0
            for i, e in enumerate(entries):
                if i in good:
                    rl, el, sh, sc = nb["meta"][i]
                    rl, el = int(rl), int(el)
                    rt = hs.RawReadTensors(nb["raw"][ro:ro + rl], nb["starts"][eo:eo + el], nb["feat"][eo:eo + el],
                                           nb["bases"][eo:eo + el], float(sh), float(sc))
                    out.append((e[0], rt, e[2], None, e[4]))
                    ro += rl
                    eo += el
                else:
                    out.append(e)
            return _bundle_of(out)
        bundle = {"idx": good, "raw": nb["raw"], "starts": nb["starts"], "feat": nb["feat"],
                  "meta": np.ascontiguousarray(nb["meta"][good]), "bases": nb["bases"]}
        if device_stats:                              # (every read is in the bundle)
            bundle["last_dur"], bundle["device_stats"] = np.ascontiguousarray(nb["last_dur"]), np.ascontiguousarray(nb["device_stats"])
        return entries, bundle
    return _bundle_of([_load_one(j) for j in jobs])


def _load_bundle_labelled(jobs, device_stats: bool, labels_dir: str):
    """`_load_bundle` for a --score run: the label bytes of the bundle's reads are read HERE, in the parser pool beside the
    parse, and ride with the bundle: bundle["labels"] = (labels uint8[N], flags) as `ScorePart.block` gives them."""
    entries, bundle = _load_bundle(jobs, True) if device_stats else _load_bundle(jobs)
    if bundle is not None and _bundle_has_bases(bundle):
        bundle["labels"] = ScorePart(None, labels_dir).block([entries[i][0] for i in bundle["idx"]], bundle["bases"], bundle["meta"][:, 1])
    return entries, bundle


def _bundle_of(loaded):
    """`_load_one` tuples -> (entries, bundle): the raw reads among them concatenated into the arrays of one device call."""
    entries, good = [], []
    for fn, rt, fq, err, dt in loaded:
        if err is None and isinstance(rt, hs.RawReadTensors):
            good.append(len(entries))
        entries.append([fn, rt, fq, err, dt])
    if not good:
        return [tuple(e) for e in entries], None
    rts = [entries[i][1] for i in good]
    bundle = {
        "idx": good,
        "raw": np.concatenate([np.ascontiguousarray(r.raw, dtype=np.int16) for r in rts]),
        "starts": np.concatenate([np.ascontiguousarray(r.starts, dtype=np.int32) for r in rts]),
        "feat": np.concatenate([np.asarray(r.feat_ev, np.float32).reshape(-1, 6) for r in rts]),
        "meta": np.array([[len(r.raw), len(r.starts), r.shift, r.scale] for r in rts], np.float64),
    }
    for i, r in zip(good, rts):
        entries[i][1] = _LightRead(r.bases, len(r.starts))
    return [tuple(e) for e in entries], bundle


def _bundle_host_stats(bundle):
    """A --device_stats bundle with the statistics of its flagged reads computed HERE (hoststage is the definition): what the
    plain loader would have delivered.  For the paths that feed a read from the host after all - an engine without the new
    calls, the per-read retries after a failed batched call."""
    if bundle is None or "device_stats" not in bundle:
        return bundle
    feat, meta = np.array(bundle["feat"], np.float32), np.array(bundle["meta"], np.float64)
    ro = eo = 0
    for r, (rl, el) in enumerate(meta[:, :2].astype(np.int64)):
        if bundle["device_stats"][r]:
            meta[r, 2], meta[r, 3], feat[eo:eo + el, 1], feat[eo:eo + el, 2] = hs.stats_columns(
                bundle["raw"][ro:ro + rl], bundle["starts"][eo:eo + el], int(bundle["last_dur"][r]))
        ro += rl
        eo += el
    out = {k: v for k, v in bundle.items() if k not in ("device_stats", "last_dur")}
    out["feat"], out["meta"] = feat, meta
    return out


def _bundle_reads(bundle):
    """The reads of a bundle as RawReadTensors VIEWS (per-read retries after a failed batched call)."""
    bundle = _bundle_host_stats(bundle)
    out, ro, eo = [], 0, 0
    for rl, el, sh, sc in bundle["meta"]:
        rl, el = int(rl), int(el)
        out.append(hs.RawReadTensors(bundle["raw"][ro:ro + rl], bundle["starts"][eo:eo + el],
                                     bundle["feat"][eo:eo + el], None, float(sh), float(sc)))
        ro += rl
        eo += el
    return out


class _OutSpec:
    """The part of the parsed arguments `write_read` needs (picklable, for the worker processes)."""

    def __init__(self, args):
        self.output_dir, self.output_format = args.output_dir, args.output_format


def _finish_in_worker(spec, T, fn, bases, a1, a2, qc):
    """Worker-process side of the merge: calls of one read + its original bases -> revised read -> its output file
    (the 0.5 ms of NumPy, string building and file IO per read that the main process' finisher thread used to spend
    under the GIL).  qc: per-window Phred characters (FASTQ) or None (FASTA).  Returns (bases written, error)."""
    try:
        seq, qual = _merge_read(T, bases, a1, a2, qc)
        write_read(spec, fn, seq, qual)
        return len(seq), None
    except Exception as e:
        return 0, repr(e)


def _finish_native(spec, T, fn, bases, a1, a2, qc):
    """`_finish_in_worker` through libnanorev_host.so (nrvh_finish_read: merge, record, temporary + rename in one C call
    with the GIL released) - for the THREAD pool of process_files.  Same return value."""
    try:
        os.makedirs(spec.output_dir, exist_ok=True)
        nb = hostlib.finish_read(bases, a1, a2, T, qc, fn.split("/")[-1].replace(" ", "|||"),
                                 out_name(spec.output_dir, fn, spec.output_format), spec.output_format == "fastq")
        if nb is None:
            return _finish_in_worker(spec, T, fn, bases, a1, a2, qc)
        return nb, None
    except Exception as e:
        return 0, repr(e)


def _native_task(spec, fns, call):
    """One native finisher call for the reads `fns` (GIL released): call(names, destinations, fastq) -> [(bases written, error)]."""
    try:
        os.makedirs(spec.output_dir, exist_ok=True)
        r = call([fn.split("/")[-1].replace(" ", "|||") for fn in fns],
                 [out_name(spec.output_dir, fn, spec.output_format) for fn in fns], spec.output_format == "fastq")
        if r is None:
            raise RuntimeError("libnanorev_host.so went away")
        return [(int(n), None if c == hostlib.OK else f"native finisher: error {int(c)}") for n, c in zip(*r)]
    except Exception as e:
        return [(0, repr(e))] * len(fns)


def _finish_bundle_native(spec, T, fns, bases, ev_len, a1, a2, qc):
    """All reads of one device call through nrvh_finish_bundle: [(bases written, error)]."""
    return _native_task(spec, fns, lambda names, dsts, fq: hostlib.finish_bundle(bases, ev_len, a1, a2, T, qc, names, dsts, fq))


def _write_records_native(spec, fns, seq, qual, off):
    """All reads of one --device_merge call through nrvh_write_records: [(bases written, error)]."""
    return _native_task(spec, fns, lambda names, dsts, fq: hostlib.write_records(seq, qual, off, names, dsts, fq))


def _fai_line(name: bytes, length: int, start: int, fastq: bool) -> bytes:
    """The samtools faidx line of the record that starts at byte `start` of its file: name, length, offset of the first base,
    linebases (= length: no wrapping), linewidth (= length + 1) and, FASTQ, the offset of the first quality."""
    o = start + len(name) + 2
    cols = [length, o, length, length + 1] + ([o + length + 3] if fastq else [])
    return name + b"\t" + "\t".join(str(int(c)) for c in cols).encode() + b"\n"


def _fai_record(cols, fastq: bool):
    """(start, bytes) of the record an index line describes."""
    name, length, o = cols[0], int(cols[1]), int(cols[2])
    return o - len(name) - 2, len(name) + (2 * length + 6 if fastq else length + 3)


class CombinedPart:
    """One process' share of --combined FILE: the records go to `path`, one faidx line per record (offsets inside the part) to
    `path`'s index part - the blob first, then the index lines, both flushed per call, so a record counts as written when its
    index line is complete.  `merge_combined` puts the parts together."""

    def __init__(self, path: Optional[str], fastq: bool = False):
        self.path, self.fastq, self._lock, self._fp, self._ix, self._size = path, fastq, threading.Lock(), None, None, 0
        self.index_path = combined_index_part(path) if path else None

    def __bool__(self):
        return self.path is not None

    def add_blob(self, fns, blob, rec_off, off):
        """The records of the reads `fns` as one blob (hoststage.pack_records' layout; off: the reads' offsets into seq)."""
        names = [hs.record_name(fn) for fn in fns]
        data = np.ascontiguousarray(blob, dtype=np.uint8)[:int(rec_off[-1])].tobytes()
        with self._lock:
            if self._fp is None:
                d = os.path.dirname(self.path)
                if d:
                    os.makedirs(d, exist_ok=True)
                self._fp, self._ix = open(self.path, "wb"), open(self.index_path, "wb")
            self._fp.write(data)
            self._fp.flush()
            self._ix.write(b"".join(_fai_line(nm, int(off[r + 1]) - int(off[r]), self._size + int(rec_off[r]), self.fastq)
                                    for r, nm in enumerate(names)))
            self._ix.flush()
            self._size += len(data)

    def add(self, fns, seq, qual, off):
        """Merged reads (hoststage.emit_calls' form) through the definition of the records."""
        seq = np.asarray(seq, np.uint8).reshape(-1)
        if self.fastq and qual is None:               # no window at all: every base keeps quality '#'
            qual = np.full(seq.size, ord("#"), np.uint8)
        blob, rec_off = hs.pack_records([hs.record_name(fn) for fn in fns], seq, qual if self.fastq else None, off)
        self.add_blob(fns, blob, rec_off, off)

    def add_read(self, fn: str, seq: str, qual: Optional[str]):
        s = np.frombuffer(seq.encode("ascii"), np.uint8)
        q = np.frombuffer(qual.encode("ascii"), np.uint8) if (self.fastq and qual is not None) else None
        self.add([fn], s, q, np.array([0, s.size], np.int64))

    def close(self):
        with self._lock:
            for fp in (self._fp, self._ix):
                if fp is not None:
                    fp.close()
            self._fp = self._ix = None


def combined_part_path(combined: str, rank) -> str:
    return f"{combined}.part{rank}"


def combined_index_part(part: str) -> str:
    """FILE.part<rank> -> FILE.fai.part<rank>."""
    head, _, rank = part.rpartition(".part")
    return f"{head}.fai.part{rank}"


def clear_combined_parts(combined: str):
    import glob
    for f in glob.glob(glob.escape(combined) + ".part*") + glob.glob(glob.escape(combined) + ".fai.part*"):
        try:
            os.remove(f)
        except OSError:
            pass


def merge_combined(combined: str, fastq: bool):
    """Parent side of --combined: the parts in ascending rank order, the parent's own last, become FILE and FILE.fai with the
    offsets shifted.  A part's records are those of its complete index lines that lie inside the part (bytes beyond the last of
    them - a worker died mid-write - are dropped); of a read with several records the LAST one stays (a lost worker's read the
    parent wrote again).  One part with nothing to drop is renamed, not copied.  Both files appear by rename; the parts are removed."""
    import glob

    def rank_of(f):
        r = f.rsplit(".part", 1)[1]
        return (1, 0) if r == "parent" else (0, int(r) if r.isdigit() else 1 << 30)
    parts = sorted((f for f in glob.glob(glob.escape(combined) + ".part*")), key=rank_of)
    ncol = 6 if fastq else 5
    recs, last = [], {}                               # (part, name, length, start, bytes); name -> index of its last record
    clean = True
    for k, f in enumerate(parts):
        try:
            size = os.path.getsize(f)
            with open(combined_index_part(f), "rb") as fp:
                lines = fp.read().split(b"\n")
        except OSError:
            clean = False
            continue
        end = 0
        if lines[-1] != b"":                          # a line cut short is not a line
            clean = False
        for ln in lines[:-1]:
            c = ln.split(b"\t")
            try:
                start, nbytes = _fai_record(c, fastq) if len(c) == ncol else (-1, 0)
            except ValueError:
                start = -1
            if start != end or start + nbytes > size:  # records lie back to back: anything else ends the part
                clean = False
                break
            if c[0] in last:
                clean = False
            last[c[0]] = len(recs)
            recs.append((k, c[0], int(c[1]), start, nbytes))
            end = start + nbytes
        if end != size:
            clean = False
    d = os.path.dirname(combined)
    if d:
        os.makedirs(d, exist_ok=True)
    if clean and len(parts) == 1:
        os.replace(combined_index_part(parts[0]), combined + ".fai")
        os.replace(parts[0], combined)
        return
    tmp, tmp_ix = f"{combined}.tmp{os.getpid()}", f"{combined}.fai.tmp{os.getpid()}"
    with open(tmp, "wb") as out, open(tmp_ix, "wb") as ix:
        pos, src, src_k = 0, None, None
        for i, (k, name, length, start, nbytes) in enumerate(recs):
            if last[name] != i:
                continue
            if src_k != k:
                if src is not None:
                    src.close()
                src, src_k = open(parts[k], "rb"), k
            src.seek(start)
            out.write(src.read(nbytes))
            ix.write(_fai_line(name, length, pos, fastq))
            pos += nbytes
        if src is not None:
            src.close()
    os.replace(tmp, combined)
    os.replace(tmp_ix, combined + ".fai")
    for f in parts:
        for g in (f, combined_index_part(f)):
            try:
                os.remove(g)
            except OSError:
                pass


def _deliver_trimmed(spec, sink, fns, payload, native, bounds, min_len):
    """`deliver` for reads that are cut to `bounds` (int64[len(fns)][2], `hoststage.trim_bounds`) first: every payload becomes
    the kept reads' own characters (a records blob is cut already and only loses the dropped reads' index lines) and goes
    through `deliver`.  A dropped read (hi - lo < min_len) is written nowhere and answers (0, None)."""
    kind, rest = payload[0], payload[1:]
    t = np.asarray(bounds, np.int64).reshape(-1, 2)
    keep = hs.trim_kept(t, min_len)
    if len(t) != len(fns):
        raise ValueError("deliver: the trim does not match the reads")
    if kind == "text":
        seq, qual = rest
        lo, hi = int(t[0, 0]), int(t[0, 1])
        return deliver(spec, sink, fns, ("text", seq[lo:hi], qual[lo:hi] if qual is not None else None), native) if keep[0] else [(0, None)]
    try:
        if kind == "calls":
            seq, qual = _merge_read(rest[0], *rest[1:])
            lo, hi = int(t[0, 0]), int(t[0, 1])
            return deliver(spec, sink, fns, ("text", seq[lo:hi], qual[lo:hi] if qual is not None else None), native) if keep[0] else [(0, None)]
        lens = (t[:, 1] - t[:, 0])[keep]
        fns_k = [fn for fn, k in zip(fns, keep) if k]
        off_k = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        if kind == "records":
            blob, rec_off, off = rest
            if len(rec_off) != len(fns) + 1:
                raise ValueError("deliver: the records do not match the reads")
            if sink is None or not sink:
                raise ValueError("deliver: records needs a sink")
            rec_off = np.asarray(rec_off, np.int64)
            sink.add_blob(fns_k, blob, np.concatenate([rec_off[:-1][keep], rec_off[-1:]]), off_k)      # a dropped read has no bytes
            res_k = [(int(n), None) for n in lens]
        else:
            if kind == "bundle":
                T, bases, ev_len, a1, a2, qc = rest
                seq, qual, off = hs.emit_calls(hostlib.bases_u8(bases), ev_len, a1, a2, qc, T)
            elif kind == "merged":
                seq, qual, off = rest
            else:
                raise ValueError(f"deliver: unknown payload {kind}")
            off = np.asarray(off, np.int64)
            at = np.repeat((off[:-1] + t[:, 0])[keep] - off_k[:-1], lens) + np.arange(int(off_k[-1]), dtype=np.int64)
            seq_k = np.asarray(seq, np.uint8).reshape(-1)[at]
            qual_k = None if qual is None else np.asarray(qual, np.uint8).reshape(-1)[at]
            if not fns_k:
                res_k = []
            elif (sink is None or not sink) and not (native and hostlib.has_write_records()):
                res_k = []
                for r, fn in enumerate(fns_k):
                    a, b = int(off_k[r]), int(off_k[r + 1])
                    res_k += deliver(spec, None, [fn], ("text", seq_k[a:b].tobytes().decode("ascii"),
                                                        None if qual_k is None else qual_k[a:b].tobytes().decode("ascii")), native)
            else:
                res_k = deliver(spec, sink, fns_k, ("merged", seq_k, qual_k, off_k), native)
        it = iter(res_k)
        return [next(it) if k else (0, None) for k in keep]
    except Exception as e:
        return [(0, repr(e))] * len(fns)


def deliver(spec, sink, fns, payload, native: bool = True, trim=None):
    """THE decision about where finished reads go, for every path that has some: into the --combined sink (`CombinedPart`, through
    hoststage.pack_records - or as they are, when the device laid the records out) or, without one, into one file per read by the
    writer the path has always used.  payload is what the path holds:
      ("text", seq, qual)                          one read as strings (`write_read`)
      ("calls", T, bases, a1, a2, qc)              one read's calls (`_finish_native` / `_finish_in_worker`)
      ("bundle", T, bases, ev_len, a1, a2, qc)     the calls of all reads of a device call (`_finish_bundle_native`)
      ("merged", seq, qual, off)                   a --device_merge call's revised reads (`_write_records_native`)
      ("records", blob, rec_off, off)              a `with_device_records` call's blob (sink only)
    trim (--trim_q): (bounds int64[len(fns)][2], min_len), or None.  THE place where the bounds are applied, for every path: a
    kept read is written as its characters [lo, hi), a dropped one not at all (0 bases, no error); the blob of a
    `with_device_trim` call is cut already.  A read written unrevised comes without a trim and is written whole.
    Returns [(bases written, error)] per read; "text" raises instead, as `write_read` does."""
    if trim is not None:
        return _deliver_trimmed(spec, sink, fns, payload, native, *trim)
    kind, rest = payload[0], payload[1:]
    if sink is None or not sink:
        if kind == "text":
            write_read(spec, fns[0], *rest)
            return [(len(rest[0]), None)]
        if kind == "calls":
            return [(_finish_native if native else _finish_in_worker)(spec, rest[0], fns[0], *rest[1:])]
        if kind == "bundle":
            return _finish_bundle_native(spec, rest[0], fns, *rest[1:])
        if kind == "merged":
            return _write_records_native(spec, fns, *rest)
        raise ValueError(f"deliver: {kind} needs a sink")
    if kind == "text":
        sink.add_read(fns[0], *rest)
        return [(len(rest[0]), None)]
    try:
        if kind == "calls":
            seq, qual = _merge_read(rest[0], *rest[1:])
            sink.add_read(fns[0], seq, qual)
            return [(len(seq), None)]
        if kind == "bundle":
            T, bases, ev_len, a1, a2, qc = rest
            seq, qual, off = hs.emit_calls(hostlib.bases_u8(bases), ev_len, a1, a2, qc, T)
            sink.add(fns, seq, qual, off)
        elif kind == "merged":
            seq, qual, off = rest
            sink.add(fns, seq, qual, off)
        else:
            blob, rec_off, off = rest
            if len(rec_off) != len(fns) + 1 or len(off) != len(fns) + 1:
                raise ValueError("deliver: the records do not match the reads")
            sink.add_blob(fns, blob, rec_off, off)
        return [(int(off[r + 1]) - int(off[r]), None) for r in range(len(fns))]
    except Exception as e:
        return [(0, repr(e))] * len(fns)


REPORT_HEADER = "name\tstatus\t" + "\t".join(hs.REPORT_NAMES)


def report_rows(T, bases, ev_len, p1, p2, a1, a2, want_qual, tie_eps):
    """--report on the host: `hoststage.revision_report` on calls the host holds, with the quality characters the writers use
    (FASTQ: `phred_chars`; FASTA: none).  uint64[len(ev_len)][24]."""
    qc = None
    if want_qual:
        qc = phred_chars(p1, p2, a1, a2) if len(a1) else np.zeros(0, np.uint8)
    return hs.revision_report(hostlib.bases_u8(bases), ev_len, a1, a2, p1, p2, qc, T, tie_eps)


def unrevised_row(n_written: int) -> np.ndarray:
    """The report row of a read written unrevised: bases_in = bases_out = edge = what was written, zeros elsewhere."""
    row = np.zeros(hs.REPORT_COLS, np.uint64)
    row[0] = row[2] = row[3] = max(int(n_written), 0)
    return row


def _second_line(path: str) -> bytes:
    try:
        with open(path, "rb") as fp:
            fp.readline()
            return fp.readline().rstrip(b"\r\n")
    except OSError:
        return b""


def written_sequence(path: str, fastq: bool) -> bytes:
    """The sequence of the one record in a per-read output file; empty when there is none.  It is the file's second line; in a
    FASTQ file that line ends with the '+' `hoststage.fastq_record` puts there without a newline in front, which is not a base."""
    line = _second_line(path)
    return line[:-1] if fastq and line.endswith(b"+") else line


def written_length(path: str) -> int:
    """Length of the second line of an output file (--report's bases of a --resume skip); 0 when there is none."""
    return len(_second_line(path))


SUMMARY_HEADER = "name\tstatus\tbases\tmean_q\tmedian_q\tq10\tq20\tq30\tgc\tA\tC\tG\tT\tother"
SUMMARY_COLS = 47                          # the columns of a profile row a part line carries: 48 less the reserved one


def profile_rows(T, bases, ev_len, p1, p2, a1, a2):
    """--summary on the host: `hoststage.read_profile` on calls the host holds.  The profile is that of the FASTQ form of the
    calls whether the run writes a quality or not: `phred_chars`, then `emit_calls`, then `read_profile`.  uint64[len(ev_len)][48]."""
    qc = phred_chars(p1, p2, a1, a2) if len(a1) else np.zeros(0, np.uint8)
    return hs.read_profile(*hs.emit_calls(hostlib.bases_u8(bases), ev_len, a1, a2, qc, T))


def trim_rule(args):
    """(Q, W, min_len) of --trim_q / --trim_window / --min_len, or None without --trim_q."""
    q = getattr(args, "trim_q", None)
    return None if q is None else (int(q), int(getattr(args, "trim_window", 10)), int(getattr(args, "min_len", 1)))


def _trim_rows_len(T, bases, ev_len, p1, p2, a1, a2, Q, W):
    """`trim_rows` and the lengths of the untrimmed revised reads: (int64[R][2], int64[R])."""
    qc = phred_chars(p1, p2, a1, a2) if len(a1) else np.zeros(0, np.uint8)
    _, qual, off = hs.emit_calls(hostlib.bases_u8(bases), ev_len, a1, a2, qc, T)
    return hs.trim_bounds(qual, off, Q, W), np.diff(off)


def trim_rows(T, bases, ev_len, p1, p2, a1, a2, Q, W):
    """--trim_q on the host: `hoststage.trim_bounds` on calls the host holds.  The qualities are those of the FASTQ form of the
    calls whether the run writes a quality or not: `phred_chars`, then `emit_calls`, then `trim_bounds`.  int64[len(ev_len)][2]."""
    return _trim_rows_len(T, bases, ev_len, p1, p2, a1, a2, Q, W)[0]


TRIM_HEADER = "name\tstatus\tbases\tlo\thi\tkept"


def trim_log_row(n_bases, bounds, min_len) -> List[int]:
    """The integers of a --trim_log line: bases of the untrimmed read, lo, hi, kept."""
    lo, hi = int(bounds[0]), int(bounds[1])
    return [int(n_bases), lo, hi, int(hi - lo >= int(min_len))]


def unrevised_trim(n_written: int) -> List[int]:
    """The --trim_log integers of a read written unrevised: whole, and kept."""
    n = max(int(n_written), 0)
    return [n, 0, n, 1]


ACCURACY_HEADER = "name\tstatus\ttruth_len\tlen_in\tdist_in\tlen_out\tdist_out\tid_in\tid_out"
ACCURACY_PART_COLS = 6                     # a part line's integers: truth_len, len_in, dist_in, len_out, dist_out, flag
ACC_WITH_TRUTH, ACC_NO_TRUTH, ACC_TOO_LONG = 0, 1, 2            # the flag


def _truth_key(name: str) -> str:
    return name[:-len(".fast5")] if name.endswith(".fast5") else name


def load_truth(path: str) -> dict:
    """--truth: {name: sequence bytes} of a FASTA file.  Records may be wrapped; sequences are upper-cased; the name is the first
    word of the header, kept without a trailing .fast5.  A name that occurs twice - with or without .fast5 - raises ValueError."""
    truths, name, parts = {}, None, []
    with open(path, "rb") as fp:
        for ln in fp:
            ln = ln.strip()
            if ln.startswith(b">"):
                if name is not None:
                    truths[name] = b"".join(parts).upper()
                words = ln[1:].split()
                name, parts = _truth_key(words[0].decode() if words else ""), []
                if name in truths:
                    raise ValueError(f"--truth: the name {name} occurs twice in {path}")
            elif ln and name is not None:
                parts.append(ln)
    if name is not None:
        truths[name] = b"".join(parts).upper()
    return truths


def truth_of(truths: dict, fast5_fn: str):
    """The truth of a fast5 file, whether its record names it with or without .fast5; None when there is none."""
    return truths.get(_truth_key(fast5_fn))


def accuracy_rows(T, bases, ev_len, a1, a2, truth, truth_off):
    """--accuracy on the host: `hoststage.read_accuracy` on calls the host holds - `emit_calls` for the untrimmed revised reads,
    then the definition.  (uint64[len(ev_len)][4], the lengths of the revised reads)."""
    b = hostlib.bases_u8(bases)
    seq, _, off = hs.emit_calls(b, ev_len, a1, a2, None, T)
    return hs.read_accuracy(b, ev_len, seq, off, truth, truth_off), np.diff(off)


def identity_field(dist: int, denom: int) -> str:
    """1 - dist / denom with six decimals, denom = max(len, truth_len) of a read or the sum of those over reads: THE identity
    of the --accuracy file, formed from the integers on every route."""
    x = 1.0 - int(dist) / int(denom) if int(denom) > 0 else 1.0
    return f"{x:.6f}"


def accuracy_fields(v) -> List[str]:
    """The fields of an --accuracy line behind name and status from a part line's integers."""
    m, len_in, d_in, len_out, d_out, flag = (int(x) for x in v[:ACCURACY_PART_COLS])
    if flag != ACC_WITH_TRUTH:
        return ["0"] + ["."] * 6
    return [str(m), str(len_in), str(d_in), str(len_out), str(d_out), identity_field(d_in, max(len_in, m)), identity_field(d_out, max(len_out, m))]


ERRCLASS_HEADER = "name\tstatus\ttruth_len\tlen_in\tmatch_in\tsub_in\tins_in\tdel_in\tlen_out\tmatch_out\tsub_out\tins_out\tdel_out"
ERRCLASS_PART_COLS = 8                     # a part line's integers: truth_len, len_in, dist_in, match_in, len_out, dist_out, match_out, flag


def error_class_rows(T, bases, ev_len, a1, a2, truth, truth_off):
    """--error_classes on the host: `hoststage.read_error_classes` on calls the host holds, as `accuracy_rows`.
    (uint64[len(ev_len)][6], the lengths of the revised reads)."""
    b = hostlib.bases_u8(bases)
    seq, _, off = hs.emit_calls(b, ev_len, a1, a2, None, T)
    return hs.read_error_classes(b, ev_len, seq, off, truth, truth_off), np.diff(off)


def error_class_fields(v, rates: bool = False) -> List[str]:
    """The fields of an --error_classes line behind name and status from a part line's integers - or, rates=True, of #total from
    their sums: THE place where the four integers m, n, d, M of a pair become its counts, substitutions S = m + n - 2M - d,
    insertions I = d - (m - M), deletions D = d - (n - M) (all linear: the counts of the sums are the sums of the counts), and
    where a rate count / truth_len gets its six decimals, on every route."""
    m, len_in, d_in, M_in, len_out, d_out, M_out, flag = (int(x) for x in v[:ERRCLASS_PART_COLS])
    if flag != ACC_WITH_TRUTH:
        return ["0"] + ["."] * 10
    out, tail = [str(m)], []
    for n, d, M in ((len_in, d_in, M_in), (len_out, d_out, M_out)):
        counts = (m + n - 2 * M - d, d - (m - M), d - (n - M))
        out += [str(n), str(M)] + [str(c) for c in counts]
        tail += [f"{(c / m if m > 0 else 0.0):.6f}" for c in counts]
    return out + (tail if rates else [])


INFIX_HEADER = ("name\tstatus\ttruth_len\tstrand\tlen_in\tdist_in\tmatch_in\tstart_in\tend_in\tid_in"
                "\tlen_out\tdist_out\tmatch_out\tstart_out\tend_out\tid_out")
INFIX_PART_COLS = 21                       # a part line's integers: truth_len, strands, len_in, len_out, the block's columns 2 .. 17, flag


def infix_rows(T, bases, ev_len, a1, a2, truth, truth_off, strands=2):
    """--infix on the host: `hoststage.read_infix` on calls the host holds, as `accuracy_rows`.
    (uint64[len(ev_len)][18], the lengths of the revised reads)."""
    b = hostlib.bases_u8(bases)
    seq, _, off = hs.emit_calls(b, ev_len, a1, a2, None, T)
    return hs.read_infix(b, ev_len, seq, off, truth, truth_off, strands), np.diff(off)


def infix_identity(match: int, dist: int) -> str:
    """match / (match + dist) with six decimals - matched columns over alignment columns -, `.` when there is no column: THE
    identity of the --infix file, formed from the integers on every route."""
    return f"{int(match) / (int(match) + int(dist)):.6f}" if int(match) + int(dist) > 0 else "."


def infix_fields(v) -> List[str]:
    """The fields of an --infix line behind name and status from a part line's integers: THE place where the strand is picked
    (`hoststage.pick_strand`: - exactly when the ORIGINAL read fits the reverse strand strictly better; both forms are then
    reported on it) and where start / end of the reverse strand become 0-based half-open positions on the region AS GIVEN
    (m - end, m - start)."""
    v = [int(x) for x in v[:INFIX_PART_COLS]]
    m, strands, len_in, len_out, flag = v[0], v[1], v[2], v[3], v[-1]
    if flag != ACC_WITH_TRUTH:
        return ["0"] + ["."] * 13
    strand = hs.pick_strand([m, strands] + v[4:20])
    out = [str(m), strand]
    for n, g in ((len_in, 4), (len_out, 12)):
        d, M, st, en = v[g + 4:g + 8] if strand == "-" else v[g:g + 4]
        if strand == "-":
            st, en = m - en, m - st
        out += [str(n), str(d), str(M), str(st), str(en), infix_identity(M, d)]
    return out


def infix_sums(v) -> List[int]:
    """What #total adds up of a read with a truth: truth_len, then len, dist, match of both forms on the strand reported."""
    f = infix_fields(v)
    return [int(f[k]) for k in (0, 2, 3, 4, 8, 9, 10)]


def unrevised_profile(seq) -> np.ndarray:
    """The profile row of a read written unrevised: the base counts of the sequence that was written (str or bytes), no histogram."""
    row = np.zeros(hs.PROFILE_COLS, np.uint64)
    text = seq.encode("ascii", "replace") if isinstance(seq, str) else bytes(seq)
    for i, c in enumerate(b"ACGT"):
        row[42 + i] = text.count(bytes([c]))
    row[46] = len(text) - int(row[42:46].sum())
    return row


def summary_fields(row) -> List[str]:
    """The fields of a summary line behind name and status, from ONE integer profile row (or a sum of rows): bases, mean_q,
    median_q, q10, q20, q30, gc, A, C, G, T, other.  Every route formats through this function, so equal rows give equal bytes."""
    v = [int(x) for x in np.asarray(row).reshape(-1)[:SUMMARY_COLS]]
    h, acgt = v[:42], v[42:47]
    bases, L = sum(acgt), sum(h)
    mean_q = format(-10 * math.log10(math.fsum(h[k] * 10.0 ** (-k / 10.0) for k in range(42)) / L), ".4f") if L else "0.0000"
    median_q, cum = 0, 0
    if L:
        for k in range(42):
            cum += h[k]
            if 2 * cum >= L:
                median_q = k
                break
    gc = format((acgt[1] + acgt[2]) / bases, ".4f") if bases else "0.0000"
    return [str(bases), mean_q, str(median_q)] + [str(sum(h[n:])) for n in (10, 20, 30)] + [gc] + [str(x) for x in acgt]


def n50(lengths) -> int:
    """The largest L such that the reads of at least L bases hold at least half of all bases; 0 when there are none."""
    ls = sorted((int(x) for x in lengths), reverse=True)
    total, cum = sum(ls), 0
    for x in ls:
        cum += x
        if 2 * cum >= total:
            return x
    return 0


def _summary_closing(lines):
    """The last line of the --summary file from its (status, integer row) pairs: revised reads, unrevised reads, N50 of the revised."""
    rev = [sum(v[42:47]) for st, v in lines if st == "revised"]
    return [f"#reads\t{len(rev)}\t{len(lines) - len(rev)}\t{n50(rev)}"]


class ReportPart:
    """One process' share of the --report file (or, with cols = SUMMARY_COLS, of the --summary file; with cols = 4, of the
    --trim_log file): a line per read, appended
    and flushed as the read's output becomes final (so a worker that dies leaves the lines of what it finished).  `merge_report`
    puts the parts together."""

    def __init__(self, path: Optional[str], cols: int = 23):
        self.path, self.cols, self._lock, self._fp = path, cols, threading.Lock(), None

    def __bool__(self):
        return self.path is not None

    def add(self, fn: str, revised: bool, row):
        if self.path is None:
            return
        line = fn + "\t" + ("revised" if revised else "unrevised") + "\t" + "\t".join(str(int(v)) for v in np.asarray(row)[:self.cols]) + "\n"
        with self._lock:
            if self._fp is None:
                self._fp = open(self.path, "a")
            self._fp.write(line)
            self._fp.flush()

    def close(self):
        with self._lock:
            if self._fp is not None:
                self._fp.close()
                self._fp = None


def report_part_path(report: str, rank) -> str:
    return f"{report}.part{rank}"


def clear_report_parts(report: str):
    import glob
    for f in glob.glob(glob.escape(report) + ".part*"):
        try:
            os.remove(f)
        except OSError:
            pass


# what `merge_report` writes from the parts' integer columns: (columns per line, header, the switch's name, the integers -> the
# fields of a line (None: the integers themselves), [(status, integers)] -> the lines behind #total (None: none))
REPORT_TABLE = (23, REPORT_HEADER, "--report", None, None)
SUMMARY_TABLE = (SUMMARY_COLS, SUMMARY_HEADER, "--summary", summary_fields, _summary_closing)
TRIM_TABLE = (4, TRIM_HEADER, "--trim_log", None, None)


def _part_rows(report: str, cols: int):
    """({name: fields of its last whole line}, the part files) of a report's parts, in the order they were written: the parent's
    own part comes last."""
    import glob
    rows = {}
    parts = sorted(glob.glob(glob.escape(report) + ".part*"), key=lambda f: (f.endswith(".partparent"), f))
    for f in parts:
        with open(f) as fp:
            for ln in fp:
                c = ln.rstrip("\n").split("\t")
                if ln.endswith("\n") and len(c) == 2 + cols:         # a line cut short by a dying worker is not a line
                    rows[c[0]] = c
    return rows, parts


def _replace_report(report: str, lines, parts):
    """The merged file appears by rename; the parts are removed."""
    d = os.path.dirname(report)
    if d:
        os.makedirs(d, exist_ok=True)
    tmp = f"{report}.tmp{os.getpid()}"
    with open(tmp, "w") as fp:
        fp.write("\n".join(lines) + "\n")
    os.replace(tmp, report)
    for f in parts:
        try:
            os.remove(f)
        except OSError:
            pass


def merge_report(report: str, names: Sequence[str], log: Callable[[str], None] = print, table=REPORT_TABLE):
    """Parent side of --report (and, with SUMMARY_TABLE, of --summary; with TRIM_TABLE, of --trim_log): the parts in the order they were written (a later line
    for the same read wins: the parent's own part comes last), one line per read of `names` sorted by file name, `#total` = the
    sums over the revised reads; the file appears by rename and the parts are removed."""
    cols, header, switch, fields, closing = table
    rows, parts = _part_rows(report, cols)
    total, seen = [0] * cols, []
    out = [header]
    for fn in sorted(names):
        c = rows.get(fn)
        if c is None:                                               # no process accounted for it: nothing was written
            log(f"[！！！Warning] {switch}: no record for {fn}")
            c = [fn, "unrevised"] + ["0"] * cols
        out.append("\t".join(c if fields is None else c[:2] + fields([int(v) for v in c[2:]])))
        if c[1] == "revised":
            total = [t + int(v) for t, v in zip(total, c[2:])]
        if closing is not None:
            seen.append((c[1], [int(v) for v in c[2:]]))
    out.append("#total\trevised\t" + "\t".join(str(t) for t in total) if fields is None else "\t".join(["#total", "revised"] + fields(total)))
    if closing is not None:
        out += closing(seen)
    _replace_report(report, out, parts)


class AccuracyPart(ReportPart):
    """One process' share of the --accuracy file, and what forms its lines: the truth set, --accuracy_max_len, the rows of the
    host routes (`host_rows`) and of a read written unrevised (`add_unrevised`)."""

    def __init__(self, path: Optional[str], truths: Optional[dict], max_len: int = 65536, log: Callable[[str], None] = print):
        super().__init__(path, ACCURACY_PART_COLS)
        self.truths, self.max_len, self.log, self.warned = truths or {}, int(max_len), log, False
        self.classes = None                           # the parent's --error_classes part rides along (`write_originals`, `finish_split_reads`)
        self.infix = None                             # ... and its --infix part (this part may then have no path: --infix without --accuracy)

    def block(self, fns, lens_in):
        """The truth set of a device call: (truth uint8[], truth_off int64[R + 1], flags).  A read without a record, or whose
        truth or original length exceeds --accuracy_max_len, has an empty truth."""
        parts, flags = [], []
        for fn, n in zip(fns, lens_in):
            t = truth_of(self.truths, fn)
            flag = ACC_NO_TRUTH if t is None or len(t) == 0 else (ACC_TOO_LONG if max(len(t), int(n)) > self.max_len else ACC_WITH_TRUTH)
            parts.append(t if flag == ACC_WITH_TRUTH else b"")
            flags.append(flag)
        toff = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
        return np.frombuffer(b"".join(parts), np.uint8), toff, flags

    @staticmethod
    def rows(acc, lens_in, lens_out, flags):
        """A part line's integers per read from an accuracy block (hoststage.read_accuracy's or the device's)."""
        return [[int(a[0]), int(n), int(a[1]), int(k), int(a[2]), f] if f == ACC_WITH_TRUTH else [0, int(n), 0, int(k), 0, f]
                for a, n, k, f in zip(np.asarray(acc).tolist(), lens_in, lens_out, flags)]

    def host_rows(self, T, fns, bases, ev_len, a1, a2):
        if not self.warned:
            self.warned = True
            self.log("[！！！Warning] --accuracy: the edit distances are computed by the host stage, about 0.1 s per read "
                     "(--device_merge computes them on the GPU)")
        truth, toff, flags = self.block(fns, ev_len)
        acc, lens_out = accuracy_rows(T, bases, ev_len, a1, a2, truth, toff)
        return self.rows(acc, ev_len, lens_out, flags)

    def add_unrevised(self, fn: str, text):
        """A read written unrevised (text: what was written, str or bytes): len_out = len_in, dist_out = dist_in."""
        if self.path is None:
            return
        text = text.encode("ascii", "replace") if isinstance(text, str) else bytes(text)
        truth, toff, (flag,) = self.block([fn], [len(text)])
        d = hs.edit_distance(truth, text) if flag == ACC_WITH_TRUTH else 0
        self.add(fn, False, [int(toff[1]), len(text), d, len(text), d, flag])


def merge_accuracy(path: str, names: Sequence[str], log: Callable[[str], None] = print):
    """Parent side of --accuracy: the parts as `merge_report` reads them, one line per read of `names` sorted by file name, then
    #total - the sums over the reads WITH a truth, revised or not, and the pooled identities 1 - sum(dist) / sum(max(len,
    truth_len)) - and #reads with_truth / no_truth / too_long; the file appears by rename and the parts are removed."""
    rows, parts = _part_rows(path, ACCURACY_PART_COLS)
    out, total, den, counts = [ACCURACY_HEADER], [0] * 5, [0, 0], [0, 0, 0]
    for fn in sorted(names):
        c = rows.get(fn)
        if c is None:
            log(f"[！！！Warning] --accuracy: no record for {fn}")
            c = [fn, "unrevised", "0", "0", "0", "0", "0", str(ACC_NO_TRUTH)]
        v = [int(x) for x in c[2:]]
        out.append("\t".join(c[:2] + accuracy_fields(v)))
        counts[v[5]] += 1
        if v[5] == ACC_WITH_TRUTH:
            total = [t + x for t, x in zip(total, v[:5])]
            den = [den[0] + max(v[1], v[0]), den[1] + max(v[3], v[0])]
    out.append("\t".join(["#total", "with_truth"] + [str(t) for t in total] + [identity_field(total[2], den[0]), identity_field(total[4], den[1])]))
    out.append("#reads\t" + "\t".join(str(x) for x in counts))
    _replace_report(path, out, parts)


class ErrclassPart(AccuracyPart):
    """One process' share of the --error_classes file: an `AccuracyPart` - the same truth set, the same --accuracy_max_len, the
    same flags - whose lines carry (d, M) of both forms of a read."""

    def __init__(self, path: Optional[str], truths: Optional[dict], max_len: int = 65536, log: Callable[[str], None] = print):
        ReportPart.__init__(self, path, ERRCLASS_PART_COLS)
        self.truths, self.max_len, self.log, self.warned, self.classes = truths or {}, int(max_len), log, False, None

    @staticmethod
    def rows(ec, lens_in, lens_out, flags):
        """A part line's integers per read from an error-class block (hoststage.read_error_classes' or the device's)."""
        return [[int(e[0]), int(n), int(e[1]), int(e[2]), int(k), int(e[3]), int(e[4]), f] if f == ACC_WITH_TRUTH else [0, int(n), 0, 0, int(k), 0, 0, f]
                for e, n, k, f in zip(np.asarray(ec).tolist(), lens_in, lens_out, flags)]

    def host_rows(self, T, fns, bases, ev_len, a1, a2):
        if not self.warned:
            self.warned = True
            self.log("[！！！Warning] --error_classes: the error classes are computed by the host stage, about 0.3 s per read "
                     "(--device_merge computes them on the GPU)")
        truth, toff, flags = self.block(fns, ev_len)
        ec, lens_out = error_class_rows(T, bases, ev_len, a1, a2, truth, toff)
        return self.rows(ec, ev_len, lens_out, flags)

    def add_unrevised(self, fn: str, text):
        """A read written unrevised (text: what was written, str or bytes): out = in, the classes of what was written."""
        if self.path is None:
            return
        text = text.encode("ascii", "replace") if isinstance(text, str) else bytes(text)
        truth, toff, (flag,) = self.block([fn], [len(text)])
        d, M = hs.edit_classes(truth, text) if flag == ACC_WITH_TRUTH else (0, 0)
        self.add(fn, False, [int(toff[1]), len(text), d, M, len(text), d, M, flag])


class InfixPart(AccuracyPart):
    """One process' share of the --infix file: an `AccuracyPart` - the same truth set (every truth a REGION here), the same
    --accuracy_max_len, the same flags - whose lines carry the infix block's sixteen figures of a read."""

    def __init__(self, path: Optional[str], truths: Optional[dict], max_len: int = 65536, strands: int = 2, log: Callable[[str], None] = print):
        ReportPart.__init__(self, path, INFIX_PART_COLS)
        self.truths, self.max_len, self.log, self.warned, self.classes, self.infix = truths or {}, int(max_len), log, False, None, None
        self.strands = int(strands)
        self.labels = None                            # --labels: a `LabelsPart` rides along (a read's labels follow from its line)

    def close(self):
        if self.labels is not None:
            self.labels.close()
        super().close()

    @staticmethod
    def rows(blk, lens_in, lens_out, flags):
        """A part line's integers per read from an infix block (hoststage.read_infix's or the device's)."""
        return [[int(e[0]), int(e[1]), int(n), int(k)] + [int(x) for x in e[2:18]] + [f] if f == ACC_WITH_TRUTH
                else [0, 0, int(n), int(k)] + [0] * 16 + [f]
                for e, n, k, f in zip(np.asarray(blk).tolist(), lens_in, lens_out, flags)]

    def host_rows(self, T, fns, bases, ev_len, a1, a2):
        if not self.warned:
            self.warned = True
            self.log("[！！！Warning] --infix: the reads are placed in their truth regions by the host stage, about 2 s per read "
                     "(--device_merge places them on the GPU)")
        truth, toff, flags = self.block(fns, ev_len)
        blk, lens_out = infix_rows(T, bases, ev_len, a1, a2, truth, toff, self.strands)
        return self.rows(blk, ev_len, lens_out, flags)

    def add_unrevised(self, fn: str, text):
        """A read written unrevised (text: what was written, str or bytes): out = in, the figures of what was written."""
        if self.path is None:
            return
        text = text.encode("ascii", "replace") if isinstance(text, str) else bytes(text)
        truth, toff, (flag,) = self.block([fn], [len(text)])
        g = [0] * 8
        if flag == ACC_WITH_TRUTH:
            g = [int(x) for rev in range(self.strands) for x in hs.infix_classes(truth, text, bool(rev))] + [0] * (4 * (2 - self.strands))
        row = [int(toff[1]), self.strands if flag == ACC_WITH_TRUTH else 0, len(text), len(text)] + g + g + [flag]
        self.add(fn, False, row)
        if self.labels is not None:                   # --labels: the bases that were written ARE the original bases
            self.labels.add_read(fn, text, row)


LABELS_HEADER = ("name\tstatus\tstrand\tstart\tend\tlen\tmatch\tsub\tins\tdel\tclip_start\tclip_end\tlead_del\t"
                 + "\t".join(f"label1_{k}" for k in range(6)) + "\t" + "\t".join(f"label2_{k}" for k in range(6)))
LABELS_PART_COLS = 24                      # a part line's integers: reverse, start, end, len, the seven figures, 6 + 6 counts, flag
LABELS_STATUS = {ACC_WITH_TRUTH: "with_truth", ACC_NO_TRUTH: "no_truth", ACC_TOO_LONG: "too_long"}


def labels_index_path(labels_dir: str) -> str:
    return os.path.join(labels_dir, "labels.tsv")


def labels_file(labels_dir: str, fast5_fn: str) -> str:
    return os.path.join(labels_dir, fast5_fn.split(".")[0] + "_labels.txt")


def labels_plan(v, n: int):
    """What --labels aligns of a read with n original bases from its --infix part line's integers: (flag, reverse, start, end),
    start / end on the strand `infix_fields` reports (`hoststage.pick_strand`), those of the ORIGINAL read.  A read that is not
    with_truth keeps its flag; one whose length or end - start exceeds LABELS_MAX_LEN becomes too_long."""
    v = [int(x) for x in v[:INFIX_PART_COLS]]
    if v[-1] != ACC_WITH_TRUTH:
        return v[-1], 0, 0, 0
    rev = hs.pick_strand([v[0], v[1]] + v[4:20]) == "-"
    st, en = (v[10], v[11]) if rev else (v[6], v[7])
    if int(n) > hs.LABELS_MAX_LEN or en - st > hs.LABELS_MAX_LEN:
        return ACC_TOO_LONG, 0, 0, 0
    return ACC_WITH_TRUTH, int(rev), st, en


class LabelsPart(ReportPart):
    """One process' share of --labels: the files DIR/<stem>_labels.txt, written by temporary + rename, and the part of the index
    DIR/labels.tsv (`merge_labels`).  It rides on an `InfixPart`: a read's labels are formed when its --infix line is."""

    def __init__(self, labels_dir: Optional[str], rank, truths: Optional[dict], log: Callable[[str], None] = print):
        super().__init__(report_part_path(labels_index_path(labels_dir), rank) if labels_dir else None, LABELS_PART_COLS)
        self.dir, self.truths, self.log, self.warned = labels_dir, truths or {}, log, False

    def add_read(self, fn: str, bases, inf_row, result=None):
        """The labels of one read: bases (its ORIGINAL bases, uint8 / bytes / str), inf_row (the integers of its --infix part
        line), result ((label bytes, the seven figures) found on the device for `labels_plan`'s bounds, or None: the host stage
        aligns, `hoststage.align_labels`)."""
        if self.path is None:
            return
        b = hs._as_u8(bases.encode("ascii", "replace") if isinstance(bases, str) else bases)
        flag, rev, st, en = labels_plan(inf_row, b.size)
        out = labels_file(self.dir, fn)
        if flag != ACC_WITH_TRUTH:                     # no file: not one an earlier run left either
            try:
                os.remove(out)
            except OSError:
                pass
            self.add(fn, False, [0, 0, 0, b.size] + [0] * 19 + [flag])
            return
        if result is None:
            if not self.warned:
                self.warned = True
                self.log("[！！！Warning] --labels: the reads are aligned to their truth regions by the host stage "
                         "(--device_merge aligns them on the GPU)")
            result = hs.align_labels(truth_of(self.truths, fn), b, bool(rev), st, en)
        lab, summ = np.asarray(result[0], np.uint8).reshape(-1), [int(x) for x in np.asarray(result[1]).reshape(-1)]
        m = int(inf_row[0])
        lo, hi = (m - en, m - st) if rev else (st, en)  # 0-based half-open on the region AS GIVEN, as the --infix line has them
        mp, l1, l2 = hs.label_strings(lab)
        head = "\t".join(["#" + fn, "-" if rev else "+", str(lo), str(hi), str(b.size)] + [str(x) for x in summ])
        tmp = f"{out}.tmp{os.getpid()}"
        with open(tmp, "w") as fp:
            fp.write("\n".join([head, b.tobytes().decode("ascii", "replace"), mp, l1, l2]) + "\n")
        os.replace(tmp, out)
        self.add(fn, True, [rev, lo, hi, b.size] + summ + [l1.count(str(k)) for k in range(6)] + [l2.count(str(k)) for k in range(6)] + [flag])


def merge_labels(labels_dir: str, names: Sequence[str], log: Callable[[str], None] = print):
    """Parent side of --labels: DIR/labels.tsv from the parts as `merge_infix` reads them - one line per read of `names` sorted by
    file name, then #total, the sums over the reads with a file of len, the seven figures and the twelve class counts (`.` in the
    columns of strand, start and end), and #reads with_truth / no_truth / too_long; the file appears by rename and the parts are
    removed."""
    path = labels_index_path(labels_dir)
    rows, parts = _part_rows(path, LABELS_PART_COLS)
    out, t, counts = [LABELS_HEADER], [0] * 20, [0, 0, 0]
    for fn in sorted(names):
        c = rows.get(fn)
        if c is None:
            log(f"[！！！Warning] --labels: no record for {fn}")
            c = [fn, "unrevised"] + ["0"] * (LABELS_PART_COLS - 1) + [str(ACC_NO_TRUTH)]
        v = [int(x) for x in c[2:]]
        counts[v[-1]] += 1
        if v[-1] == ACC_WITH_TRUTH:
            out.append("\t".join([fn, LABELS_STATUS[v[-1]], "-" if v[0] else "+"] + [str(x) for x in v[1:23]]))
            t = [a + b for a, b in zip(t, v[3:23])]
        else:
            out.append("\t".join([fn, LABELS_STATUS[v[-1]], ".", ".", ".", str(v[3])] + ["."] * 19))
    out.append("\t".join(["#total", "with_truth", ".", ".", "."] + [str(x) for x in t]))
    out.append("#reads\t" + "\t".join(str(x) for x in counts))
    _replace_report(path, out, parts)


SCORE_SCORED, SCORE_STALE, SCORE_NO_LABELS = 0, 1, 2
SCORE_STATUS = {SCORE_SCORED: "scored", SCORE_STALE: "stale_labels", SCORE_NO_LABELS: "no_labels"}
SCORE_PART_COLS = hs.SCORE_COLS + 1        # a part line's integers: the read's row of the score block, then its flag
SCORE_HEADER = ("name\tstatus\twindows\tlabelled\tcorrect1\tcorrect2\tacc1\tacc2\tloss1\tloss2\t"
                + "\t".join(f"{d}_{k}" for d in hs.SCORE_DECISIONS for k in hs.SCORE_KINDS) + "\tsub_right")


def score_fields(v) -> List[str]:
    """The fields of a --score line behind name and status from a row of the score block: integers, and the four figures that
    follow from integers alone - acc = correct / labelled and loss = nll16 sum x ln 2 / 65536 / labelled (nats), six decimals,
    `.` without a labelled window."""
    v = [int(x) for x in v[:hs.SCORE_COLS]]
    n = v[hs.SC_LABELLED]
    ok1, ok2 = sum(v[hs.SC_CONF1 + 7 * k] for k in range(6)), sum(v[hs.SC_CONF2 + 6 * k] for k in range(5))
    ratio = lambda a: f"{a / n:.6f}" if n else "."
    loss = lambda s: f"{s * math.log(2.0) / 65536.0 / n:.6f}" if n else "."
    return [str(v[0]), str(n), str(ok1), str(ok2), ratio(ok1), ratio(ok2), loss(v[hs.SC_NLL1]), loss(v[hs.SC_NLL2])] + \
        [str(x) for x in v[hs.SC_DEC_KIND:hs.SC_DEC_KIND + 20]] + [str(v[hs.SC_SUB_RIGHT])]


def _score_closing(t) -> List[str]:
    """The lines behind #total from the summed block: the two confusion matrices (a line per TRUE class, a column per answer) and,
    per model, a line per non-empty confidence bin - the Phred the quality rule gives the bin, n, ok and the empirical Phred
    -10 log10((n - ok + 0.5) / (n + 1)), two decimals."""
    out = [f"#confusion1\t{k}\t" + "\t".join(str(x) for x in t[hs.SC_CONF1 + 6 * k:hs.SC_CONF1 + 6 * k + 6]) for k in range(6)]
    out += [f"#confusion2\t{k}\t" + "\t".join(str(x) for x in t[hs.SC_CONF2 + 5 * k:hs.SC_CONF2 + 5 * k + 5]) for k in range(5)]
    for tag, at_n, at_ok in (("#calibration1", hs.SC_CAL1_N, hs.SC_CAL1_OK), ("#calibration2", hs.SC_CAL2_N, hs.SC_CAL2_OK)):
        for b in range(hs.SCORE_BINS):
            n, ok = t[at_n + b], t[at_ok + b]
            if n:
                out.append(f"{tag}\t{b + 1}\t{n}\t{ok}\t{-10.0 * math.log10((n - ok + 0.5) / (n + 1)):.2f}")
    return out


class ScorePart(ReportPart):
    """One process' share of the --score file, and what forms its lines: the label bytes of a read from --labels_from
    (`read_labels`, `block`), the rows of the host routes (`host_rows`) and of a read written unrevised (`add_unrevised`)."""

    def __init__(self, path: Optional[str], labels_dir: Optional[str], log: Callable[[str], None] = print):
        super().__init__(path, SCORE_PART_COLS)
        self.dir, self.log, self.warned = labels_dir, log, False

    def announce(self, fns, flags):
        """One warning per process, for the first stale labels file it meets."""
        for fn, f in zip(fns, flags):
            if f == SCORE_STALE and not self.warned:
                self.warned = True
                self.log(f"[！！！Warning] --score: {labels_file(self.dir, fn)} does not hold this read's bases; it is not scored "
                         "(stale_labels; further ones are not announced)")

    def read_labels(self, fn: str, bases):
        """(label bytes uint8[n], flag) of a read with the original bases `bases` (uint8): from <stem>_labels.txt where its
        bases line is the read's; every byte 0xFF where there is no file (no_labels) or it holds other bases (stale_labels).
        Silent (it also runs in the parser pool): `announce` speaks."""
        none = np.full(bases.size, hs.SCORE_UNLABELLED, np.uint8)
        try:
            with open(labels_file(self.dir, fn)) as fp:
                lines = fp.read().split("\n")
        except OSError:
            return none, SCORE_NO_LABELS
        try:
            if lines[1].encode("ascii", "replace") != bases.tobytes():
                raise ValueError("other bases")
            return hs.score_labels_from_text(*lines[:5]), SCORE_SCORED
        except (ValueError, IndexError, TypeError):
            return none, SCORE_STALE

    def block(self, fns, bases, ev_len):
        """The labels of a device call: (labels uint8[N], flags)."""
        b, off = hostlib.bases_u8(bases), np.concatenate([[0], np.cumsum(np.asarray(ev_len, np.int64))])
        got = [self.read_labels(fn, b[int(off[r]):int(off[r + 1])]) for r, fn in enumerate(fns)]
        return (np.concatenate([g[0] for g in got]) if got else np.zeros(0, np.uint8)), [g[1] for g in got]

    @staticmethod
    def rows(block, flags):
        """A part line's integers per read from a score block (hoststage.score_calls' or the device's)."""
        return [row + [f] for row, f in zip(np.asarray(block).tolist(), flags)]

    def host_rows(self, T, fns, bases, ev_len, p1, p2, a1, a2, found=None):
        """The same on a host route, from the calls; found: (labels, flags) where `block` has run for these reads already."""
        labels, flags = found if found is not None else self.block(fns, bases, ev_len)
        self.announce(fns, flags)
        return self.rows(hs.score_calls(hostlib.bases_u8(bases), ev_len, a1, a2, p1, p2, labels, phred_thresholds(), T), flags)

    def add_unrevised(self, fn: str):
        self.add(fn, False, [0] * SCORE_PART_COLS)


def merge_score(path: str, names: Sequence[str], log: Callable[[str], None] = print):
    """Parent side of --score: the parts as `merge_report` reads them, one line per read of `names` sorted by file name
    (`score_fields`), then #total - the sums over the scored reads -, the lines of `_score_closing` on those sums and #reads
    scored / stale_labels / no_labels / unrevised; the file appears by rename and the parts are removed."""
    rows, parts = _part_rows(path, SCORE_PART_COLS)
    out, t, counts = [SCORE_HEADER], [0] * hs.SCORE_COLS, [0, 0, 0, 0]
    for fn in sorted(names):
        c = rows.get(fn)
        if c is None:
            log(f"[！！！Warning] --score: no record for {fn}")
            c = [fn, "unrevised"] + ["0"] * SCORE_PART_COLS
        v = [int(x) for x in c[2:]]
        status = SCORE_STATUS.get(v[-1], "scored") if c[1] == "revised" else "unrevised"
        counts[3 if status == "unrevised" else v[-1]] += 1
        out.append("\t".join([fn, status] + score_fields(v)))
        if status == "scored":
            t = [a + b for a, b in zip(t, v)]
    out.append("\t".join(["#total", "scored"] + score_fields(t)))
    out += _score_closing(t)
    out.append("#reads\t" + "\t".join(str(x) for x in counts))
    _replace_report(path, out, parts)


def merge_infix(path: str, names: Sequence[str], log: Callable[[str], None] = print):
    """Parent side of --infix: the parts as `merge_report` reads them, one line per read of `names` sorted by file name, then
    #total - over the reads WITH a truth, revised or not, the sums of truth_len and of len, dist and match of both forms (`.` in
    the columns of strand, start and end, which do not add up) and the pooled identities sum(match) / (sum(match) + sum(dist)) -
    and #reads with_truth / no_truth / too_long; the file appears by rename and the parts are removed."""
    rows, parts = _part_rows(path, INFIX_PART_COLS)
    out, t, counts = [INFIX_HEADER], [0] * 7, [0, 0, 0]
    for fn in sorted(names):
        c = rows.get(fn)
        if c is None:
            log(f"[！！！Warning] --infix: no record for {fn}")
            c = [fn, "unrevised"] + ["0"] * (INFIX_PART_COLS - 1) + [str(ACC_NO_TRUTH)]
        v = [int(x) for x in c[2:]]
        out.append("\t".join(c[:2] + infix_fields(v)))
        counts[v[-1]] += 1
        if v[-1] == ACC_WITH_TRUTH:
            t = [a + b for a, b in zip(t, infix_sums(v))]
    out.append("\t".join(["#total", "with_truth", str(t[0]), ".", str(t[1]), str(t[2]), str(t[3]), ".", ".", infix_identity(t[3], t[2]),
                          str(t[4]), str(t[5]), str(t[6]), ".", ".", infix_identity(t[6], t[5])]))
    out.append("#reads\t" + "\t".join(str(x) for x in counts))
    _replace_report(path, out, parts)


def merge_error_classes(path: str, names: Sequence[str], log: Callable[[str], None] = print):
    """Parent side of --error_classes: the parts as `merge_report` reads them, one line per read of `names` sorted by file name,
    then #total - the sums over the reads WITH a truth, revised or not, and the pooled rates count / sum(truth_len) - and #reads
    with_truth / no_truth / too_long; the file appears by rename and the parts are removed."""
    rows, parts = _part_rows(path, ERRCLASS_PART_COLS)
    out, total, counts = [ERRCLASS_HEADER], [0] * (ERRCLASS_PART_COLS - 1), [0, 0, 0]
    for fn in sorted(names):
        c = rows.get(fn)
        if c is None:
            log(f"[！！！Warning] --error_classes: no record for {fn}")
            c = [fn, "unrevised"] + ["0"] * (ERRCLASS_PART_COLS - 1) + [str(ACC_NO_TRUTH)]
        v = [int(x) for x in c[2:]]
        out.append("\t".join(c[:2] + error_class_fields(v)))
        counts[v[-1]] += 1
        if v[-1] == ACC_WITH_TRUTH:
            total = [t + x for t, x in zip(total, v[:-1])]
    out.append("\t".join(["#total", "with_truth"] + error_class_fields(total + [ACC_WITH_TRUTH], rates=True)))
    out.append("#reads\t" + "\t".join(str(x) for x in counts))
    _replace_report(path, out, parts)


EDITS_HEADER = "#pos_in\tpos_out\tkind\tref\talt\tqual\tconf"


def edits_name(edits_dir: str, fast5_fn: str) -> str:
    return os.path.join(edits_dir, fast5_fn.split(".")[0] + "_edits.tsv")


def edit_rows(T, bases, ev_len, p1, p2, a1, a2, want_qual):
    """--edits on the host: `hoststage.revision_edits` on calls the host holds, with the quality characters the writers use
    (FASTQ: `phred_chars`; FASTA: none).  (edits, edit_off)."""
    qc = None
    if want_qual:
        qc = phred_chars(p1, p2, a1, a2) if len(a1) else np.zeros(0, np.uint8)
    return hs.revision_edits(hostlib.bases_u8(bases), ev_len, a1, a2, p1, p2, qc, T)


def write_edits(edits_dir: str, fast5_fn: str, edits=None, want_qual: bool = False):
    """One read's <stem>_edits.tsv by temporary + rename: the header, then one line per record (None: a read written unrevised,
    the header alone)."""
    os.makedirs(edits_dir, exist_ok=True)
    lines = [EDITS_HEADER]
    if edits is not None:
        for pi, po, k, ref, alt, q, conf in np.asarray(edits).tolist():
            lines.append(f"{pi}\t{po}\t{hs.EDIT_KINDS[k]}\t{chr(ref)}\t{chr(alt)}\t{chr(q) if want_qual else '.'}\t"
                         + format(float(np.float32(conf)), ".9g"))
    dst = edits_name(edits_dir, fast5_fn)
    tmp = f"{dst}.tmp{os.getpid()}"
    with open(tmp, "w") as fp:
        fp.write("\n".join(lines) + "\n")
    os.replace(tmp, dst)


def _host_merge_form(packed):
    """A `with_device_merge` / `with_device_report` / `with_device_edits` / `with_device_records` / `with_device_profile` /
    `with_device_trim` / `with_device_accuracy` / `with_device_error_classes` / `with_device_infix` / `with_device_score` tuple back in the form whose call returns (p1, p2, a1, a2): for the paths that
    keep the host merge."""
    if packed is None or len(packed) not in (12, 14, 16, 20, 22, 27, 30, 31, 33, 36):
        return packed
    return tuple(packed[:7]) if packed[7] is None else tuple(packed[:9])


def _is_merged_ticket(tk) -> bool:
    """The ticket of a call that comes back as revised reads (seq, qual, off[, report]): engine.Reviser.begin_packed_raw."""
    return isinstance(tk, tuple) and len(tk) == 3


def _bundle_has_bases(bundle) -> bool:
    """This bundle carries one original base per event: what the bundle finishers and the device merge work from."""
    return "bases" in bundle and len(bundle["bases"]) == int(bundle["meta"][:, 1].sum())


def _route_batch(rv, bundle, n_reads, pipelined, native_pool, device_merge, report, edits=False, combined=False, summary=False,
                 trim=False, accuracy=False, error_classes=False, infix=False, score=False):
    """The one decision about a batch: (packed form `_FileRun.submit` builds, route `_FileRun.run_batch` takes).  Pure: it looks at what
    the engine object offers, at the bundle (None: reads that arrived one by one) and at the run's switches - pipelined (one
    engine, NRV_CLI_PIPELINE != 0), native_pool (libnanorev_host.so driven from the thread pool), device_merge (--device_merge
    and what it needs: pipelined, native_pool, nrvh_write_records), report (--report), edits (--edits), combined (--combined),
    summary (--summary), trim (--trim_q), accuracy (--truth / --accuracy), error_classes (--error_classes), infix (--infix), score
    (--score).  "bases":
    `_bundle_has_bases`.  A form is
    the length of the packed tuple (engine.Reviser), None, or "host-merge": the merge form built and taken back.

      bundle  engine offers / bundle / switches                              form            route
      none    one read                                                       None            per-read
      none    several reads, no pack_reads_raw                               None            predict_many
      none    several reads, pack_reads_raw                                  7 [1]           predict_many
      yes     no run_packed_raw                                              None            predict_many (one read: per-read)
      yes     run_packed_raw; bundle without / with "device_stats"           7 / 9           by the last three rows
      yes     + device_merge, with_device_merge, bases; report off           12              by the last three rows
      yes     + report on, with_device_report                                14              by the last three rows
      yes     + report on, no with_device_report                             host-merge [2]  by the last three rows
      yes     + edits on, with_device_edits (+ report on: with_device_report)  16 [4]          by the last three rows
      yes     + edits on, one of them missing                                host-merge [2]  by the last three rows
      yes     + combined on, a form 12 / 14 / 16 above, with_device_records  20 [5]          by the last three rows
      yes     + combined on, no with_device_records                          12 / 14 / 16 [6]  by the last three rows
      yes     + summary on, a form 12 / 14 / 16 / 20 above, with_device_profile  22 [7]        by the last three rows
      yes     + summary on, such a form, no with_device_profile              host-merge [2]  by the last three rows
      yes     + trim on, a form 12 / 14 / 16 / 20 / 22 above, with_device_trim  27 [8]         by the last three rows
      yes     + trim on, such a form, no with_device_trim                    host-merge [2]  by the last three rows
      yes     + accuracy on, a form 12 ... 27 above, with_device_accuracy    30 [9]          by the last three rows
      yes     + accuracy on, such a form, no with_device_accuracy            host-merge [2]  by the last three rows
      yes     + error_classes on, form 30 above, with_device_error_classes   31 [10]         by the last three rows
      yes     + error_classes on, form 30 above, no with_device_error_classes  host-merge [2]  by the last three rows
      yes     + infix on, a form 12 ... 31 above, with_device_accuracy + _infix  33 [11]         by the last three rows
      yes     + infix on, such a form, one of the two missing                host-merge [2]  by the last three rows
      yes     + score on, a form 12 ... 33 above, with_device_score          36 [12]         by the last three rows
      yes     + score on, such a form, no with_device_score                  host-merge [2]  by the last three rows
      yes     any form; pipelined, native_pool, begin_packed_raw, bases                      pipelined [3]
      yes     any form; native_pool, bases, not (pipelined, begin_packed_raw)                packed+finish_bundle
      yes     any form; no native_pool, or no bases                                          packed sliced

    [1] None when `prepare_many` declines (not all raw reads) or building a form raises; the route is then predict_many.
    [2] the whole bundle on the host: merge, quality and report rows from the calls.
    [3] begin_packed_raw raising -> packed+finish_bundle.  Every route but this one takes a 12 / 14 form back through
        `_host_merge_form`; any call raising -> per-read retries on reads that `_bundle_reads` completes on the host.
    [4] the one call carries the report too when --report is set.
    [5] the one call carries the report and the edit list too when --report / --edits are set; its blob is appended to the
        --combined part as it is, and no native writer is called.
    [6] the merged reads come back and the host forms the records (hoststage.pack_records), as on every host route.
    [7] the one call carries whatever the form above carried (report, edit list, records) and the per-read profile last; every
        other route forms the summary rows on the host from the calls (`profile_rows`).
    [8] the one call carries whatever the form above carried and the per-read trim bounds last; its records, where it has some,
        are those of the trimmed reads.  Every other route finds the bounds on the host from the calls (`trim_rows`); `deliver`
        applies them on every route.
    [9] the one call carries whatever the form above carried and the accuracy block last: per read the edit distance of the
        original and of the (untrimmed) revised read to its truth.  Every other route computes the rows on the host from the
        reads it holds (`accuracy_rows`).
    [10] the one call is the form 30 call with the error-class block behind the accuracy block: per read the edits and the matched
        columns of the original and of the (untrimmed) revised read against its truth.  Every other route computes the rows on
        the host (`error_class_rows`) - an engine without the call too: a form 30 call need not hand the merged characters back,
        so the route is the one the accuracy takes without ITS call.
    [11] the one call is the form 30 / 31 call - without --accuracy a form 30 call whose accuracy block nobody reads - with the
        infix block last: per read where the original and the (untrimmed) revised read lie in the truth region, per strand.
        Every other route computes the rows on the host (`infix_rows`).
    [12] the one call is the call of the form above - `_route_batch(..., score=False)` names it - with the label bytes of its
        reads going up and the score block last.  Every other route scores on the host from the calls (`ScorePart.host_rows`)."""
    unpacked = "per-read" if n_reads == 1 else "predict_many"
    if bundle is None:
        return (7 if n_reads > 1 and hasattr(rv, "pack_reads_raw") else None), unpacked
    if not hasattr(rv, "run_packed_raw"):
        return None, unpacked
    bases = _bundle_has_bases(bundle)
    form = 9 if "device_stats" in bundle else 7
    if device_merge and hasattr(rv, "with_device_merge") and bases:
        form = 12 if not report else (14 if hasattr(rv, "with_device_report") else "host-merge")
        if edits:
            form = 16 if hasattr(rv, "with_device_edits") and form != "host-merge" else "host-merge"
        if combined and form != "host-merge" and hasattr(rv, "with_device_records"):
            form = 20
        if summary and form != "host-merge":
            form = 22 if hasattr(rv, "with_device_profile") else "host-merge"
        if trim and form != "host-merge":
            form = 27 if hasattr(rv, "with_device_trim") else "host-merge"
        if accuracy and form != "host-merge":
            form = 30 if hasattr(rv, "with_device_accuracy") else "host-merge"
        if error_classes and form == 30:
            form = 31 if hasattr(rv, "with_device_error_classes") else "host-merge"
        if infix and form != "host-merge":
            if form not in (30, 31):
                form = 30 if hasattr(rv, "with_device_accuracy") else "host-merge"
            if form != "host-merge":
                form = 33 if hasattr(rv, "with_device_infix") else "host-merge"
        if score and form != "host-merge":
            form = 36 if hasattr(rv, "with_device_score") else "host-merge"
    if not (native_pool and bases):
        return form, "packed sliced"
    return form, ("pipelined" if pipelined and hasattr(rv, "begin_packed_raw") else "packed+finish_bundle")


def usable_cores() -> int:
    """Cores this process can really use: its affinity mask, cut down to the cgroup's CPU quota (a container that shows
    256 CPUs and grants 16 runs sixteen parser workers, not the 32 that --thread's default of 100 would otherwise give:
    r03, 4000 reads: 8 workers 11.1, 16 workers 10.4 M bases/s end to end)."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            cores = min(cores, int(float(q) / float(per) + 0.5))
    except Exception:
        pass
    return max(1, cores)


def write_read(args, fast5_fn: str, seq: str, qual: Optional[str]):
    os.makedirs(args.output_dir, exist_ok=True)
    if args.output_format == "fastq":
        text = hs.fastq_record(fast5_fn, list(seq), list(qual if qual is not None else "#" * len(seq)))
    else:
        text = hs.fasta_record(fast5_fn, list(seq))
    # atomic: a worker killed mid-write leaves a stray temporary, never a truncated <read>_out file
    dst = out_name(args.output_dir, fast5_fn, args.output_format)
    tmp = f"{dst}.tmp{os.getpid()}"
    with open(tmp, "w") as fp:
        fp.write(text)
    os.replace(tmp, dst)


kNativePoolMax = 4      # parser THREADS per GPU worker with the native host stage: 4 deliver 23 M bases/s (r04, 16-core cgroup),
                        # twice what one GPU takes; more only take the GIL from the engine thread (r04, 4000 reads end to
                        # end: 2 / 4 / 8 / 16 threads = 11.2 / 11.3 / 10.2 / 9.3 M bases/s).  NRV_PARSER_THREADS_MAX overrides
                        # it (INTEGRATION.md "Process-wide settings"); the cap was tuned at kSwitchInterval.
kSwitchInterval = 2e-4  # CPython switch interval while the parser threads run (see process_files)


def native_pool_max() -> int:
    try:
        return max(1, int(os.environ.get("NRV_PARSER_THREADS_MAX", kNativePoolMax)))
    except ValueError:
        return kNativePoolMax


def parser_pool_size(threads: int, cores: int, gpu_workers: int, n_files: int, native: bool = False) -> int:
    """Parser workers of ONE GPU worker: --thread, capped at this worker's share of the cores the process may use
    (cores // gpu_workers, at least 1), at 32 (processes on the Python host stage) or kNativePoolMax (threads on the
    native one) and at the number of files."""
    share = max(1, cores // max(1, gpu_workers))
    return max(1, min(int(threads), share, native_pool_max() if native else 32, max(1, n_files)))


class _Trace:
    """NRV_CLI_TRACE=1: where the wall time of a `process_files` call goes, to the log.  Without it no method does anything."""

    def __init__(self):
        self.on, self.t_start, self.items = bool(os.environ.get("NRV_CLI_TRACE")), time.perf_counter(), []
        if self.on:
            try:                                      # age of this process: interpreter start, imports, main() so far
                with open("/proc/self/stat") as f:
                    ticks = int(f.read().rsplit(")", 1)[1].split()[19])
                with open("/proc/uptime") as f:
                    self.items.append(("mark", 0.0, f"process age {float(f.read().split()[0]) - ticks / os.sysconf('SC_CLK_TCK'):.2f} s at"))
            except Exception:
                pass

    def mark(self, what):
        if self.on:
            self.items.append(("mark", time.perf_counter() - self.t_start, what))

    def call_begin(self, t0):
        if self.on:
            self.items.append(("call", t0 - self.t_start, 0.0))
            return len(self.items) - 1

    def call_end(self, ti, t0):
        if ti is not None:
            self.items[ti] = ("call", t0 - self.t_start, time.perf_counter() - t0)

    def log_summary(self, log, n_engines):
        calls = sorted((c for c in self.items if c[0] == "call"), key=lambda c: c[1])
        if self.items and not calls:                  # every file failed before a device call: only the marks
            log("[trace] " + "; ".join(f"{w} {t:.3f} s" for k, t, w in self.items if k == "mark") + "; no device call")
        if not calls:
            return
        t_end = time.perf_counter() - self.t_start
        busy, idle, end = sum(c[2] for c in calls), 0.0, calls[0][1]
        for _, t, d in calls:                         # time with NO engine inside a call, between the first and the last call
            idle += max(0.0, t - end)
            end = max(end, t + d)
        log("[trace] " + "; ".join(f"{w} {t:.3f} s" for k, t, w in self.items if k == "mark"))
        log(f"[trace] process_files {t_end:.3f} s: first device call at {calls[0][1]:.3f} s, {len(calls)} calls on "
            f"{n_engines} engine(s), {busy:.3f} s summed, no call running for {idle:.3f} s, "
            f"tail after the last call {t_end - end:.3f} s; first call {calls[0][2]:.3f} s, "
            f"median call {sorted(c[2] for c in calls)[len(calls) // 2]:.4f} s")


class _FileRun:
    """One `process_files` call: its state and its three kinds of thread.  MAIN reads `results()`, packs device calls as
    `_route_batch` says (`submit`) and collects the pooled finishers; the ENGINE thread(s) make the calls (`run_batch`, `collect`);
    the one FINISHER thread merges, reports and writes, or hands that to the parser pool (`finish_batch`, `finish_call`)."""
    def __init__(self, stack, args, files, reviser, log, on_file, gpu_workers, core_share, report_part, combined_part=None,
                 summary_part=None, trim_part=None, accuracy_part=None, errclass_part=None, infix_part=None, score_part=None):
        self.args, self.log, self.note = args, log, on_file or (lambda fn, ok: None)
        self.stats = {"reads": 0, "bases": 0, "failed": [], "host_s": 0.0, "engine_s": 0.0}
        self.stats_lock = threading.Lock()
        self.report = ReportPart(report_part)
        self.rep_rows = {}                            # fn -> the row of a read whose output is not final yet
        self.sumpart = ReportPart(summary_part, SUMMARY_COLS)        # --summary: stashed and emitted wherever a report row is
        self.sum_rows = {}
        self.trim = trim_rule(args)                   # --trim_q: (Q, W, min_len); the bounds are stashed like a report row and
        self.trim_rows = {}                           # applied by `deliver`; fn -> (bases of the untrimmed read, (lo, hi))
        self.trimpart = ReportPart(trim_part if self.trim else None, 4)
        # --truth / --accuracy: the rows are stashed like a report row; every process loads the truth set itself
        self.accpart = AccuracyPart(accuracy_part, load_truth(args.truth) if accuracy_part or infix_part else None,
                                    getattr(args, "accuracy_max_len", 65536), log)
        self.acc_rows = {}
        # --error_classes: its own part next to the accuracy's, on the truth set that one loaded
        self.eclpart = ErrclassPart(errclass_part if accuracy_part else None, self.accpart.truths, self.accpart.max_len, log)
        self.ecl_rows = {}
        # --infix: a part of its own on the same truth set, with or without --accuracy
        self.infpart = InfixPart(infix_part, self.accpart.truths, self.accpart.max_len,
                                 1 if getattr(args, "infix_strand", "both") == "forward" else 2, log)
        self.inf_rows = {}
        # --labels: rides on the infix part (the part of its index carries the suffix of the infix part); fn -> (the read's
        # original bases, its labels from the device | None) is stashed wherever an infix row is
        if getattr(args, "labels", None) and infix_part:
            self.infpart.labels = LabelsPart(args.labels, infix_part.rsplit(".part", 1)[-1], self.accpart.truths, log)
        # --score: the rows are stashed like a report row; id(batch) -> (labels, flags) of a form 36 call, until its reads are final
        self.scorepart = ScorePart(score_part, getattr(args, "labels_from", None), log)
        self.score_rows, self.score_in = {}, {}
        self.lab_in = {}
        self.lab_truth = {}                           # id(batch) -> (truth, truth_off) of a form 33 call, until its call is back
        self.acc_flags = {}                           # id(batch) -> the flags of a form 30 call's truth block, until its call is back
        self.tie_eps = float(getattr(args, "report_tie_eps", hs.REPORT_TIE_EPS))
        self.edits_dir = getattr(args, "edits", None) # --edits: every read's list is written BEFORE its output is
        self.sink = CombinedPart(combined_part, args.output_format == "fastq") if combined_part else None   # --combined (`deliver`)
        self.trace = _Trace()
        self.want_qual, self.spec = args.output_format == "fastq", _OutSpec(args)
        # `reviser` may be a zero-argument factory: the engine is then created by the engine thread as its first task, WHILE
        # the parser pool starts and the first reads are parsed (nrv_create: HIP context + weight packing, 0.15-0.3 s)
        self.lazy = callable(reviser) and not hasattr(reviser, "predict_read")
        self.factory, self.rv = reviser, (None if self.lazy else reviser)
        # NRV_CLI_ENGINES=n: n engines on the same device, one thread each, so that one call's fill / drain overlaps the other's
        # kernels.  Slower than one (HISTORY.md r03j: 10.1-10.4 against 11.0 M bases/s): the default stays ONE, the knob is tested.
        self.n_eng = max(1, int(os.environ.get("NRV_CLI_ENGINES", "1"))) if self.lazy else 1
        self.free, self.engines = queue.Queue(), []   # engines not inside a call; all engines
        if not self.lazy:
            self.free.put(reviser)
            self.engines.append(reviser)
        self.created = None                           # the future of the first engine's creation (lazy)
        self.native_threads = hostlib.load() is not None and os.environ.get("NRV_HOST_THREADS", "1") != "0"
        self.nworkers = parser_pool_size(int(args.thread), usable_cores(), gpu_workers, len(files), native=self.native_threads) \
            if core_share is None else parser_pool_size(int(args.thread), int(core_share), 1, len(files), native=self.native_threads)
        self.stats["parser_workers"] = self.nworkers
        self.jobs = [(os.path.join(args.fast5_base_dir, fn), fn, args.basecall_group, args.basecall_subgroup,
                      args.output_format == "fastq") for fn in files]
        # One worker task = one device call of >= batch_events events (~6.5 k per read), handed back concatenated (`_load_bundle`):
        # 16 launch groups (HISTORY.md r03: 8 -> 7.6, 16 -> 10.2, 32 -> 10.3 M bases/s), but never so many reads that the workers run dry
        self.batch_events = int(os.environ.get("NRV_CLI_GROUPS", "16")) * max(int(getattr(args, "batch", 4096)), 1024)
        self.per_task = max(1, min(32, self.batch_events // 6500, -(-len(self.jobs) // (2 * self.nworkers))))
        self.finishing = []                           # (future, fn, rt, fq) of merges handed to the pool
        self.pending = {}                             # id(engine) -> the call in flight on it: (ticket, batch, bundle, trace index, t0)
        self.inflight = deque()                       # futures of the engine thread's tasks, oldest first
        self.done = Future()                          # what an engine task returns when it handed nothing to the finisher
        self.done.set_result(None)
        self._start(stack, len(files))

    def _start(self, stack, n_files):
        """The parser pool - THREADS inside libnanorev_host.so (one C call per bundle and per finished read, GIL released), else
        PROCESSES on the Python host stage -, the switches that depend on it, and the engine and finisher threads.  `stack`
        undoes each step from the moment it is taken: the switch interval is restored and the pool never outlives the call."""
        args, self.pool = self.args, None
        self.stats["host_stage"] = "native, threads" if self.native_threads else \
            ("python, processes" if hostlib.load() is None else "native, processes")
        if self.nworkers > 1 and n_files >= 4 and self.native_threads:
            # A pool thread back from its C call waits a switch interval for the GIL (r04: at 5 ms four threads deliver what one
            # does).  Only touched when at CPython's default, never with NRV_SWITCH_INTERVAL=0.
            try:
                want = float(os.environ.get("NRV_SWITCH_INTERVAL", kSwitchInterval))
            except ValueError:
                want = kSwitchInterval
            if want > 0 and abs(sys.getswitchinterval() - 0.005) < 1e-9:
                stack.callback(sys.setswitchinterval, sys.getswitchinterval())
                sys.setswitchinterval(want)
            self.pool = ThreadPoolExecutor(self.nworkers)
        elif self.nworkers > 1 and n_files >= 4:
            import multiprocessing as mp
            for v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):   # the workers never call BLAS (HISTORY.md r03)
                os.environ.setdefault(v, "1")
            self.pool = ProcessPoolExecutor(self.nworkers, mp_context=mp.get_context("spawn"))
        if self.pool is not None:
            stack.callback(self.pool.shutdown, wait=False, cancel_futures=True)
        # PIPELINED two deep (r06): the engine thread enqueues bundle k+1 (nrv_reads_raw_begin) BEFORE it collects bundle k
        self.pipelined = self.n_eng == 1 and os.environ.get("NRV_CLI_PIPELINE", "1") != "0"
        self.native_pool = self.native_threads and self.pool is not None
        # --device_stats / --device_merge: statistics, merge and records move into the pipelined call, and only there
        self.device_stats = bool(getattr(args, "device_stats", False)) and self.pipelined and self.native_pool
        self.device_merge = (bool(getattr(args, "device_merge", False)) and self.pipelined and self.native_pool
                             and hostlib.has_write_records())
        if self.device_stats:
            self.stats["read_stats"] = "device"
        if self.device_merge:
            self.stats["merge"] = "device"
        self.eng = stack.enter_context(ThreadPoolExecutor(self.n_eng))
        self.fin = stack.enter_context(ThreadPoolExecutor(1))
        if self.lazy:
            self.created = self.eng.submit(self.create, True)
        for _ in range(self.n_eng - 1):
            self.eng.submit(self.create, False)

    def create(self, first):
        if not first and self.created.exception() is not None:       # one at a time, the first one first - or none
            return
        try:
            rv = self.factory()
        except BaseException as e:
            if first:
                raise                                 # no engine at all: loud (submit() re-raises it)
            self.log(f"[s:::] a second engine on this device could not be created ({e!r}): continuing with one")
            return
        if first:
            self.rv = rv
        self.engines.append(rv)
        self.free.put(rv)
        self.trace.mark("engine created")

    def end(self):
        """Main thread, behind the last `submit`: everything in flight comes in, the pool ends in order."""
        if self.pipelined:
            self.inflight.append(self.eng.submit(self.flush_pipeline))
        self.drain(0)
        if self.created is not None:
            self.created.result()
        self.collect_finished(True)
        if self.pool is not None:                     # all work is in: an orderly end of the workers (their queues' semaphores
            self.pool.shutdown(wait=True)             # are released here, not left to the resource tracker)

    def summary(self):
        """After the threads have ended: the report part closed, the trace and the range guard logged; the statistics."""
        self.report.close()
        self.sumpart.close()
        self.trimpart.close()
        self.accpart.close()
        self.eclpart.close()
        self.infpart.close()
        if self.sink is not None:
            self.sink.close()
        self.trace.log_summary(self.log, len(self.engines))
        guarded = [rv for rv in self.engines if callable(getattr(rv, "saturated", None))]
        if guarded:                                   # f16x2 range guard: stages re-run on the f32 kernels
            self.stats["range_reruns"] = sum(int(rv.saturated()[1]) for rv in guarded)
            if self.stats["range_reruns"]:
                self.log(f"[s:::] {self.stats['range_reruns']} device stage(s) held out-of-range signal (spikes / tiny MAD) "
                         "and were computed on the f32 kernels")
        return self.stats

    def results(self):
        """Yields (entries, bundle): `_load_one` tuples, and for pooled tasks their pre-concatenated raw reads."""
        if self.pool is None:
            for j in self.jobs:
                yield [_load_one(j)], None
            return
        pend, nw, per_task = deque(), self.nworkers, self.per_task
        for k in range(0, len(self.jobs), per_task):
            pend.append(self.pool.submit(_load_bundle_labelled, self.jobs[k:k + per_task], self.device_stats, self.scorepart.dir) if self.scorepart
                        else self.pool.submit(_load_bundle, self.jobs[k:k + per_task], True) if self.device_stats
                        else self.pool.submit(_load_bundle, self.jobs[k:k + per_task]))
            if k == 0:
                self.trace.mark("first task submitted (workers started)")
            if len(pend) >= 3 * nw:
                if len(pend) == 3 * nw and k == (3 * nw - 1) * per_task:
                    self.trace.mark("3 x workers tasks submitted")
                yield pend.popleft().result()
                if k == (3 * nw - 1) * per_task:
                    self.trace.mark("first bundle back")
        while pend:
            yield pend.popleft().result()

    def fallback(self, fn, rt, fq, e):                # NanoReviser.py:146-152 / :173-179
        args, log = self.args, self.log
        self.stats["failed"].append(fn)
        log(f"[！！！Error] revising {fn.split('.')[0]}: {e}; writing the original basecalls")
        nw, text = 0, ""
        if self.edits_dir:                            # unrevised: the header alone, replacing what a revision may have left
            try:
                write_edits(self.edits_dir, fn)
            except Exception as e2:
                log(f"[！！！Error] stroring : {fn.split('.')[0]}_edits.tsv...... {e2}")
        try:
            if args.output_format == "fastq" and fq is not None:
                b, q = hs.trim_fastq(fq)
                deliver(args, self.sink, [fn], ("text", b, q))
                nw, text = len(b), b
            else:
                orig = "".join(x.decode() for x in np.asarray(rt.bases).tolist())
                deliver(args, self.sink, [fn], ("text", orig, None))
                nw, text = len(orig), orig
        except Exception as e2:
            log(f"[！！！Error] stroring : {fn.split('.')[0]}_out.{args.output_format}...... {e2}")
        if self.report:
            self.rep_rows.pop(fn, None)
            self.report.add(fn, False, unrevised_row(nw))
        if self.sumpart:
            self.sum_rows.pop(fn, None)
            self.sumpart.add(fn, False, unrevised_profile(text))
        self.trim_rows.pop(fn, None)
        self.trimpart.add(fn, False, unrevised_trim(nw))
        self.acc_rows.pop(fn, None)
        self.accpart.add_unrevised(fn, text)
        self.ecl_rows.pop(fn, None)
        self.eclpart.add_unrevised(fn, text)
        self.inf_rows.pop(fn, None)
        self.lab_in.pop(fn, None)
        self.infpart.add_unrevised(fn, text)
        self.score_rows.pop(fn, None)
        self.scorepart.add_unrevised(fn)
        self.note(fn, False)

    def finished(self, fn, nb):
        self.stats["bases"] += nb
        if self.report:
            row = self.rep_rows.pop(fn, None)
            if row is None:                           # cannot happen: every path that finishes a read stashes its row first
                self.log(f"[！！！Warning] --report: no counts for {fn}")
            self.report.add(fn, row is not None, row if row is not None else unrevised_row(nb))
        if self.sumpart:
            row = self.sum_rows.pop(fn, None)
            if row is None:                           # cannot happen, as above
                self.log(f"[！！！Warning] --summary: no counts for {fn}")
            self.sumpart.add(fn, row is not None, row if row is not None else np.zeros(hs.PROFILE_COLS, np.uint64))
        if self.accpart:
            row = self.acc_rows.pop(fn, None)
            if row is None:                           # cannot happen, as above
                self.log(f"[！！！Warning] --accuracy: no distances for {fn}")
            self.accpart.add(fn, row is not None, row if row is not None else [0, nb, 0, nb, 0, ACC_NO_TRUTH])
        if self.eclpart:
            row = self.ecl_rows.pop(fn, None)
            if row is None:                           # cannot happen, as above
                self.log(f"[！！！Warning] --error_classes: no counts for {fn}")
            self.eclpart.add(fn, row is not None, row if row is not None else [0, nb, 0, 0, nb, 0, 0, ACC_NO_TRUTH])
        if self.infpart:
            row = self.inf_rows.pop(fn, None)
            if row is None:                           # cannot happen, as above
                self.log(f"[！！！Warning] --infix: no figures for {fn}")
            self.infpart.add(fn, row is not None, row if row is not None else [0, 0, nb, nb] + [0] * 16 + [ACC_NO_TRUTH])
            if self.infpart.labels is not None:
                bases, found = self.lab_in.pop(fn, (b"", None))
                self.infpart.labels.add_read(fn, bases, row if row is not None else [0, 0, nb, nb] + [0] * 16 + [ACC_NO_TRUTH], found)
        if self.scorepart:
            row = self.score_rows.pop(fn, None)
            if row is None:                           # cannot happen, as above
                self.log(f"[！！！Warning] --score: no counts for {fn}")
            self.scorepart.add(fn, row is not None, row if row is not None else [0] * SCORE_PART_COLS)
        if self.trim:
            row = self.trim_rows.pop(fn, None)
            log_row = trim_log_row(row[0], row[1], self.trim[2]) if row is not None else unrevised_trim(nb)
            self.trimpart.add(fn, row is not None, log_row)
            if not log_row[3]:
                self.log(f"[p:::] {fn.split('.')[0]} was dropped by --trim_q ({log_row[2] - log_row[1]} of {log_row[0]} bases left)......")
                self.note(fn, True)
                return
        if not self.args.test_mode:
            self.log(f"[p:::] {fn.split('.')[0]}_out.{self.args.output_format} was saved......")
        else:
            self.log("INFO Congratulations, NanoReviser is installed properly")
        self.note(fn, True)

    def submit(self, batch, bundle=None):
        """One batch to the engine thread, in the packed form and on the route `_route_batch` gives.  The NumPy half of the device
        call (descriptors, output arrays, concatenation) happens HERE, while the engine thread is inside the previous call."""
        if self.created is not None:
            self.created.result()                     # raises what the factory raised: loud, no fallback engine
        rv, cls, packed = self.rv, type(self.rv), None
        try:
            if bundle is not None and "device_stats" in bundle and not (hasattr(rv, "run_packed_raw") and hasattr(rv, "with_device_stats")):
                bundle = _bundle_host_stats(bundle)   # an engine without the new calls: the host computes them after all
            form, route = _route_batch(rv, bundle, len(batch), self.pipelined, self.native_pool, self.device_merge, bool(self.report),
                                       edits=bool(self.edits_dir), combined=self.sink is not None, summary=bool(self.sumpart),
                                       trim=self.trim is not None, accuracy=bool(self.accpart), error_classes=bool(self.eclpart),
                                       infix=bool(self.infpart), score=bool(self.scorepart))
            score = form == 36                        # --score: the call of the form without it, with one block more
            if score:
                form, _ = _route_batch(rv, bundle, len(batch), self.pipelined, self.native_pool, self.device_merge, bool(self.report),
                                       edits=bool(self.edits_dir), combined=self.sink is not None, summary=bool(self.sumpart),
                                       trim=self.trim is not None, accuracy=bool(self.accpart), error_classes=bool(self.eclpart),
                                       infix=bool(self.infpart))
            if form is not None and bundle is None:
                packed = prepare_many(cls, [rt for _, rt, _ in batch], rv.T)
            elif form is not None:
                packed = cls.pack_bundle(bundle["raw"], bundle["starts"], bundle["feat"], bundle["meta"], rv.T)
                if "device_stats" in bundle:
                    packed = cls.with_device_stats(packed, bundle["last_dur"], bundle["device_stats"])
                if form != len(packed):               # a merge form: alone, taken back, or - --report - counted on the device too
                    packed = cls.with_device_merge(packed, bundle["bases"], self.want_qual)
                    if form == "host-merge":
                        packed = _host_merge_form(packed)
                    elif form != len(packed):
                        infix, form = form == 33, (31 if form == 33 and self.eclpart else 30 if form == 33 else form)   # --infix: form 30 / 31 with one block more
                        classes, form = form == 31, (30 if form == 31 else form)   # --error_classes: form 30 with one block more
                        if self.report:
                            packed = cls.with_device_report(packed, self.tie_eps)
                        if form == 16 or (form in (20, 22, 27, 30) and self.edits_dir):   # --edits: the list behind the merge (and the report)
                            packed = cls.with_device_edits(packed)
                        if form == 20 or (form in (22, 27, 30) and self.sink is not None and hasattr(rv, "with_device_records")):
                            # --combined: the records behind them all; seq / qual stay on the device
                            packed = cls.with_device_records(packed, [hs.record_name(fn) for fn, _, _ in batch], hand_back=False)
                        if form == 22 or (form in (27, 30) and self.sumpart):   # --summary: the profile, behind whatever the call carries
                            packed = cls.with_device_profile(packed)
                        if form == 27 or (form == 30 and self.trim):   # --trim_q: the bounds last; the records above are then those of the trimmed reads
                            packed = cls.with_device_trim(packed, *self.trim)
                        if form == 30:                # --accuracy: the distances to the truth, behind everything else
                            fns = [fn for fn, _, _ in batch]
                            truth, toff, flags = self.accpart.block(fns, bundle["meta"][:, 1].tolist())
                            packed = cls.with_device_accuracy(packed, truth, toff)
                            self.acc_flags[id(batch)] = flags
                            if classes:               # --error_classes: behind the accuracy, on the same truth block
                                packed = cls.with_device_error_classes(packed)
                            if infix:                 # --infix: last, on the same truth block
                                packed = cls.with_device_infix(packed, self.infpart.strands)
                                if self.infpart.labels is not None:
                                    self.lab_truth[id(batch)] = (truth, toff)
                    if score:                         # --score: the labels of the call's reads go up with it, the block comes back last
                        found = bundle.get("labels") or self.scorepart.block([fn for fn, _, _ in batch], bundle["bases"], bundle["meta"][:, 1])
                        packed = cls.with_device_score(packed, found[0], phred_thresholds())
                        self.score_in[id(batch)] = found
        except Exception:
            packed = None
        if packed is None:
            route = "predict_many"                    # (one read: `predict_one`)
        self.inflight.append(self.eng.submit(self.run_batch, batch, packed, bundle, route))
        self.drain(self.n_eng + 1)

    def drain(self, limit):
        while len(self.inflight) > limit:
            self.inflight.popleft().result().result()

    def collect_finished(self, block):
        """Results of the pooled merges (main thread).  An entry is one read, or (fn is a list) all reads of a device call."""
        finishing = self.finishing
        while finishing and (block or finishing[0][0].done()):
            fut, fn, rt, fq = finishing.pop(0)
            many = isinstance(fn, list)
            try:
                res = fut.result()
                res = res if many else res[0]         # (`deliver` answers per read)
            except Exception as e:                    # the pool broke (a parser process died)
                res = [(0, repr(e))] * len(fn) if many else (0, repr(e))
            for (nb, err), f1, r1, q1 in (zip(res, fn, rt, fq) if many else [(res, fn, rt, fq)]):
                if err is None:
                    self.finished(f1, nb)
                else:
                    self.fallback(f1, r1, q1, err)

    def finish_batch(self, batch, calls):
        """Read by read: with a worker pool the merge + file write is a pool task (~20 KB per read), without one it happens here."""
        T = self.rv.T
        self.acc_flags.pop(id(batch), None)
        self.lab_truth.pop(id(batch), None)
        self.score_in.pop(id(batch), None)
        for (fn, rt, fq), c in zip(batch, calls):
            if isinstance(c, Exception):
                self.fallback(fn, rt, fq, c)
                continue
            try:
                if self.report:
                    self.rep_rows[fn] = report_rows(T, rt.bases, [len(np.asarray(rt.bases))], *c, self.want_qual, self.tie_eps)[0]
                if self.sumpart:
                    self.sum_rows[fn] = profile_rows(T, rt.bases, [len(np.asarray(rt.bases))], *c)[0]
                trim = None
                if self.trim:
                    tb, tl = _trim_rows_len(T, rt.bases, [len(np.asarray(rt.bases))], *c, *self.trim[:2])
                    self.trim_rows[fn], trim = (int(tl[0]), tb[0]), (tb, self.trim[2])
                if self.accpart:
                    self.acc_rows[fn] = self.accpart.host_rows(T, [fn], rt.bases, [len(np.asarray(rt.bases))], c[2], c[3])[0]
                if self.eclpart:
                    self.ecl_rows[fn] = self.eclpart.host_rows(T, [fn], rt.bases, [len(np.asarray(rt.bases))], c[2], c[3])[0]
                if self.infpart:
                    self.inf_rows[fn] = self.infpart.host_rows(T, [fn], rt.bases, [len(np.asarray(rt.bases))], c[2], c[3])[0]
                    if self.infpart.labels is not None:
                        self.lab_in[fn] = (hostlib.bases_u8(rt.bases), None)
                if self.scorepart:
                    self.score_rows[fn] = self.scorepart.host_rows(T, [fn], rt.bases, [len(np.asarray(rt.bases))], *c)[0]
                if self.edits_dir:
                    write_edits(self.edits_dir, fn, edit_rows(T, rt.bases, [len(np.asarray(rt.bases))], *c, self.want_qual)[0], self.want_qual)
                if self.pool is not None or self.sink is not None:
                    p1, p2, a1, a2 = c
                    qc = phred_chars(p1, p2, a1, a2) if self.want_qual and len(a1) else None
                    payload = ("calls", T, np.asarray(rt.bases), np.asarray(a1), np.asarray(a2), qc)
                    if self.sink is None:
                        task = self.pool.submit(deliver, self.spec, None, [fn], payload, self.native_threads, trim)
                        self.finishing.append((task, fn, rt, fq))
                        continue
                    (nb, err), = deliver(self.spec, self.sink, [fn], payload, trim=trim)      # the sink is this process' own: written here
                    if err is not None:
                        raise RuntimeError(err)
                    self.finished(fn, nb)
                    continue
                seq, qual = _finish_read(T, rt, *c, want_qual=self.want_qual)
                (nb, _), = deliver(self.args, None, [fn], ("text", seq, qual), trim=trim)
                self.finished(fn, nb)
            except Exception as e:
                self.fallback(fn, rt, fq, e)

    def stash_labels(self, fns, bases, ev_len, found=None):
        """--labels: every read's original bases - and, found = (labels, b_off, summary) of `device_labels`, its labels - until
        `finished` forms its line."""
        b, off = hostlib.bases_u8(bases), np.concatenate([[0], np.cumsum(np.asarray(ev_len, np.int64))])
        for r, fn in enumerate(fns):
            got = None if found is None else (found[0][int(found[1][r]):int(found[1][r + 1])], found[2][r])
            self.lab_in[fn] = (b[int(off[r]):int(off[r + 1])], got)

    def device_labels(self, reviser, batch, bundle, outs):
        """--labels on the device route: the labels of ALL reads of a form 33 call by ONE nrv_align_labels call, made on the engine's
        thread right behind the call's `end_packed_raw` - on a stream of its own, so the next call stays in flight.  The regions
        are the call's truth block, the bounds and the strand those `labels_plan` reads off the infix block; a read that gets no
        file goes up empty, with an empty region.  None where the engine cannot (the host stage aligns then)."""
        kept = self.lab_truth.pop(id(batch), None)
        flags = self.acc_flags.get(id(batch))
        if kept is None or flags is None or len(outs) not in (13, 14) or not hasattr(reviser, "align_labels_arrays"):
            return None
        truth, toff = kept
        ev_len = bundle["meta"][:, 1].astype(np.int64)
        rows = self.infpart.rows(outs[12], ev_len.tolist(), np.diff(outs[2]).tolist(), flags)
        plans = [labels_plan(v, n) for v, n in zip(rows, ev_len.tolist())]
        bases, off = hostlib.bases_u8(bundle["bases"]), np.concatenate([[0], np.cumsum(ev_len)])
        parts = [truth[int(toff[r]):int(toff[r + 1])] if p[0] == ACC_WITH_TRUTH else truth[:0] for r, p in enumerate(plans)]
        texts = [bases[int(off[r]):int(off[r + 1])] if p[0] == ACC_WITH_TRUTH else bases[:0] for r, p in enumerate(plans)]   # (the call refuses a read above its limit)
        a_off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
        b_off = np.concatenate([[0], np.cumsum([len(x) for x in texts])]).astype(np.int64)
        lab, summ = reviser.align_labels_arrays(np.concatenate(parts) if parts else truth[:0], a_off, np.concatenate(texts) if texts else bases[:0], b_off,
                                                [p[1] for p in plans], [p[2] for p in plans], [p[3] for p in plans])
        return lab, b_off, summ

    def finish_call(self, batch, bundle, outs, merged, labels=None):
        """ALL reads of a device call as one pool task: merge + record + file (nrvh_finish_bundle), or - merged, a --device_merge
        call that came back as revised reads - record + file alone (nrvh_write_records).  labels: what `device_labels` found."""
        try:
            fns, rts, fqs = map(list, zip(*batch))
            trim = None
            flags = self.acc_flags.pop(id(batch), None)
            self.lab_truth.pop(id(batch), None)
            found = self.score_in.pop(id(batch), None) or (bundle.get("labels") if bundle is not None else None)
            if merged:
                if len(outs) == 14:                   # a `with_device_score` call: the block was counted behind the merge, last output;
                    if self.scorepart and found is not None:   # blocks the call does not carry are None
                        self.scorepart.announce(fns, found[1])
                        self.score_rows.update(zip(fns, self.scorepart.rows(outs[13], found[1])))
                    outs = outs[:13] if outs[12] is not None else outs[:12] if outs[11] is not None else outs[:11]
                if len(outs) == 13:                   # a `with_device_infix` call: (..., accuracy, error classes | None, infix)
                    if self.infpart and flags is not None:
                        ev_len = bundle["meta"][:, 1].astype(np.int64)
                        self.inf_rows.update(zip(fns, self.infpart.rows(outs[12], ev_len.tolist(), np.diff(outs[2]).tolist(), flags)))
                        if self.infpart.labels is not None:
                            self.stash_labels(fns, bundle["bases"], ev_len, labels)
                    outs = outs[:12] if outs[11] is not None else outs[:11]
                if len(outs) == 12:                   # a `with_device_error_classes` call: the counts were found behind the distances, last output
                    if self.eclpart and flags is not None:
                        ev_len = bundle["meta"][:, 1].astype(np.int64)
                        self.ecl_rows.update(zip(fns, self.eclpart.rows(outs[11], ev_len.tolist(), np.diff(outs[2]).tolist(), flags)))
                    outs = outs[:11]
                if len(outs) == 11:                   # a `with_device_accuracy` call: the distances were found behind everything else, last output
                    if self.accpart and flags is not None:
                        ev_len = bundle["meta"][:, 1].astype(np.int64)
                        self.acc_rows.update(zip(fns, self.accpart.rows(outs[10], ev_len.tolist(), np.diff(outs[2]).tolist(), flags)))
                    outs = outs[:10]
                if len(outs) == 10:                   # a `with_device_trim` call: the bounds were found behind the merge, last output
                    if self.trim:
                        self.trim_rows.update(zip(fns, zip(np.diff(outs[2]).tolist(), outs[9])))
                        trim = (outs[9], self.trim[2])
                    outs = outs[:9]
                if len(outs) == 9:                    # a `with_device_profile` call: the rows were counted behind the merge, last output
                    if self.sumpart:
                        self.sum_rows.update(zip(fns, outs[8]))
                    outs = outs[:8]
                if self.report:                       # a `with_device_report` call: the rows were counted behind the merge
                    self.rep_rows.update(zip(fns, outs[3]))
                if self.edits_dir:                    # a `with_device_edits` call: the lists were compacted behind the merge
                    self.write_call_edits(fns, outs[4], outs[5])
                payload = ("records", outs[6], outs[7], outs[2]) if len(outs) == 8 and outs[6] is not None else \
                    ("merged", outs[0], outs[1] if self.want_qual else None, outs[2])
            else:
                p1, p2, a1, a2 = outs
                T, ev_len = self.rv.T, bundle["meta"][:, 1].astype(np.int64)
                if self.report:
                    self.rep_rows.update(zip(fns, report_rows(T, bundle["bases"], ev_len, p1, p2, a1, a2, self.want_qual, self.tie_eps)))
                if self.sumpart:
                    self.sum_rows.update(zip(fns, profile_rows(T, bundle["bases"], ev_len, p1, p2, a1, a2)))
                if self.trim:
                    tb, tl = _trim_rows_len(T, bundle["bases"], ev_len, p1, p2, a1, a2, *self.trim[:2])
                    self.trim_rows.update(zip(fns, zip(tl.tolist(), tb)))
                    trim = (tb, self.trim[2])
                if self.accpart:
                    self.acc_rows.update(zip(fns, self.accpart.host_rows(T, fns, bundle["bases"], ev_len.tolist(), a1, a2)))
                if self.eclpart:
                    self.ecl_rows.update(zip(fns, self.eclpart.host_rows(T, fns, bundle["bases"], ev_len.tolist(), a1, a2)))
                if self.infpart:
                    self.inf_rows.update(zip(fns, self.infpart.host_rows(T, fns, bundle["bases"], ev_len.tolist(), a1, a2)))
                    if self.infpart.labels is not None:
                        self.stash_labels(fns, bundle["bases"], ev_len)
                if self.scorepart:
                    self.score_rows.update(zip(fns, self.scorepart.host_rows(T, fns, bundle["bases"], ev_len.tolist(), p1, p2, a1, a2, found)))
                if self.edits_dir:
                    self.write_call_edits(fns, *edit_rows(T, bundle["bases"], ev_len, p1, p2, a1, a2, self.want_qual))
                qc = phred_chars(p1, p2, a1, a2) if self.want_qual and len(a1) else None
                payload = ("bundle", T, bundle["bases"], ev_len, a1, a2, qc)
            if self.sink is None:
                self.finishing.append((self.pool.submit(deliver, self.spec, None, fns, payload, True, trim), fns, rts, fqs))
                return
            for (nb, err), fn, rt, fq in zip(deliver(self.spec, self.sink, fns, payload, trim=trim), fns, rts, fqs):   # one append, here
                if err is None:
                    self.finished(fn, nb)
                else:
                    self.fallback(fn, rt, fq, err)
        except Exception as e:
            for fn, rt, fq in batch:
                self.fallback(fn, rt, fq, e)

    def write_call_edits(self, fns, edits, edit_off):
        """--edits for all reads of a device call: read r owns edits[edit_off[r]:edit_off[r + 1]]."""
        for r, fn in enumerate(fns):
            write_edits(self.edits_dir, fn, edits[int(edit_off[r]):int(edit_off[r + 1])], self.want_qual)

    def engine_time(self, t0, ti=None, t_call=None):
        """Books the engine time since t0; with a trace index, the end of that device call (begun at t_call, else t0) as well."""
        with self.stats_lock:
            self.stats["engine_s"] += time.perf_counter() - t0
        self.trace.call_end(ti, t0 if t_call is None else t_call)

    def collect(self, reviser, item):
        """Second half of a pipelined call: wait for it, hand its reads to the finisher; a failure is isolated read by read."""
        tk, batch, bundle, ti, t_begin = item
        t0 = time.perf_counter()
        try:
            outs = reviser.end_packed_raw(tk)
        except Exception:
            # the per-read retries are other entry points of the handle: first collect the call that was enqueued behind this one
            nxt = self.pending.pop(id(reviser), None)
            if nxt is not None:
                self.collect(reviser, nxt)
            calls = _predict_each(reviser, _bundle_reads(bundle))
            self.engine_time(t0)
            return self.fin.submit(self.finish_batch, batch, calls)      # (the finisher is one thread: behind nxt's hand-over)
        labels = None
        if self.infpart.labels is not None and _is_merged_ticket(tk):
            try:                                       # --labels: ONE call for the reads of this one, while the next is in flight
                labels = self.device_labels(reviser, batch, bundle, outs)
            except Exception as e:
                self.log(f"[！！！Warning] --labels: the device call failed ({e}); the host stage aligns these reads")
        self.engine_time(t0, ti, t_begin)
        return self.fin.submit(self.finish_call, batch, bundle, outs, _is_merged_ticket(tk), labels)

    def flush_pipeline(self):
        """Behind the last batch: whatever is still in flight."""
        last = self.done
        for rv in list(self.engines):
            item = self.pending.pop(id(rv), None)
            if item is not None:
                last = self.collect(rv, item)
        return last

    def run_batch(self, batch, packed, bundle, route):
        """One device call for the batch on an engine that is not inside a call (all have the same T, weights): the routes of
        `_route_batch` with their fall-throughs (its note [3]); merging and writing go to the finisher."""
        reviser = self.free.get()
        try:
            t0 = time.perf_counter()
            ti = self.trace.call_begin(t0)
            prev = self.pending.pop(id(reviser), None)
            if route == "pipelined":
                try:
                    tk = reviser.begin_packed_raw(packed)
                except Exception:
                    tk = None                             # e.g. a handle that could not grow its buffers: the synchronous path decides
                if tk is not None:
                    self.pending[id(reviser)] = (tk, batch, bundle, ti, t0)
                    self.engine_time(t0)
                    return self.collect(reviser, prev) if prev is not None else self.done
                route = "packed+finish_bundle"
            if prev is not None:                          # between a call's two halves nothing else may run on its handle
                self.collect(reviser, prev)
            packed = _host_merge_form(packed)             # every route below merges on the host
            rts = None
            try:
                if route in ("packed+finish_bundle", "packed sliced"):
                    p1, p2, a1, a2 = reviser.run_packed_raw(packed)
                    if route == "packed+finish_bundle":
                        self.engine_time(t0, ti)
                        return self.fin.submit(self.finish_call, batch, bundle, (p1, p2, a1, a2), False)
                    calls = _slice_calls((p1, p2, a1, a2), bundle["meta"][:, 1], reviser.T)
                else:                                     # predict_many / per-read: the reads as tensors
                    rts = _bundle_reads(bundle) if bundle is not None else [rt for _, rt, _ in batch]
                    calls = predict_many(reviser, rts, packed)
            except Exception:                             # isolate the failing read(s)
                calls = _predict_each(reviser, rts if rts is not None else
                                      _bundle_reads(bundle) if bundle is not None else [rt for _, rt, _ in batch])
            self.engine_time(t0, ti)
            return self.fin.submit(self.finish_batch, batch, calls)
        finally:
            self.free.put(reviser)


def process_files(args, files: Sequence[str], reviser, log: Callable[[str], None],
                  on_file: Optional[Callable[[str, bool], None]] = None, gpu_workers: int = 1,
                  core_share: Optional[int] = None, report_part: Optional[str] = None, combined_part: Optional[str] = None,
                  summary_part: Optional[str] = None, trim_part: Optional[str] = None, accuracy_part: Optional[str] = None,
                  errclass_part: Optional[str] = None, infix_part: Optional[str] = None, score_part: Optional[str] = None) -> dict:
    """Revise `files` (names inside args.fast5_base_dir) with one engine.  The host stage (HDF5 parsing, event collapse,
    statistics) runs --thread parser workers that stay a bounded number of reads ahead of the device: THREADS of this process
    inside libnanorev_host.so (at most kNativePoolMax), or PROCESSES on the Python host stage without it / with NRV_HOST_THREADS=0.
    on_file(fn, revised): called once per file when its output is final (revised, or the original
    basecalls after a failure; revised=False also for files that could not be parsed at all).
    gpu_workers: how many such calls run on this host at the same time (one per GPU, `run_workers`): the cores are
    SHARED, so each call's parser pool gets usable_cores() // gpu_workers of them - eight workers on a 16-core cgroup
    start 8 x 2 parser workers, not 8 x 16.  core_share: this call's cores, when the caller has already
    divided them (a GPU worker pinned to its NUMA slice: `_worker`).  report_part (--report): the file this call appends
    one line per read to, ahead of on_file (`ReportPart`).  combined_part (--combined): the part this call appends
    every read's record to INSTEAD of writing one file per read (`CombinedPart`, `deliver`).  summary_part (--summary): as
    report_part, for the summary's lines.  trim_part (--trim_log): as report_part, for the trim log's lines.  accuracy_part
    (--accuracy): as report_part, for the accuracy file's lines.  errclass_part (--error_classes): as accuracy_part, for that file's.  infix_part
    (--infix): the same for the infix file's.  score_part (--score): the same for the score file's."""
    import contextlib
    with contextlib.ExitStack() as stack:             # its exit ends the run's threads and undoes what `_FileRun._start` did
        run = _FileRun(stack, args, files, reviser, log, on_file, gpu_workers, core_share, report_part, combined_part, summary_part, trim_part, accuracy_part, errclass_part, infix_part, score_part)
        batch, nev = [], 0                            # unbundled reads are grouped into device calls of >= batch_events events
        for entries, bundle in run.results():
            bundled = []
            for k, (fn, rt, fq, err, dt) in enumerate(entries):
                run.stats["host_s"] += dt
                run.stats["reads"] += 1
                if rt is None:                        # could not be parsed at all: nothing to write
                    log(f"！！！[Error] fast5 file: {fn.split('.')[0]} {err}")
                    run.stats["failed"].append(fn)
                    run.report.add(fn, False, unrevised_row(0))
                    run.sumpart.add(fn, False, unrevised_profile(b""))
                    run.trimpart.add(fn, False, unrevised_trim(0))
                    run.accpart.add_unrevised(fn, b"")
                    run.eclpart.add_unrevised(fn, b"")
                    run.infpart.add_unrevised(fn, b"")
                    run.scorepart.add_unrevised(fn)
                    run.note(fn, False)
                elif err is not None:
                    run.fallback(fn, rt, fq, err)
                elif bundle is not None and k in bundle["idx"]:
                    bundled.append((fn, rt, fq))
                else:
                    batch.append((fn, rt, fq))       # unbundled reads (sequential mode, non-int16 signals)
                    nev += len(rt.feat_ev)
                    if nev >= run.batch_events:
                        run.submit(batch)
                        batch, nev = [], 0
            if bundled:
                run.submit(bundled, bundle)
            run.collect_finished(False)
        if batch:
            run.submit(batch)
        run.end()
    return run.summary()


def _default_factory(args, device: int):
    from .engine import Reviser
    p1, p2 = model_paths(args)
    return Reviser(load_model(p1), load_model(p2), device=device, batch=args.batch)


def _cpulist(text: str) -> List[int]:
    """'0-3,8,10-11' -> [0, 1, 2, 3, 8, 10, 11] (sysfs cpulist format)."""
    out = []
    for part in text.strip().split(","):
        if not part:
            continue
        a, _, b = part.partition("-")
        out.extend(range(int(a), int(b or a) + 1))
    return out


def gpu_local_cpus(device: int, sysfs: str = "/sys") -> Optional[List[int]]:
    """CPUs of the NUMA node HIP device `device` hangs on, or None when that cannot be told.  No HIP call: the KFD topology
    lists the GPU nodes (simd_count > 0) in the order the runtime enumerates them; *_VISIBLE_DEVICES given as a plain
    list of integers is honoured, any other form gives None."""
    try:
        vis = None
        for v in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            if os.environ.get(v, "") != "":
                if vis is not None:
                    return None                        # two layers of re-mapping: not guessed
                vis = [int(x) for x in os.environ[v].split(",")]
        if vis is not None:
            device = vis[device]
        base = os.path.join(sysfs, "class", "kfd", "kfd", "topology", "nodes")
        gpus = []
        for node in sorted(os.listdir(base), key=int):
            props = dict(ln.split()[:2] for ln in open(os.path.join(base, node, "properties")) if len(ln.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:
                gpus.append(props)
        pr = gpus[device]
        loc, dom = int(pr["location_id"]), int(pr.get("domain", "0"))
        bdf = "%04x:%02x:%02x.%d" % (dom, (loc >> 8) & 0xFF, (loc >> 3) & 0x1F, loc & 7)
        dev = os.path.join(sysfs, "bus", "pci", "devices", bdf)
        try:
            cpus = _cpulist(open(os.path.join(dev, "local_cpulist")).read())
        except OSError:
            cpus = []
        if not cpus:
            node = int(open(os.path.join(dev, "numa_node")).read())
            if node < 0:
                return None
            cpus = _cpulist(open(os.path.join(sysfs, "devices", "system", "node", f"node{node}", "cpulist")).read())
        return cpus or None
    except Exception:
        return None


def primary_threads(cpus: Sequence[int], sysfs: str = "/sys") -> List[int]:
    """One logical CPU per physical core: the lowest-numbered hardware thread of every core that has a thread in `cpus`.
    Two busy hardware threads of one core each run at ~60 % speed and are charged full CPU time: under a cgroup CPU quota
    the same host stage delivered 70-80 M or 115-125 M bases/s depending on where the scheduler happened to put the parser
    threads (r05, 2 x 64 cores x 2 threads, quota 16: scripts/host_scaling.py).  Without topology information: `cpus`."""
    keep, have = [], set(cpus)
    try:
        for c in sorted(have):
            sib = _cpulist(open(os.path.join(sysfs, "devices", "system", "cpu", f"cpu{c}", "topology", "thread_siblings_list")).read())
            if c == min(x for x in sib if x in have):
                keep.append(c)
    except Exception:
        return sorted(have)
    return keep or sorted(have)


def worker_cpus(rank: int, world: int, devices: Optional[Sequence[int]] = None, allowed: Optional[Sequence[int]] = None,
                sysfs: str = "/sys") -> Optional[List[int]]:
    """The cores GPU worker `rank` of `world` pins itself to (NanoReviser.py:203-219 leaves its Pool wherever the kernel
    puts it), or None = leave the affinity alone.  The cores this process may use - one hardware thread of each
    (`primary_threads`) - are divided so that each worker gets cores of ITS GPU's NUMA node (fast5 buffers, pinned staging memory and the HIP runtime's threads then sit next to the
    GPU's PCIe root); workers whose GPUs share a node share its cores evenly; without NUMA information the allowed
    cores are cut into `world` contiguous slices.  NRV_CPU_AFFINITY=0 turns it off; fewer than two cores per worker: off."""
    if os.environ.get("NRV_CPU_AFFINITY", "1") == "0" or world < 1:
        return None
    try:
        allowed = sorted(allowed if allowed is not None else os.sched_getaffinity(0))
    except AttributeError:
        return None
    if len(allowed) < 2 * world:
        return None
    prim = primary_threads(allowed, sysfs)             # one hardware thread per core, when that still leaves two per worker
    if len(prim) >= 2 * world:
        allowed = prim
    devices = list(devices) if devices is not None else list(range(world))
    aset = set(allowed)
    local = []
    for r in range(world):
        c = gpu_local_cpus(devices[r], sysfs)
        c = sorted(aset.intersection(c)) if c else None
        local.append(tuple(c) if c else None)
    if any(c is None for c in local):
        lo, hi = rank * len(allowed) // world, (rank + 1) * len(allowed) // world
        return allowed[lo:hi]
    mine = local[rank]
    peers = [r for r in range(world) if local[r] == mine]
    k, n = peers.index(rank), len(peers)
    part = list(mine[k * len(mine) // n:(k + 1) * len(mine) // n])
    return part if len(part) >= 2 else None


def probe_rename_rate(out_dir: str, pairs: int = 2000) -> Optional[float]:
    """create + write + rename pairs per second the OUTPUT directory's filesystem sustains (one output per read appears
    that way: write_read / nrvh_finish_read), measured on `pairs` small files in a scratch sub-directory.  Why: r05 found
    the sandbox's overlay root to cost ten times the system time of a real filesystem once a directory has seen a few
    thousand creates + renames - the same eight workers fed 68-78 M bases/s writing there and 120-131 M writing to tmpfs,
    i.e. less than eight GPUs consume.  None when the directory cannot be probed."""
    d = os.path.join(out_dir, f".nrv_probe_{os.getpid()}")
    try:
        os.makedirs(d, exist_ok=True)
        payload = b">probe\n" + b"ACGT" * 2048                 # ~8 KB: a typical record
        t0 = time.perf_counter()
        for i in range(pairs):
            tmp = os.path.join(d, f"p{i}.tmp")
            with open(tmp, "wb") as fp:
                fp.write(payload)
            os.replace(tmp, os.path.join(d, f"p{i}_out.fasta"))
        dt = time.perf_counter() - t0
        return pairs / max(dt, 1e-9)
    except OSError:
        return None
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)


def check_output_rate(args, world: int, n_reads: int, log=print) -> Optional[float]:
    """With several GPU workers and enough reads for it to matter: warn when the output directory cannot take the files the
    GPUs will produce.  One MI355X revises ~12.5 M bases/s = ~1600 reads of 8 k bases per second; ONE thread's probe rate
    must cover the whole run's share with a factor of two to spare (the finishers are a few threads per worker).
    NRV_OUTPUT_PROBE=0 turns the probe off, =1 forces it."""
    mode = os.environ.get("NRV_OUTPUT_PROBE", "")
    if getattr(args, "combined", None):               # --combined: no per-read creates, nothing to probe
        return None
    if mode == "0" or (mode != "1" and (world < 2 or n_reads < 4000)):
        return None
    rate = probe_rename_rate(args.output_dir)
    need = 1600.0 * world
    if rate is not None and rate < 2.0 * need:
        log(f"[！！！Warning] the output directory sustains {rate:.0f} file creations + renames per second (one thread, "
            f"2000 files); {world} GPU workers produce up to ~{need:.0f} reads per second.  The run will be bound by this "
            "filesystem, not by the GPUs: put -o on a local disk or a tmpfs (overlay / network filesystems are the usual cause).")
    return rate


def share_device() -> bool:
    """NRV_SHARE_DEVICE=1: worker rank r drives device r % device_count - a 1-GPU box rehearsing the N-worker command
    line with the real engine (bench.py --share-device, tests/test_gpu_multirank.py).  Never the default."""
    return os.environ.get("NRV_SHARE_DEVICE", "0") == "1"


def plan_splits(names: Sequence[str], sizes: Sequence[int], world: int, split_mb: float):
    """Which files are revised whole and which by window range.  A fast5 is split only when it would unbalance the run - it is
    larger than a worker's fair share of all bytes - and is worth it (above `split_mb` MB: every worker that holds a slice parses
    the whole file, ~3 ms per MB); it is cut into min(world, ceil(size / max(fair share, split_mb))) slices.  File size is the only
    thing known before parsing (~100 bytes per event).  Returns (units, unit_sizes): a unit is a file name or (file name, slice, slices)."""
    units, usz = [], []
    lim = int(split_mb * (1 << 20)) if split_mb and split_mb > 0 else 0
    fair = sum(int(x) for x in sizes) / max(1, world)
    cut = max(lim, int(fair))
    for fn, sz in zip(names, sizes):
        parts = min(world, -(-int(sz) // cut)) if lim and world > 1 and sz > cut else 1
        if parts <= 1:
            units.append(fn)
            usz.append(int(sz))
        else:
            for k in range(parts):
                units.append((fn, k, parts))
                usz.append(int(sz) // parts)
    return units, usz


def revise_part(args, reviser, fn: str, k: int, parts: int):
    """Slice k of `parts` of ONE read (BASELINE config 5): the read is parsed here (every worker that holds a
    slice parses the file: the host stage is cheap beside 100 k+ windows), `shard.split_read_windows` gives the event
    range [lo, hi) whose windows are exactly windows [lo, hi - T) of the read, and those events alone go to the device -
    whole raw samples, sliced starts / features, so every window is cut and computed as in the unsplit read.
    Returns (payload, error): the slice's calls (+ the original bases and the Fastq record with slice 0)."""
    job = (os.path.join(args.fast5_base_dir, fn), fn, args.basecall_group, args.basecall_subgroup, True)
    _, rt, fq, err, _ = _load_one(job)
    if rt is None or err is not None:
        return None, err or "unreadable"
    T, N = int(reviser.T), len(rt.feat_ev)
    lo, hi = split_read_windows(N, T, parts)[k]
    if hi > lo:
        if isinstance(rt, hs.RawReadTensors):
            p1, p2, a1, a2 = reviser.predict_reads_raw([rt.raw], [rt.starts[lo:hi]], [rt.feat_ev[lo:hi]], [rt.shift], [rt.scale])
        else:
            p1, p2, a1, a2 = reviser.predict_read(rt.sig_ev[lo:hi], rt.feat_ev[lo:hi])
    else:
        p1, p2 = np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32)
        a1 = a2 = np.zeros(0, np.int8)
    qc = phred_chars(p1, p2, a1, a2) if args.output_format == "fastq" and len(a1) else None
    out = {"T": T, "n_ev": N, "lo": lo, "a1": np.array(a1, np.int8), "a2": np.array(a2, np.int8), "qc": qc}
    if getattr(args, "report", None) or getattr(args, "edits", None) or getattr(args, "summary", None) or getattr(args, "score", None) \
            or getattr(args, "trim_q", None) is not None:   # the parent reports the read once its slices are merged: near-ties (and the edits' conf, the score's loss) need the rows
        out["p1"], out["p2"] = np.array(p1, np.float32), np.array(p2, np.float32)
    if k == 0:
        out["bases"], out["fq"] = np.asarray(rt.bases), fq
    return out, None


def _worker(rank: int, world: int, args, files: List[str], q, factory=None, parts=()):
    """One GPU worker.  Streams a ("file", rank, fn, revised) record through the queue as each file's output
    becomes final, so that the parent knows exactly which files are done should this process die; the slices of
    split reads (`parts`: (fn, slice, slices)) go first - they are the long poles - and come back as ("part", ...)."""
    try:
        cores_all = usable_cores()
        ndev = None
        if share_device():
            from .engine import device_count
            ndev = max(1, device_count())
        device = rank % ndev if ndev else rank
        cpus = worker_cpus(rank, world, [r % ndev if ndev else r for r in range(world)])
        share = None
        if cpus:
            try:
                os.sched_setaffinity(0, cpus)          # before the engine: the HIP runtime's threads inherit it
                share = max(1, min(len(cpus), cores_all // max(1, world)))
            except OSError:
                cpus = None
        made = []

        def make():                                   # one engine per call; process_files may call it from its engine thread
            made.append((factory or _default_factory)(args, device))
            return made[-1]
        rv = make() if parts else None                # slices need the engine now; whole files let it come up beside the parsers
        for fn, k, n in parts:
            try:
                payload, err = revise_part(args, rv, fn, k, n)
            except Exception as e:
                payload, err = None, repr(e)
            q.put(("part", rank, fn, k, payload, err))
        st = process_files(args, files, rv if rv is not None else make, print,
                           on_file=lambda fn, ok: q.put(("file", rank, fn, bool(ok))), gpu_workers=world, core_share=share,
                           report_part=report_part_path(args.report, rank) if getattr(args, "report", None) else None,
                           combined_part=combined_part_path(args.combined, rank) if getattr(args, "combined", None) else None,
                           summary_part=report_part_path(args.summary, rank) if getattr(args, "summary", None) else None,
                           trim_part=report_part_path(args.trim_log, rank) if getattr(args, "trim_log", None) else None,
                           accuracy_part=report_part_path(args.accuracy, rank) if getattr(args, "accuracy", None) else None,
                           errclass_part=report_part_path(args.error_classes, rank) if getattr(args, "error_classes", None) else None,
                           infix_part=report_part_path(args.infix, rank) if getattr(args, "infix", None) else None,
                           score_part=report_part_path(args.score, rank) if getattr(args, "score", None) else None)
        st["cpus"] = len(cpus) if cpus else 0
        for e in made:
            e.close()
        q.put(("done", rank, st, None))
    except BaseException as e:           # engine could not be created: loud, no silent fallback
        q.put(("done", rank, None, repr(e)))


def write_originals(args, files: Sequence[str], log: Callable[[str], None], report: Optional[ReportPart] = None,
                    sink: Optional[CombinedPart] = None, summary: Optional[ReportPart] = None,
                    trimlog: Optional[ReportPart] = None, accuracy: Optional["AccuracyPart"] = None,
                    score: Optional["ScorePart"] = None) -> List[str]:
    """The failure contract for reads whose WORKER is gone (NanoReviser.py:146-152 / :173-179): every
    file in `files` - the ones the dead worker never reported as final - gets its original basecalls
    written by this process (atomically, replacing whatever an earlier run left under that name).
    Returns the files handled (all of them count as failed reads)."""
    done = []
    for fn in files:
        done.append(fn)
        nw, text = 0, ""
        try:
            rd, fq = parse_read(os.path.join(args.fast5_base_dir, fn), args.basecall_group, args.basecall_subgroup)
            if getattr(args, "edits", None):         # unrevised: the header alone
                write_edits(args.edits, fn)
            if args.output_format == "fastq" and fq is not None:
                b, q = hs.trim_fastq(fq)
                deliver(args, sink, [fn], ("text", b, q))
            else:
                b = "".join(x.decode() for x in np.asarray(rd.bases).tolist())
                deliver(args, sink, [fn], ("text", b, None))
            nw, text = len(b), b
        except Exception as e:
            log(f"！！！[Error] fast5 file: {fn.split('.')[0]} {e!r}")
        if report is not None:
            report.add(fn, False, unrevised_row(nw))
        if summary is not None:
            summary.add(fn, False, unrevised_profile(text))
        if trimlog is not None:
            trimlog.add(fn, False, unrevised_trim(nw))
        if accuracy is not None:
            accuracy.add_unrevised(fn, text)
            if accuracy.classes is not None:
                accuracy.classes.add_unrevised(fn, text)
            if accuracy.infix is not None:
                accuracy.infix.add_unrevised(fn, text)
        if score is not None:
            score.add_unrevised(fn)
    return done


def finish_split_reads(args, split_fns: dict, parts_got: dict, log: Callable[[str], None], report: Optional[ReportPart] = None,
                       sink: Optional[CombinedPart] = None, summary: Optional[ReportPart] = None,
                       trimlog: Optional[ReportPart] = None, accuracy: Optional["AccuracyPart"] = None,
                       score: Optional["ScorePart"] = None):
    """Parent side of the split reads: the slices' calls in slice order are the read's calls (window i of slice k is
    window lo_k + i of the read), merged and written exactly as an unsplit read's.  A read with a slice missing (its
    worker died) or failed gets its original basecalls (NanoReviser.py:146-152).  Returns (bases written, failed names)."""
    spec, nb, failed = _OutSpec(args), 0, []
    for fn, n in sorted(split_fns.items()):
        got = parts_got.get(fn, {})
        pl = [got.get(k, (None, "slice never came back"))[0] for k in range(n)]
        err = next((e for k in range(n) for e in [got.get(k, (None, "slice never came back"))[1]] if e), None)
        ok = n > 0 and err is None and all(p is not None for p in pl) and "bases" in pl[0]
        if ok:                                         # every worker parsed the same file: same event count, slices abut
            T, N = pl[0]["T"], pl[0]["n_ev"]
            want = split_read_windows(N, T, n)
            ok = all(p["n_ev"] == N and p["T"] == T and p["lo"] == want[k][0] and len(p["a1"]) == max(want[k][1] - want[k][0] - T, 0)
                     for k, p in enumerate(pl))
            err = None if ok else "slices do not tile the read"
        if ok:
            a1, a2 = np.concatenate([p["a1"] for p in pl]), np.concatenate([p["a2"] for p in pl])
            qc = np.concatenate([p["qc"] if p["qc"] is not None else np.zeros(0, np.uint8) for p in pl]) \
                if args.output_format == "fastq" and len(a1) else None
            have_p = all("p1" in p for p in pl)
            if getattr(args, "edits", None):
                write_edits(args.edits, fn, hs.revision_edits(
                    hostlib.bases_u8(pl[0]["bases"]), [N], a1, a2,
                    np.concatenate([p["p1"] for p in pl]) if have_p else None, np.concatenate([p["p2"] for p in pl]) if have_p else None,
                    (qc if qc is not None else np.zeros(0, np.uint8)) if args.output_format == "fastq" else None, T)[0],
                    args.output_format == "fastq")
            trim, rule = None, trim_rule(args)
            if rule is not None and not have_p:
                ok, err = False, "the slices carry no rows to trim by"
            elif rule is not None:
                tb, tl = _trim_rows_len(T, pl[0]["bases"], [N], np.concatenate([p["p1"] for p in pl]),
                                        np.concatenate([p["p2"] for p in pl]), a1, a2, *rule[:2])
                trim = (tb, rule[2])
        if ok:
            (w, e2), = deliver(spec, sink, [fn], ("calls", T, pl[0]["bases"], a1, a2, qc), hostlib.load() is not None, trim)
            if e2 is None:
                nb += w
                if trim is not None and trimlog is not None:
                    trimlog.add(fn, True, trim_log_row(tl[0], tb[0], rule[2]))
                log(f"[p:::] {fn.split('.')[0]}_out.{args.output_format} was saved...... ({n} slices)" if trim is None or hs.trim_kept(tb, rule[2])[0]
                    else f"[p:::] {fn.split('.')[0]} was dropped by --trim_q...... ({n} slices)")
                if report is not None and report:
                    row = hs.revision_report(
                        hostlib.bases_u8(pl[0]["bases"]), [N], a1, a2,
                        np.concatenate([p["p1"] for p in pl]) if have_p else None, np.concatenate([p["p2"] for p in pl]) if have_p else None,
                        (qc if qc is not None else np.zeros(0, np.uint8)) if args.output_format == "fastq" else None, T,
                        float(getattr(args, "report_tie_eps", hs.REPORT_TIE_EPS)))[0]
                    report.add(fn, True, row)
                if accuracy is not None and accuracy:  # the slices are merged: the read's distances, here in the parent
                    accuracy.add(fn, True, accuracy.host_rows(T, [fn], pl[0]["bases"], [N], a1, a2)[0])
                    if accuracy.classes is not None:
                        accuracy.classes.add(fn, True, accuracy.classes.host_rows(T, [fn], pl[0]["bases"], [N], a1, a2)[0])
                if accuracy is not None and accuracy.infix is not None:
                    inf_row = accuracy.infix.host_rows(T, [fn], pl[0]["bases"], [N], a1, a2)[0]
                    accuracy.infix.add(fn, True, inf_row)
                    if accuracy.infix.labels is not None:
                        accuracy.infix.labels.add_read(fn, hostlib.bases_u8(pl[0]["bases"]), inf_row)
                if score is not None and score:        # the slices are merged: the read's score, here in the parent
                    score.add(fn, True, score.host_rows(T, [fn], pl[0]["bases"], [N],
                                                        np.concatenate([p["p1"] for p in pl]) if have_p else None,
                                                        np.concatenate([p["p2"] for p in pl]) if have_p else None, a1, a2)[0])
                if summary is not None and summary and have_p:
                    summary.add(fn, True, profile_rows(T, pl[0]["bases"], [N], np.concatenate([p["p1"] for p in pl]),
                                                       np.concatenate([p["p2"] for p in pl]), a1, a2)[0])
                continue
            err = e2
        log(f"[！！！Error] revising {fn.split('.')[0]}: {err}; writing the original basecalls")
        write_originals(args, [fn], log, report, sink, summary, trimlog, accuracy, score)
        failed.append(fn)
    return nb, failed


def run_workers(args, shards: List[List[str]], factory=None, poll_s: float = 0.2, part_shards=None, parts_out=None):
    """One worker process per GPU (NanoReviser.py:203-219 fans out the same way, one Pool task per
    file).  The parent never blocks on the result queue alone: a worker that dies hard - a HIP memory
    fault aborts the process, a segfault, the OOM killer - posts nothing, so liveness is polled next to
    the queue.  The other workers finish their own shards (reads are independent).
    Returns [(rank, stats or None, error or None, files)] with files = {fn: revised} for every file the
    worker reported final before it ended (file existence is never used as evidence).
    part_shards[r]: the (fn, slice, slices) units of worker r; their results are collected into parts_out
    {fn: {slice: (payload, error)}} for `finish_split_reads`."""
    import multiprocessing as mp
    import queue as _q
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world = len(shards)
    procs = [ctx.Process(target=_worker, args=(r, world, args, shards[r], q, factory,
                                               tuple(part_shards[r]) if part_shards else ())) for r in range(world)]
    for pr in procs:
        pr.start()
    res = {}
    files = [dict() for _ in range(world)]

    def drain(timeout):
        try:
            while True:
                msg = q.get(timeout=timeout)
                if msg[0] == "file":
                    files[msg[1]][msg[2]] = msg[3]
                elif msg[0] == "part":
                    if parts_out is not None:
                        parts_out.setdefault(msg[2], {})[msg[3]] = (msg[4], msg[5])
                else:
                    _, rank, st, err = msg
                    res[rank] = (rank, st, err)
                timeout = 0.0
        except _q.Empty:
            pass

    while len(res) < world:
        drain(poll_s)
        for r, pr in enumerate(procs):
            if r not in res and not pr.is_alive():
                drain(0.5)                            # its last messages may still be in the pipe
                if r not in res:
                    res[r] = (r, None, f"worker {r} died without reporting (exit code {pr.exitcode})")
    for pr in procs:
        pr.join(30)
        if pr.is_alive():
            pr.terminate()
    return [res[r] + (files[r],) for r in range(world)]


def main(argv: Optional[Sequence[str]] = None, reviser_factory=None, standalone: bool = False,
         worker_factory=None, world: Optional[int] = None) -> int:
    """standalone=True (the NanoReviser.py entry point): this process is only the command line, so the
    engine is loaded without importing torch first (~1.5 s of start-up).  Library callers keep the
    default: engine.load_library imports torch first so that one HIP runtime serves both.
    worker_factory (a picklable module-level callable (args, device) -> engine) and world replace the
    engine constructor and the device count in the multi-process path (tests).
    Returns 0, 2 (nothing could run) or 3 (a GPU worker was lost; its reads were written unrevised)."""
    args = get_args(argv)
    rc = 0
    if args.output_format not in ("fasta", "fastq"):
        print("[！！！Error] output_format must be fasta or fastq", file=sys.stderr)
        return 2
    model_paths(args)                     # existence check up front (NanoReviser.py:194)
    names = sorted(f for f in os.listdir(args.fast5_base_dir) if f.endswith(".fast5"))
    os.makedirs(args.output_dir, exist_ok=True)
    t0 = time.time()
    all_names = list(names)
    if args.report:                       # --report: every process appends to a part of its own, `merge_report` ends the run
        clear_report_parts(args.report)
        d = os.path.dirname(args.report)
        if d:
            os.makedirs(d, exist_ok=True)
    parent_report = ReportPart(report_part_path(args.report, "parent") if args.report else None)
    if args.summary:                      # --summary: parts and a parent-side merge as for --report
        clear_report_parts(args.summary)
        d = os.path.dirname(args.summary)
        if d:
            os.makedirs(d, exist_ok=True)
    parent_summary = ReportPart(report_part_path(args.summary, "parent") if args.summary else None, SUMMARY_COLS)
    sum_part0 = report_part_path(args.summary, 0) if args.summary else None
    trim_log = getattr(args, "trim_log", None)
    if trim_log:                          # --trim_log: parts and a parent-side merge as for --report
        clear_report_parts(trim_log)
        d = os.path.dirname(trim_log)
        if d:
            os.makedirs(d, exist_ok=True)
    parent_trim = ReportPart(report_part_path(trim_log, "parent") if trim_log else None, 4)
    trim_part0 = report_part_path(trim_log, 0) if trim_log else None
    parent_acc, acc_part0 = None, None
    if args.accuracy or args.infix:       # --accuracy (--infix without it: a part without a path): parts and a parent-side merge as for --report; the truth set is checked here
        try:
            truths = load_truth(args.truth)
        except (OSError, ValueError) as e:
            print(f"[！！！Error] {e}", file=sys.stderr)
            return 2
        if args.accuracy:
            clear_report_parts(args.accuracy)
            d = os.path.dirname(args.accuracy)
            if d:
                os.makedirs(d, exist_ok=True)
            acc_part0 = report_part_path(args.accuracy, 0)
        parent_acc = AccuracyPart(report_part_path(args.accuracy, "parent") if args.accuracy else None, truths, args.accuracy_max_len)
    ecl_part0 = None
    if args.error_classes:                # --error_classes: the same again, on the truth set just loaded
        clear_report_parts(args.error_classes)
        d = os.path.dirname(args.error_classes)
        if d:
            os.makedirs(d, exist_ok=True)
        parent_acc.classes = ErrclassPart(report_part_path(args.error_classes, "parent"), truths, args.accuracy_max_len)
        ecl_part0 = report_part_path(args.error_classes, 0)
    inf_part0 = None
    if args.infix:                        # --infix: the same again
        clear_report_parts(args.infix)
        d = os.path.dirname(args.infix)
        if d:
            os.makedirs(d, exist_ok=True)
        parent_acc.infix = InfixPart(report_part_path(args.infix, "parent"), truths, args.accuracy_max_len,
                                     1 if args.infix_strand == "forward" else 2)
        inf_part0 = report_part_path(args.infix, 0)
        if args.labels:                   # --labels: the files' directory; the parts of its index ride on the infix parts
            os.makedirs(args.labels, exist_ok=True)
            clear_report_parts(labels_index_path(args.labels))
            parent_acc.infix.labels = LabelsPart(args.labels, "parent", truths)
    if args.score:                        # --score: parts and a parent-side merge as for --report
        clear_report_parts(args.score)
        d = os.path.dirname(args.score)
        if d:
            os.makedirs(d, exist_ok=True)
    parent_score = ScorePart(report_part_path(args.score, "parent") if args.score else None, args.labels_from)
    score_part0 = report_part_path(args.score, 0) if args.score else None
    if args.combined:                     # --combined: a part per process too, `merge_combined` ends the run
        clear_combined_parts(args.combined)
    parent_sink = CombinedPart(combined_part_path(args.combined, "parent"), args.output_format == "fastq") if args.combined else None
    part0 = combined_part_path(args.combined, 0) if args.combined else None
    kept_failed, n_resumed = [], 0
    if args.resume:
        # A finished read is a non-empty <stem>_out.<fmt>: outputs only ever appear by rename of a complete temporary.
        # Reads an earlier run wrote UNREVISED (fallback after a lost GPU worker / an engine failure / a failed split-read
        # merge) are in its failed-reads file: they are taken out of `skip` and revised again - write_read replaces the
        # output atomically.  --resume_keep_failed: they stay as they are, stay listed, and the run returns 3.
        def done(f):
            try:
                return os.path.getsize(out_name(args.output_dir, f, args.output_format)) > 0
            except OSError:
                return False
        skip = {f for f in names if done(f)}
        try:
            with open(os.path.join(args.output_dir, args.failed_reads_filename)) as fp:
                earlier_failed = [ln.strip() for ln in fp if ln.strip() in skip]
        except OSError:
            earlier_failed = []
        if args.resume_keep_failed:
            kept_failed = earlier_failed
            if kept_failed:
                rc = 3
        else:
            skip -= set(earlier_failed)
        n_resumed, names = len(skip), [f for f in names if f not in skip]
        for f in sorted(skip):            # not revised by THIS run: reported as what lies on disk
            parent_report.add(f, False, unrevised_row(written_length(out_name(args.output_dir, f, args.output_format))))
            if args.summary:
                parent_summary.add(f, False, unrevised_profile(written_sequence(out_name(args.output_dir, f, args.output_format),
                                                                                  args.output_format == "fastq")))
        print(f"[s:::] --resume: {n_resumed} reads already have their output, {len(names)} to do"
              + (f" ({len(earlier_failed)} of them written unrevised by the earlier run"
                 + (", left as they are)" if args.resume_keep_failed else ", revised again)") if earlier_failed else ""))
    if reviser_factory is not None:       # in-process (tests / embedding): one engine, no sharding
        rv = reviser_factory(args, 0)
        stats = [process_files(args, names, rv, print, report_part=report_part_path(args.report, 0) if args.report else None,
                               combined_part=part0, summary_part=sum_part0, trim_part=trim_part0, accuracy_part=acc_part0, errclass_part=ecl_part0, infix_part=inf_part0, score_part=score_part0)]
    else:
        # the command line needs no torch: without it a process starts ~1.5 s sooner.  (engine.py imports
        # torch first only so that a LATER torch import in the same process finds one HIP runtime.)
        if standalone and "torch" not in sys.modules:
            os.environ.setdefault("NRV_NO_TORCH", "1")
        if world is not None:
            ndev = int(world)
        else:
            from .engine import device_count
            ndev = device_count()
        if ndev == 0:
            print("[！！！Error] no MI355X / HIP device visible: the reviser has no CPU path", file=sys.stderr)
            return 2
        # workers: --gpus (default: every visible device), never more than there are units of work; NRV_SHARE_DEVICE=1
        # (rehearsal) lets --gpus exceed the device count, worker r then drives device r % count
        want = min(args.gpus or ndev, args.gpus if (share_device() and args.gpus) else ndev)
        sizes = [os.path.getsize(os.path.join(args.fast5_base_dir, f)) for f in names]
        units, usz = plan_splits(names, sizes, want, args.split_reads_above)
        world = max(1, min(want, len(units)))
        parts = shard_reads(usz, world)
        check_output_rate(args, world, len(names), lambda m: print(m, file=sys.stderr))
        if world == 1:
            made = []

            def make():                               # runs in the engine thread, beside the parser pool's start-up
                made.append((worker_factory or _default_factory)(args, 0))
                return made[-1]                       # called once per engine (process_files: NRV_CLI_ENGINES)
            stats = [process_files(args, names, make, print, report_part=report_part_path(args.report, 0) if args.report else None,
                                   combined_part=part0, summary_part=sum_part0, trim_part=trim_part0, accuracy_part=acc_part0, errclass_part=ecl_part0, infix_part=inf_part0, score_part=score_part0)]
            for rv in made:
                rv.close()
        else:
            shards = [[units[i] for i in parts[r] if isinstance(units[i], str)] for r in range(world)]
            part_shards = [[units[i] for i in parts[r] if not isinstance(units[i], str)] for r in range(world)]
            split_fns = {u[0]: u[2] for u in units if not isinstance(u, str)}      # file -> slices
            parts_got = {}
            res = run_workers(args, shards, worker_factory, part_shards=part_shards, parts_out=parts_got)
            stats = [s for _, s, _, _ in res if s is not None]
            if split_fns:
                nb_split, failed_split = finish_split_reads(args, split_fns, parts_got, print, parent_report, parent_sink, parent_summary, parent_trim, parent_acc, parent_score)
                stats.append({"reads": len(split_fns), "bases": nb_split, "failed": failed_split, "host_s": 0.0, "engine_s": 0.0})
                if failed_split:
                    rc = 3
            for r, s_, e, final in res:
                if s_ is None:                        # the shard's files still get an output + a failed_reads entry
                    print(f"[！！！Error] GPU worker {r} failed: {e}; writing the original basecalls of its "
                          f"unfinished reads", file=sys.stderr)
                    # what the worker reported final stays (its failed reads keep their failed_reads entry);
                    # everything else - started or not, whatever lies on disk - is written unrevised
                    lost = write_originals(args, [f for f in shards[r] if f not in final], print, parent_report, parent_sink, parent_summary, parent_trim, parent_acc, parent_score)
                    lost += [f for f, ok in final.items() if not ok]
                    stats.append({"reads": len(shards[r]), "bases": 0, "failed": lost, "host_s": 0.0, "engine_s": 0.0})
                    rc = 3
    parent_report.close()
    if args.report:
        merge_report(args.report, all_names)
    parent_summary.close()
    if args.summary:
        merge_report(args.summary, all_names, table=SUMMARY_TABLE)
    parent_trim.close()
    if trim_log:
        merge_report(trim_log, all_names, table=TRIM_TABLE)
    if parent_acc is not None:
        parent_acc.close()
        if args.accuracy:
            merge_accuracy(args.accuracy, all_names)
        if parent_acc.infix is not None:
            parent_acc.infix.close()
            merge_infix(args.infix, all_names)
            if args.labels:
                merge_labels(args.labels, all_names)
        if parent_acc.classes is not None:
            parent_acc.classes.close()
            merge_error_classes(args.error_classes, all_names)
    parent_score.close()
    if args.score:
        merge_score(args.score, all_names)
    if args.combined:
        parent_sink.close()
        merge_combined(args.combined, args.output_format == "fastq")
    failed = kept_failed + [f for s in stats for f in s["failed"]]
    with open(os.path.join(args.output_dir, args.failed_reads_filename), "w") as fp:
        fp.write("".join(f + "\n" for f in failed))
    dt = time.time() - t0
    if not args.test_mode:
        nb = sum(s["bases"] for s in stats)
        print("[s:::] All subprocesses done.")
        print("[s:::] NanoReviser time consuming:%.2f seconds" % dt)
        print(f"[s:::] {sum(s['reads'] for s in stats)} reads, {nb} bases, {len(failed)} failed, "
              f"{nb / max(dt, 1e-9):.0f} bases/s end to end "
              f"(host stage {sum(s['host_s'] for s in stats):.1f} s summed over workers, "
              f"engine thread {sum(s['engine_s'] for s in stats):.1f} s)")
    return rc


if __name__ == "__main__":
    sys.exit(main(standalone=True))
