"""What the one-shot entry points refuse, to the letter (MI355X only, -m gpu): nrv_merge_calls*, nrv_edit_distance, nrv_edit_classes,
nrv_infix_classes, nrv_align_labels, nrv_trim_reads and nrv_pack_records_trim.

For every refusal the C entry point is called directly - the Python wrappers in engine.py check some arguments themselves -, the
code is NRV_E_INVALID and nrv_last_error gives the WHOLE text below, compared with ==.  Every refusal is decided on the host, from
the scalars and the offset arrays alone, before any block is allocated and before any kernel is launched; the arrays a refused
call never reads are one element long here.  After each refusal the same handle answers one valid pair, "A" against "A"."""
import ctypes as C

import numpy as np
import pytest

from nanoreviser_amd import engine as E
from nanoreviser_amd import hoststage as hs

pytestmark = pytest.mark.gpu

NRV_E_INVALID = -1
TRUTH_TEXT = ": null truth / truth_off, offsets that do not ascend from 0, or a truth of 2^31 - 64 characters and more"
PAIR_TEXT = ": null sequences / offsets, offsets that do not ascend from 0, or a sequence of 2^31 - 64 characters and more"
INFIX_LEN_TEXT = "a truth region, or a read that has one, above NRV_INFIX_MAX_LEN = 2^21 - 1 characters"


def u8(x):
    return np.frombuffer(x, np.uint8).copy() if isinstance(x, bytes) else np.asarray(x, np.uint8)


def i64(*x):
    return np.asarray(x, np.int64)


@pytest.fixture(scope="module")
def rv(species_models):
    r = E.Reviser(*species_models["ecoli"])
    yield r
    r.close()


A = u8(b"A")
OUT = [np.zeros(4, np.int64) for _ in range(4)]


def _pair(**kw):
    """The arguments of a pair door for "A" against "A", some of them replaced."""
    d = dict(a=A, a_off=i64(0, 1), b=A, b_off=i64(0, 1), n=1)
    d.update(kw)
    return d


def _cases(T):
    """[(symbol, its C types, the arguments behind the handle, the text)]"""
    out = []
    # ---- the three pair doors
    for sym, types, outs, extra in (("nrv_edit_distance", E._EDIT_DISTANCE_T, 1, ()), ("nrv_edit_classes", E._EDIT_CLASSES_T, 2, ()),
                                    ("nrv_infix_classes", E._INFIX_CLASSES_T, 4, (0,))):
        def call(k=outs, extra=extra, **kw):
            d = _pair(**kw)
            return (d["a"], d["a_off"], d["b"], d["b_off"], d["n"]) + tuple(extra) + tuple(d.get("outs", OUT[:k]))
        out.append((sym, types, call(n=-1), sym + ": bad arguments"))
        out.append((sym, types, call(outs=OUT[:outs - 1] + [None]), sym + ": bad arguments"))
        bad_pair = sym + (": null sequences / offsets, or offsets that do not ascend from 0" if sym == "nrv_infix_classes" else PAIR_TEXT)
        out.append((sym, types, call(a_off=i64(1, 2)), bad_pair))
        out.append((sym, types, call(b_off=i64(0, -1)), bad_pair))
        out.append((sym, types, call(a_off=None), bad_pair))
        out.append((sym, types, call(b=None), bad_pair))
    big = np.full(E.INFIX_MAX_LEN + 1, ord("A"), np.uint8)
    out.append(("nrv_infix_classes", E._INFIX_CLASSES_T, (A, i64(0, 1), A, i64(0, 1), 1, 2) + tuple(OUT), "nrv_infix_classes: reverse must be 0 or 1"))
    out.append(("nrv_infix_classes", E._INFIX_CLASSES_T, (A, i64(1, 2), A, i64(0, 1), 1, -1) + tuple(OUT), "nrv_infix_classes: reverse must be 0 or 1"))
    out.append(("nrv_infix_classes", E._INFIX_CLASSES_T, (big, i64(0, big.size), A, i64(0, 1), 1, 0) + tuple(OUT), "nrv_infix_classes: " + INFIX_LEN_TEXT))
    out.append(("nrv_infix_classes", E._INFIX_CLASSES_T, (A, i64(0, 1), big, i64(0, big.size), 1, 1) + tuple(OUT), "nrv_infix_classes: " + INFIX_LEN_TEXT))
    # ---- nrv_align_labels
    LT = E._ALIGN_LABELS_T
    rev, st, en, lab, summ = u8([0]), i64(0), i64(1), np.zeros(70000, np.uint8), np.zeros((1, E.LABEL_COLS), np.int64)

    def labels(a=A, a_off=i64(0, 1), b=A, b_off=i64(0, 1), n=1, rev=rev, st=st, en=en, lab=lab, summ=summ):
        return (a, a_off, b, b_off, n, rev, st, en, lab, summ)
    out.append(("nrv_align_labels", LT, labels(n=-1), "nrv_align_labels: bad arguments"))
    out.append(("nrv_align_labels", LT, labels(summ=None), "nrv_align_labels: bad arguments"))
    out.append(("nrv_align_labels", LT, labels(rev=None), "nrv_align_labels: bad arguments"))
    seqs = "nrv_align_labels: null sequences / offsets / labels, or offsets that do not ascend from 0"
    out.append(("nrv_align_labels", LT, labels(a_off=i64(1, 2)), seqs))
    out.append(("nrv_align_labels", LT, labels(b_off=i64(0, -1)), seqs))
    out.append(("nrv_align_labels", LT, labels(lab=None), seqs))
    out.append(("nrv_align_labels", LT, labels(rev=u8([2])), "nrv_align_labels: reverse must be 0 or 1"))
    bounds = "nrv_align_labels: bounds outside the region (0 <= start <= end <= its length)"
    out.append(("nrv_align_labels", LT, labels(st=i64(-1)), bounds))
    out.append(("nrv_align_labels", LT, labels(st=i64(1), en=i64(0)), bounds))
    out.append(("nrv_align_labels", LT, labels(en=i64(2)), bounds))
    long_b = np.full(E.LABELS_MAX_LEN + 1, ord("A"), np.uint8)
    too_long = "nrv_align_labels: a read, or an end - start, above NRV_LABELS_MAX_LEN = 65536 characters"
    out.append(("nrv_align_labels", LT, labels(b=long_b, b_off=i64(0, long_b.size)), too_long))
    out.append(("nrv_align_labels", LT, labels(a=long_b, a_off=i64(0, long_b.size), en=i64(long_b.size)), too_long))
    # ---- nrv_trim_reads
    TT = E._TRIM_READS_T
    q1, tr = u8(b"I"), np.zeros((2, 2), np.int64)
    out.append(("nrv_trim_reads", TT, (q1, i64(0, 1), -1, 10, 1, tr), "nrv_trim_reads: bad arguments"))
    out.append(("nrv_trim_reads", TT, (q1, None, 1, 10, 1, tr), "nrv_trim_reads: bad arguments"))
    out.append(("nrv_trim_reads", TT, (q1, i64(1, 2), 1, 10, 1, tr), "nrv_trim_reads: bad arguments"))
    out.append(("nrv_trim_reads", TT, (q1, i64(0, 1), 1, 10, 1, None), "nrv_trim_reads: bad arguments"))
    for Q, W in ((0, 1), (41, 1), (10, 0), (10, 65)):
        out.append(("nrv_trim_reads", TT, (q1, i64(0, 1), 1, Q, W, tr), "nrv_trim_reads: Q must be in 1 .. 40 and W in 1 .. 64"))
    out.append(("nrv_trim_reads", TT, (q1, i64(0, 1, 0), 2, 10, 1, tr), "nrv_trim_reads: off does not ascend"))
    out.append(("nrv_trim_reads", TT, (None, i64(0, 1), 1, 10, 1, tr), "nrv_trim_reads: null qual"))
    # ---- nrv_pack_records_trim: (seq, qual, off, n_reads, names, name_off, trim, min_len, blob, rec_off)
    PT = E._PACK_RECORDS_TRIM_T
    blob, roff, nm = np.zeros(64, np.uint8), np.zeros(3, np.int64), u8(b"r")

    def pack(seq=A, qual=None, off=i64(0, 1), n=1, names=nm, name_off=i64(0, 1), trim=None, min_len=0, blob=blob, roff=roff):
        return (seq, qual, off, n, names, name_off, trim, min_len, blob, roff)
    out.append(("nrv_pack_records_trim", PT, pack(n=-1), "nrv_pack_records: bad arguments"))
    out.append(("nrv_pack_records_trim", PT, pack(off=None), "nrv_pack_records: bad arguments"))
    out.append(("nrv_pack_records_trim", PT, pack(roff=None), "nrv_pack_records: bad arguments"))
    out.append(("nrv_pack_records_trim", PT, pack(off=i64(1, 2)), "nrv_pack_records: bad arguments"))
    out.append(("nrv_pack_records_trim", PT, pack(off=i64(0, 1, 0), n=2), "nrv_pack_records: off does not ascend"))
    out.append(("nrv_pack_records_trim", PT, pack(trim=i64(0, 1), min_len=-1), "nrv_pack_records_trim: negative min_len"))
    for t in (i64(-1, 1), i64(1, 0), i64(0, 2)):
        out.append(("nrv_pack_records_trim", PT, pack(trim=t), "nrv_pack_records_trim: a trim outside its read"))
    names_text = "nrv_pack_records: null names / name_off, or offsets that do not ascend from 0"
    out.append(("nrv_pack_records_trim", PT, pack(name_off=None), names_text))
    out.append(("nrv_pack_records_trim", PT, pack(name_off=i64(1, 2)), names_text))
    out.append(("nrv_pack_records_trim", PT, pack(names=None), names_text))
    out.append(("nrv_pack_records_trim", PT, pack(seq=None), "nrv_pack_records: null seq / blob"))
    out.append(("nrv_pack_records_trim", PT, pack(blob=None), "nrv_pack_records: null seq / blob"))
    out.append(("nrv_pack_records_trim", PT, pack(off=i64(0, 1 << 32)), "nrv_pack_records: records of 4 GiB and more in one call"))
    # ---- nrv_merge_calls*: (bases, ev_len, n_reads, a1, a2, p1, p2, n_win, q_thr, seq, qual, off) and the blocks behind them
    MT = E._MERGE_CALLS_T
    N, n = T + 2, 2
    bases, a12, seq, off = np.full(N, ord("A"), np.uint8), np.zeros(n, np.int8), np.zeros(N + n, np.uint8), np.zeros(2, np.int64)
    p1, p2, thr = np.zeros((n, 6), np.float32), np.zeros((n, 5), np.float32), np.zeros(39, np.float32)

    def merge(ev_len=i64(N), n_reads=1, n_win=n, off=off, p=(None, None)):
        return (bases, ev_len, n_reads, a12, a12) + tuple(p) + (n_win, None, seq, None, off)
    out.append(("nrv_merge_calls", MT, merge(n_reads=-1), "nrv_merge_calls: bad arguments"))
    out.append(("nrv_merge_calls", MT, merge(n_win=-1), "nrv_merge_calls: bad arguments"))
    out.append(("nrv_merge_calls", MT, merge(off=None), "nrv_merge_calls: bad arguments"))
    out.append(("nrv_merge_calls", MT, merge(ev_len=None), "nrv_merge_calls: bad arguments"))
    out.append(("nrv_merge_calls", MT, merge(ev_len=i64(-1)), "nrv_merge_calls: a negative read length (or 2^31 events and more)"))
    out.append(("nrv_merge_calls", MT, merge(ev_len=i64(1 << 30, 1 << 30), n_reads=2),
                "nrv_merge_calls: a negative read length (or 2^31 events and more)"))
    out.append(("nrv_merge_calls", MT, merge(n_win=n + 1), "nrv_merge_calls: n_win is not sum(ev_len) - T, or a null array"))
    trim_t = MT + E._TRIM[0] + E._RECORDS[0]
    trim_blk = (thr, 10, 10, 1, np.zeros((1, 2), np.int64))
    out.append(("nrv_merge_calls_trim", trim_t, merge(p=(p1, p2)) + trim_blk + (nm, i64(1, 2), blob, roff),
                "nrv_merge_calls_trim: null names / name_off, or offsets that do not ascend from 0"))
    out.append(("nrv_merge_calls_trim", trim_t, merge(p=(p1, p2)) + trim_blk + (nm, i64(0, 1), None, roff),
                "nrv_merge_calls_trim: null blob (or records of 4 GiB and more)"))
    blocks = {"nrv_merge_calls_accuracy": np.zeros((1, E.ACCURACY_COLS), np.uint64), "nrv_merge_calls_errclass": np.zeros((1, E.ERRCLASS_COLS), np.uint64),
              "nrv_merge_calls_infix": np.zeros((1, E.INFIX_COLS), np.uint64)}
    for sym, blk in blocks.items():
        infix = sym == "nrv_merge_calls_infix"
        types = MT + (E._TRUTH[0][:2] + E._INFIX[0] if infix else E._TRUTH[0])
        tail = (lambda s=2, blk=blk: (s, blk)) if infix else (lambda s=2, blk=blk: (blk,))
        out.append((sym, types, merge() + (A, i64(1, 2)) + tail(), sym + TRUTH_TEXT))
        out.append((sym, types, merge() + (None, i64(0, 1)) + tail(), sym + TRUTH_TEXT))
        out.append((sym, types, merge(ev_len=i64(1 << 30), n_win=(1 << 30) - T) + (None, i64(0, 0)) + tail(), sym + ": 2^30 events and more"))
    sym, types = "nrv_merge_calls_infix", MT + E._TRUTH[0][:2] + E._INFIX[0]
    strands = sym + ": strands must be 1 or 2, and no truth region or read that has one above NRV_INFIX_MAX_LEN = 2^21 - 1 characters"
    out.append((sym, types, merge() + (A, i64(0, 1), 3, blocks[sym]), strands))
    out.append((sym, types, merge() + (big, i64(0, big.size), 2, blocks[sym]), strands))
    out.append(("nrv_merge_calls_edits", MT + E._REPORT[0] + E._EDITS[0], merge() + (0.05, None, None, np.zeros(2, np.int64)),
                "nrv_merge_calls_edits: null edits"))
    return out


def _valid_pair(rv, sym):
    """One valid pair on the same handle, through the door that refused where it takes pairs: "A" against "A"."""
    if sym == "nrv_edit_classes":
        assert [x.tolist() for x in rv.edit_classes_offsets(A, [0, 1], A, [0, 1])] == [[0], [1]]
    elif sym == "nrv_infix_classes":
        assert [x.tolist() for x in rv.infix_classes_offsets(A, [0, 1], A, [0, 1])] == [[0], [1], [0], [1]]
    elif sym == "nrv_align_labels":
        lab, summ = rv.align_labels_arrays(A, [0, 1], A, [0, 1], [0], [0], [1])
        want_lab, want_sum = hs.align_labels(b"A", b"A", 0, 0, 1)
        assert lab.tolist() == np.asarray(want_lab).tolist() == [5] and summ.tolist() == [np.asarray(want_sum).tolist()]
    else:
        assert rv.edit_distance_offsets(A, [0, 1], A, [0, 1]).tolist() == [0]


def test_every_refusal_word_for_word_and_the_handle_stays_usable(rv):
    cases = _cases(rv.T)
    assert {c[0] for c in cases} >= {"nrv_merge_calls", "nrv_edit_distance", "nrv_edit_classes", "nrv_infix_classes", "nrv_align_labels",
                                     "nrv_trim_reads", "nrv_pack_records_trim"}
    for sym, types, args, text in cases:
        assert len(args) + 1 == len(types), (sym, len(args), len(types))
        rc = getattr(rv._lib, sym)(*E._marshal((rv._h,) + tuple(args), types))
        got = rv._lib.nrv_last_error(rv._h).decode()
        assert rc == NRV_E_INVALID and got == text, (sym, rc, got, text)
        _valid_pair(rv, sym)


def test_a_null_handle_is_refused_without_a_text(rv):
    for sym, types, args in (("nrv_edit_distance", E._EDIT_DISTANCE_T, (A, i64(0, 1), A, i64(0, 1), 1, OUT[0])),
                             ("nrv_trim_reads", E._TRIM_READS_T, (A, i64(0, 1), 1, 10, 1, np.zeros((1, 2), np.int64)))):
        assert getattr(rv._lib, sym)(*E._marshal((C.c_void_p(),) + args, types)) == NRV_E_INVALID
    _valid_pair(rv, "nrv_edit_distance")
