"""What engine.Reviser hands to the C library for every packed form of a raw-read call and for the stand-alone merge calls
(CPU only, no library: `_lib` is a recorder).  Pins, per form and per half, the symbol, the number of arguments, the address
behind every pointer, NULL where the form has no statistics / no quality, the scalars, and what comes back - tickets included.
"""
import ctypes as C

import numpy as np
import pytest

from nanoreviser_amd.engine import NrvError, Reviser

T = 11
REPORT_SYMBOLS = ("nrv_revise_reads_raw_report", "nrv_revise_reads_raw_report_begin", "nrv_merge_calls_report")


class Recorder:
    """Stands where the CDLL stands: any nrv_* attribute is a function that stores (name, args) and returns 0."""

    def __init__(self, report=True):
        self.calls, self.report = [], report

    def __getattr__(self, name):
        if not name.startswith("nrv_") or (name in REPORT_SYMBOLS and not self.report):
            raise AttributeError(name)

        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


def _reviser(report=True):
    rv = object.__new__(Reviser)
    rv._lib, rv._h, rv.T = Recorder(report), C.c_void_p(0x1000), T
    return rv


def _addr(p):
    if p is None:
        return None
    return C.addressof(p) if isinstance(p, C.Array) else C.cast(p, C.c_void_p).value


def _check_args(args, want):
    """want: an array (a pointer to its data), None (NULL), an int / float (a scalar, plain or as a ctypes value) or
    ("is", obj) for an object handed over as it is."""
    assert len(args) == len(want)
    for i, (a, w) in enumerate(zip(args, want)):
        if isinstance(w, tuple):
            assert a is w[1], i
        elif w is None:
            assert a is None, i
        elif isinstance(w, np.ndarray):
            assert _addr(a) == w.ctypes.data, i
        elif isinstance(w, float):
            assert isinstance(a, C.c_float) and a.value == np.float32(w), i
        else:
            assert isinstance(a, int) and not isinstance(a, bool) and a == w, i


@pytest.fixture(scope="module")
def plain():
    rng = np.random.default_rng(7)
    ev = (7, 9)                                                          # 16 events, T = 11: 5 windows
    raws = [rng.integers(-500, 500, 10 * n).astype(np.int16) for n in ev]
    starts = [(np.arange(n) * 10).astype(np.int32) for n in ev]
    feats = [rng.random((n, 6), dtype=np.float32) for n in ev]
    packed = Reviser.pack_reads_raw(raws, starts, feats, [1.5, 2.5], [3.0, 4.0], T)
    assert len(packed) == 7 and packed[4] == 2 and packed[5] == 16 and packed[6][2].shape == (5,)
    return packed


THR = np.linspace(0.3, 0.99, 39).astype(np.float32)
BASES = np.frombuffer(b"ACGTACGTACGTACGT", np.uint8).copy()


def _forms(plain):
    """name -> packed tuple: the four forms, the merge forms with and without statistics and quality."""
    stats = Reviser.with_device_stats(plain, np.array([4, 6], np.int32), np.array([1, 0], np.uint8))
    out = {"7": plain, "9": stats}
    for tag, base in (("", plain), ("s", stats)):
        for fq in (False, True):
            m = Reviser.with_device_merge(base, BASES, fq, THR if fq else None)
            m[11][2][-1] = 3                                             # as if the call had produced three bases
            out[f"12{tag}{'q' if fq else ''}"] = m
            out[f"14{tag}{'q' if fq else ''}"] = Reviser.with_device_report(m, 2.5e-4)
    return out


def _want_args(rv, p):
    raw, st, feat, descs, nr, N, calls = p[:7]
    want = [("is", rv._h), raw, int(raw.size), st, feat, 16, ("is", descs), 2]
    if len(p) == 7:
        return want + list(calls)
    if len(p) == 9:
        return want + [p[7], p[8]] + list(calls)
    want += [p[7], p[8], p[9], p[10]] + list(p[11])                      # None stays None: no statistics, no quality
    return want + ([float(p[12]), p[13]] if len(p) == 14 else [])


SYMBOL = {7: ("nrv_predict_reads_raw", "nrv_reads_raw_begin"), 9: ("nrv_predict_reads_raw_stats", "nrv_reads_raw_stats_begin"),
          12: ("nrv_revise_reads_raw", "nrv_revise_reads_raw_begin"),
          14: ("nrv_revise_reads_raw_report", "nrv_revise_reads_raw_report_begin")}
FORMS = ["7", "9", "12", "12q", "12s", "12sq", "14", "14q", "14s", "14sq"]


def _check_result(p, res):
    if len(p) in (7, 9):
        assert len(res) == 4 and all(a is b for a, b in zip(res, p[6]))
        return
    seq, qual, off = p[11]
    assert len(res) == (3 if len(p) == 12 else 4)
    assert res[0].shape == (3,) and np.shares_memory(res[0], seq) and res[2] is off
    if qual is None:
        assert res[1] is None
    else:
        assert res[1].shape == (3,) and np.shares_memory(res[1], qual)
    if len(p) == 14:
        assert res[3] is p[13] and res[3].shape == (2, 24) and res[3].dtype == np.uint64


@pytest.mark.parametrize("form", FORMS)
def test_run_packed_raw(plain, form):
    p = _forms(plain)[form]
    if len(p) >= 12:
        assert (p[7] is None) == (p[8] is None) == ("s" not in form) and (p[10] is None) == (p[11][1] is None) == ("q" not in form)
    rv = _reviser()
    res = rv.run_packed_raw(p)
    (name, args), = rv._lib.calls
    assert name == SYMBOL[len(p)][0]
    _check_args(args, _want_args(rv, p))
    _check_result(p, res)


@pytest.mark.parametrize("form", FORMS)
def test_begin_and_end_packed_raw(plain, form):
    p = _forms(plain)[form]
    rv = _reviser()
    tk = rv.begin_packed_raw(p)
    (name, args), = rv._lib.calls
    assert name == SYMBOL[len(p)][1]
    _check_args(args[:-1], _want_args(rv, p))                            # the ticket pointer comes last
    assert isinstance(tk, tuple) and tk[0] == -1                         # (the recorder writes no ticket)
    if len(p) in (7, 9):
        assert len(tk) == 2 and len(tk[1]) == 4 and all(a is b for a, b in zip(tk[1], p[6]))
    else:
        assert len(tk) == 3 and tk[2] == "merged" and isinstance(tk[1], tuple)
        assert all(a is b for a, b in zip(tk[1], p[11])) and len(tk[1]) == (3 if len(p) == 12 else 4)
        assert len(p) == 12 or tk[1][3] is p[13]
    res = rv.end_packed_raw(tk)
    name, args = rv._lib.calls[1]
    assert name == "nrv_reads_raw_end" and len(args) == 2 and args[0] is rv._h and args[1] == -1
    _check_result(p, res)


def test_report_form_needs_the_report_symbols(plain):
    forms = _forms(plain)
    rv = _reviser(report=False)
    for half in (rv.run_packed_raw, rv.begin_packed_raw):
        with pytest.raises((NrvError, AttributeError)):                  # loud either way: the engine's error, or the missing symbol's
            half(forms["14q"])
        half(forms["12q"])                                               # the other forms do not need them
    assert [n for n, _ in rv._lib.calls] == ["nrv_revise_reads_raw", "nrv_revise_reads_raw_begin"]
    with pytest.raises(NrvError) as e:
        rv.merge_calls_report_device(BASES, [7, 9], np.zeros(5, np.int8), np.zeros(5, np.int8))
    assert e.value.code == -1
    assert len(rv.merge_calls_device(BASES, [7, 9], np.zeros(5, np.int8), np.zeros(5, np.int8))) == 3


@pytest.mark.parametrize("report", [False, True])
@pytest.mark.parametrize("quality", ["none", "p", "p+thr"])
def test_merge_calls(report, quality):
    rng = np.random.default_rng(3)
    el = np.array([7, 9], np.int64)
    a1, a2 = rng.integers(0, 6, 5).astype(np.int8), rng.integers(0, 5, 5).astype(np.int8)
    p1, p2 = rng.random((5, 6), dtype=np.float32), rng.random((5, 5), dtype=np.float32)
    kw = {"none": {}, "p": {"p1": p1, "p2": p2}, "p+thr": {"p1": p1, "p2": p2, "q_thr": THR}}[quality]
    rv = _reviser()
    res = rv.merge_calls_report_device(BASES, el, a1, a2, tie_eps=1e-3, **kw) if report else rv.merge_calls_device(BASES, el, a1, a2, **kw)
    (name, args), = rv._lib.calls
    assert name == ("nrv_merge_calls_report" if report else "nrv_merge_calls") and len(args) == (15 if report else 13)
    with_p = quality == "p+thr" or (report and quality == "p")           # the plain merge takes p1 / p2 only with q_thr
    _check_args(args[:10], [("is", rv._h), BASES, el, 2, a1, a2, p1 if with_p else None, p2 if with_p else None, 5,
                            THR if quality == "p+thr" else None])
    seq, qual, off = args[10:13]
    assert seq is not None and off is not None and (qual is None) == (quality != "p+thr")
    assert res[0].shape == (0,) and res[2].shape == (3,) and res[2].dtype == np.int64 and _addr(off) == res[2].ctypes.data
    assert (res[1] is None) == (quality != "p+thr") and len(res) == (4 if report else 3)
    if report:
        assert isinstance(args[13], C.c_float) and args[13].value == np.float32(1e-3)
        assert res[3].shape == (2, 24) and res[3].dtype == np.uint64 and _addr(args[14]) == res[3].ctypes.data


def test_merge_calls_refuse_what_does_not_match():
    rv = _reviser()
    a = np.zeros(5, np.int8)
    p1, p2 = np.zeros((5, 6), np.float32), np.zeros((5, 5), np.float32)
    for call in (rv.merge_calls_device, rv.merge_calls_report_device):
        with pytest.raises(ValueError):
            call(BASES, [7, 8], a, a)                                    # ev_len does not sum to the bases
        with pytest.raises(ValueError):
            call(BASES, [7, 9], a, a[:4])
        with pytest.raises(ValueError):
            call(BASES, [7, 9], a, a, p1, p2, THR[:38])
        with pytest.raises(ValueError):
            call(BASES, [7, 9], a, a, p1[:4], p2, THR)
    with pytest.raises(ValueError):
        rv.merge_calls_report_device(BASES, [7, 9], a, a, p1[:4], p2)    # checked without q_thr as well
    with pytest.raises(ValueError):
        rv.merge_calls_report_device(BASES, [7, 9], a, a, q_thr=THR)     # q_thr needs p1 / p2
    assert not rv._lib.calls
