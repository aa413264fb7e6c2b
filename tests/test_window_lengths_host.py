"""Window lengths other than the shipped 11, host side (CPU only): T = 1, 2, 12, 13, 32 (tests/window_cases.py says why these).

  1. the case builders became functions of T: at T = 11 every one of them returns exactly the arrays it returned before (sha256
     over each case's arrays, taken from the builders as they were when T was a module constant);
  2. the host definitions against the rule text at every T, on the T-derived cases: hoststage.revision_report == loop_report,
     revision_edits == loop_edits, emit_calls == revise_read / cli._merge_read read by read, the edit records replayed on the
     original bases give the merged read, pack_records == loop_records on the merged result; at T = 12 also on the call of
     257 * 256 + 3 events;
  3. nrvh_finish_bundle and nrvh_write_records (libnanorev_host.so) against the Python definitions at T = 1, 2, 12, 32: the
     bytes of every file (11 and 13 are held elsewhere);
  4. what engine.Reviser packs for a raw-read call at each T, through the echo engine and a recorder in the library's place:
     N - T windows, N + max(N - T, 0) characters, max(N - T, 0) edit records, the blob bound - each equal to what the definitions
     need in the worst case (every window two characters) - and N = T, N = T - 1: no window, nothing for the device to do.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

from nanoreviser_amd import cli, hostlib
from nanoreviser_amd import hoststage as hs
from nanoreviser_amd.engine import _RAW_FORMS, Reviser
from echo_engine import EchoEngine, HashEngine, PackedEcho
from edits_cases import carry_case, density_case, loop_edits, replay
from records_cases import carry_records_case, loop_records, names_for, parse_records, report_records_case
from report_cases import EV_LEN, TIE_EPS, ev_len_for, loop_report, report_case
from test_engine_marshalling import Recorder, _check_args
from window_cases import DENSITIES, T_SET, calls_cases, check_case_holds

# ---- 1. the T = 11 cases did not move ----------------------------------------------------------------------------------------------
PINS = {
    "report": "27d9171942d467b79293d336bcfbb2309469be90763fcd9fef4795907c107719",
    "density deletion": "b5fef2c35846cb8fe4bcd8fba92dd60dbec8cac1ce741b554ef02d29fba016ad",
    "density deletion 700": "574c59d122ff432f9715b2d236c15ce1126a82733a29fe2f76e6b632aea30d00",
    "density insertion": "3b96f251a1f9af2b8a6e31ebbf68af5955d3e7d1c885a936850cf76426814f96",
    "density insertion 700": "2f149608ceb68d417cd3d2dad2ccc0dd7af5d635b74495f96de8fb821d427acc",
    "density none": "a9d1a1a793f1c3467aeaa3bc01e757daf4051438d7c918b82177a9aa2a723861",
    "density none 700": "f0cb49f2ad5295fc63d687c524774207788e74e26bab53a453564a315fabf58b",
    "carry False": "e8e182441a020f170325738543c19655d3de26875a7610885cb9a2ed32e3d157",
    "carry True": "9c4eaeb27995f663dd072766cc436089a6b7af23decb451153644a5184cf9e94",
    "report records False": "a0c404325ffb07bdfc18318e5d6c5a35476f30734d657d291be374217385c655",
    "carry records False": "29f989ea4313f7ddecfcc6eafe6220eb7978eca5eda00f207b14979b65605286",
    "report records True": "906a26a54c6f8965c046b69f27e29d668000c300b2ff251a3b75e12e184dbf21",
    "carry records True": "a44dc3297b5d6886c80f50b436b27378ff2ee559982c8a7ccbf3743e02919ee0",
}


def case_digest(c):
    """sha256 over a case: every key in order, arrays by dtype, shape and bytes, names as bytes, integers, nested cases."""
    h = hashlib.sha256()
    for k in sorted(c):
        v = c[k]
        h.update(k.encode() + b"=")
        if isinstance(v, dict):
            h.update(case_digest(v).encode())
        elif isinstance(v, np.ndarray):
            h.update(f"{v.dtype.str}{v.shape}".encode() + np.ascontiguousarray(v).tobytes())
        elif isinstance(v, list):
            h.update(repr([bytes(x) for x in v]).encode())
        else:
            h.update(repr(v if v is None else int(v)).encode())
        h.update(b";")
    return h.hexdigest()


def _t11_cases(**kw):
    out = {"report": report_case(**kw)}
    for what in DENSITIES:
        out[f"density {what}"] = density_case(what, **kw)
        out[f"density {what} 700"] = density_case(what, ev_len=(700,), **kw)
    for d in (False, True):
        out[f"carry {d}"] = carry_case(d, **kw)
    for fq in (False, True):
        out[f"report records {fq}"] = report_records_case(fq, **kw)
        out[f"carry records {fq}"] = carry_records_case(fq, **kw)
    return out


@pytest.mark.parametrize("kw", [{}, {"T": 11}], ids=["default", "T=11"])
def test_the_cases_of_the_shipped_window_length_did_not_move(kw):
    got = {k: case_digest(c) for k, c in _t11_cases(**kw).items()}
    assert got == PINS
    assert ev_len_for(11) == EV_LEN == [0, 256, 0, 10, 11, 12, 1, 13, 255, 257, 600, 3 * 256 + 5, 0, 600, 0]
    assert case_digest(report_case(T=12)) != PINS["report"]              # (the digest does see T)


def test_report_case_lengths_follow_the_window_length():
    for T in T_SET:
        el = ev_len_for(T)
        assert el == [0, 256, 0, T - 1, T, T + 1, 1, T + 2, 255, 257, 600, 3 * 256 + 5, 0, 600, 0] and min(el) == 0
        c = report_case(T=T)
        assert c["ev_len"].tolist() == el and c["N"] == sum(el) and c["n"] == c["N"] - T == len(c["a1"])
        assert [x for x in el if x][0] == 256                            # the first non-empty read still ends on a tile edge
        first600 = sum(el[:10])
        assert el[10] == 600 and first600 + 10 < c["w0"] and c["w0"] + 32 < first600 + 600 - T - 10      # the planted windows: mid-read
        assert np.isnan(c["p1"][c["w0"] + 7, 2]) and c["p1"][c["w0"], 3] == 1


# ---- 2. the definitions against the rule text --------------------------------------------------------------------------------------
def _forms(c):
    return {"fastq": (c["p1"], c["p2"], c["qc"]), "rows": (c["p1"], c["p2"], None), "bare": (None, None, None)}


def _check_definitions(c, T, what, report_forms=("fastq", "rows", "bare")):
    ins = (c["bases"], c["ev_len"], c["a1"], c["a2"])
    for form, (p1, p2, qc) in _forms(c).items():
        if form in report_forms:
            got, want = hs.revision_report(*ins, p1, p2, qc, T, TIE_EPS), loop_report(*ins, p1, p2, qc, T, TIE_EPS)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (what, form, np.argwhere(got != want)[:8].tolist())
        edits, edit_off = hs.revision_edits(*ins, p1, p2, qc, T)
        blob, want_off = loop_edits(*ins, p1, p2, qc, T)
        assert edit_off.tolist() == want_off and edits.tobytes() == blob, (what, form)
    # the merge, read by read, and the edit records replayed on the original bases
    seq, qual, off = hs.emit_calls(*ins, c["qc"], T)
    fasta = hs.emit_calls(*ins, None, T)
    assert fasta[1] is None and np.array_equal(fasta[0], seq) and np.array_equal(fasta[2], off)
    edits, edit_off = hs.revision_edits(*ins, None, None, None, T)
    e0 = 0
    for r, L in enumerate(int(x) for x in c["ev_len"]):
        k = max(L - T, 0)
        b = c["bases"][e0:e0 + L].view("S1")
        s, q = cli._merge_read(T, b, c["a1"][e0:e0 + k], c["a2"][e0:e0 + k], c["qc"][e0:e0 + k])
        assert s == hs.revise_read(b, c["a1"][e0:e0 + k], c["a2"][e0:e0 + k], T), (what, r)
        assert seq[off[r]:off[r + 1]].tobytes().decode() == s and qual[off[r]:off[r + 1]].tobytes().decode() == q, (what, r, L)
        assert replay(b.tobytes(), edits[edit_off[r]:edit_off[r + 1]]) == s.encode(), (what, r, L)
        e0 += L
    assert off[-1] == len(seq) == len(qual)


@pytest.mark.parametrize("T", T_SET)
def test_definitions_equal_the_rule_text(T):
    for name, c in calls_cases(T).items():
        check_case_holds(name, c, T)
        _check_definitions(c, T, (T, name))


def test_definitions_on_the_carry_case_at_an_even_window_length():
    c = carry_case(False, T=12)
    assert c["N"] == 257 * 256 + 3 and c["n"] == c["N"] - 12
    _check_definitions(c, 12, "carry", report_forms=("bare",))


@pytest.mark.parametrize("T", T_SET)
def test_pack_records_equals_the_rule_text_on_the_merged_reads(T):
    for fastq in (False, True):
        c = report_records_case(fastq, T=T)
        assert c["calls"]["n"] == c["calls"]["N"] - T and (c["qual"] is not None) == fastq
        blob, rec_off = hs.pack_records(c["names"], c["seq"], c["qual"], c["off"])
        want, want_off = loop_records(c["names"], c["seq"], c["qual"], c["off"])
        assert blob.tobytes() == want and rec_off.tolist() == want_off
        recs = parse_records(blob, fastq)
        assert [len(s) for _, s, _ in recs] == np.diff(c["off"]).tolist() and [n for n, _, _ in recs] == c["names"]


# ---- 3. the native finishers -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_library():
    import __graft_entry__ as g
    g.build_host()
    assert hostlib.has_write_records(), "libnanorev_host.so lacks nrvh_write_records"


@pytest.mark.parametrize("fastq", [False, True])
@pytest.mark.parametrize("T", [1, 2, 12, 32])
def test_native_finishers_equal_the_python_definitions(host_library, tmp_path, T, fastq):
    c = calls_cases(T)["report"]
    R = len(c["ev_len"])
    qc = c["qc"] if fastq else None
    names = [f"read|||{r}|||w{T}.fast5" for r in range(R)]
    ext = "fastq" if fastq else "fasta"
    da, db = [str(tmp_path / f"a{r}.{ext}") for r in range(R)], [str(tmp_path / f"b{r}.{ext}") for r in range(R)]
    seq, qual, off = hs.emit_calls(c["bases"], c["ev_len"], c["a1"], c["a2"], qc, T)
    nw_a, st_a = hostlib.finish_bundle(c["bases"].view("S1"), c["ev_len"], c["a1"], c["a2"], T, qc, names, da, fastq)
    nw_b, st_b = hostlib.write_records(seq, qual, off, names, db, fastq)
    assert not st_a.any() and not st_b.any()
    assert np.array_equal(nw_a, np.diff(off)) and np.array_equal(nw_b, np.diff(off))
    e0 = 0
    for r, L in enumerate(int(x) for x in c["ev_len"]):
        k = max(L - T, 0)
        s, q = cli._merge_read(T, c["bases"][e0:e0 + L].view("S1"), c["a1"][e0:e0 + k], c["a2"][e0:e0 + k], None if qc is None else qc[e0:e0 + k])
        want = (hs.fastq_record(names[r], list(s), list(q)) if fastq else hs.fasta_record(names[r], list(s))).encode()
        assert open(da[r], "rb").read() == want, (T, r, L, "nrvh_finish_bundle")
        assert open(db[r], "rb").read() == want, (T, r, L, "nrvh_write_records")
        e0 += L


# ---- 4. marshalling ----------------------------------------------------------------------------------------------------------------
THR = np.linspace(0.3, 0.99, 39).astype(np.float32)
COLOR = {ord("A"): 250, ord("G"): 180, ord("T"): 100, ord("C"): 30}


def _reads(ev, seed=5):
    """Reads of ev[r] events whose feature column 0 is the base colour the echo engines read: (raws, starts, feats, bases uint8[N])."""
    rng = np.random.default_rng(seed)
    raws = [rng.integers(-500, 500, 10 * n).astype(np.int16) for n in ev]
    starts = [(np.arange(n) * 10).astype(np.int32) for n in ev]
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sum(ev)))].copy()
    feats, e0 = [], 0
    for n in ev:
        f = rng.random((n, 6), dtype=np.float32)
        f[:, 0] = np.array([COLOR[b] for b in bases[e0:e0 + n]], np.float32) / 300
        feats.append(f)
        e0 += n
    return raws, starts, feats, bases


def _reviser(T):
    rv = object.__new__(Reviser)
    rv._lib, rv._h, rv.T = Recorder(), C.c_void_p(0x1000), T
    return rv


def _full_form(p, bases, fastq, names):
    m = Reviser.with_device_merge(p, bases, fastq, THR if fastq else None)
    return Reviser.with_device_records(Reviser.with_device_edits(Reviser.with_device_report(m, TIE_EPS)), names)


def _check_capacities(p, T, N, nr, fastq, name_bytes):
    n = max(N - T, 0)
    assert len(p) == 20 and p[4] == nr and p[5] == N
    assert [x.shape for x in p[6]] == [(n, 6), (n, 5), (n,), (n,)]
    seq, qual, off = p[11]
    assert seq.size == max(N + n, 1) and (qual.size == seq.size if fastq else qual is None) and off.shape == (nr + 1,) and off.dtype == np.int64
    assert p[13].shape == (nr, 24) and p[13].dtype == np.uint64
    assert p[14].dtype == hs.EDIT_DTYPE and p[14].dtype.itemsize == 16 and p[14].size == max(n, 1) and p[15].shape == (nr + 1,)
    q = 2 if fastq else 1
    assert p[18].size == max(name_bytes + q * (N + n) + 3 * q * nr, 1) and p[19].shape == (nr + 1,) and int(p[17][-1]) == name_bytes


def _want_args(rv, p):
    """The C arguments of nrv_revise_reads_raw_records for a 20-tuple without device statistics (include/nanorev.h)."""
    raw, st, feat, descs, nr, N = p[:6]
    return [("is", rv._h), raw, int(raw.size), st, feat, N, ("is", descs), nr, None, None, p[9], p[10], p[11][0], p[11][1], p[11][2],
            float(p[12]), p[13], p[14].ctypes.data, p[15], p[16], p[17], p[18], p[19]]


@pytest.mark.parametrize("T", T_SET)
def test_packed_calls_have_the_sizes_the_definitions_need(T):
    ev = (T + 3, 0, max(T - 1, 0), T, T + 1, 40)
    raws, starts, feats, bases = _reads(ev)
    N, nr, n = sum(ev), len(ev), sum(ev) - T
    names = names_for(nr)
    nb = sum(len(x) for x in names)
    plain = Reviser.pack_reads_raw(raws, starts, feats, [1.0] * nr, [2.0] * nr, T)
    assert len(plain) == 7 and plain[4] == nr and plain[5] == N and plain[6][2].shape == (n,)
    assert [(d.ev_off, d.ev_len, d.raw_off, d.raw_len) for d in plain[3]] == \
        [(sum(ev[:r]), ev[r], 10 * sum(ev[:r]), 10 * ev[r]) for r in range(nr)]
    # the echo engine at this T says "the original base" in every window, the straddling ones included: the merge is the identity
    for eng in (PackedEcho(T=T), EchoEngine(T=T)):
        assert eng.T == T and EchoEngine.T == 11
    p1, p2, a1, a2 = PackedEcho(T=T).run_packed_raw(plain)
    assert len(a1) == n and np.array_equal(a2, a1 - 1)
    q1, q2, b1, b2 = EchoEngine(T=T).predict_read(np.zeros((N, 50), np.float32), plain[2])
    assert np.array_equal(a1, b1) and np.array_equal(p1, q1) and HashEngine(T=T).predict_read(None, plain[2])[2].shape == (n,)
    seq, _, off = hs.emit_calls(bases, ev, a1, a2, None, T)
    assert np.array_equal(seq, bases) and off.tolist() == np.concatenate([[0], np.cumsum(ev)]).tolist()
    assert not hs.revision_edits(bases, ev, a1, a2, None, None, None, T)[1].any()
    for fastq in (False, True):
        p = _full_form(plain, bases, fastq, names)
        _check_capacities(p, T, N, nr, fastq, nb)
        # the worst case of the definitions fits: every window two characters
        worst = hs.emit_calls(bases, ev, np.zeros(n, np.int8), np.ones(n, np.int8), np.full(n, 40, np.uint8) if fastq else None, T)
        assert len(worst[0]) <= p[11][0].size and len(hs.pack_records(names, *worst)[0]) <= p[18].size
        # ... and what reaches the library: the records entry point, 23 arguments, every array by its address
        rv = _reviser(T)
        for begin in (False, True):
            res = rv.begin_packed_raw(p) if begin else rv.run_packed_raw(p)
            name, args = rv._lib.calls[-1]
            assert name == _RAW_FORMS[20][1 if begin else 0]
            _check_args(args[:-1] if begin else args, _want_args(rv, p))
            if begin:
                res = rv.end_packed_raw(res)
            assert len(res) == 8 and res[2] is p[11][2] and res[3] is p[13] and res[5] is p[15] and res[7] is p[19]
    # one read: every window is the read's own, and the worst case fills the capacities exactly
    L = T + 5
    raws, starts, feats, bases = _reads((L,))
    one = Reviser.pack_reads_raw(raws, starts, feats, [1.0], [2.0], T)
    for fastq in (False, True):
        p = _full_form(one, bases, fastq, [b"r"])
        _check_capacities(p, T, L, 1, fastq, 1)
        worst = hs.emit_calls(bases, [L], np.zeros(5, np.int8), np.ones(5, np.int8), np.full(5, 40, np.uint8) if fastq else None, T)
        assert len(worst[0]) == p[11][0].size == L + 5 and len(hs.pack_records([b"r"], *worst)[0]) == p[18].size
        assert hs.revision_edits(bases, [L], np.zeros(5, np.int8), np.ones(5, np.int8), None, None, None, T)[1][-1] == p[14].size == 5


@pytest.mark.parametrize("T", T_SET)
def test_a_call_without_a_window_leaves_nothing_for_the_device(T):
    """N = T and N = T - 1 (none at T = 1): the library sees N <= T and output arrays for zero windows, which is the condition of
    its host branch (nrv_api.hip raw_begin: n = 0, nothing is enqueued); the merged block still has room for the reads as they are."""
    for N in {T, T - 1} - {0}:
        ev = (N - N // 2, 0, N // 2)
        raws, starts, feats, bases = _reads(ev)
        plain = Reviser.pack_reads_raw(raws, starts, feats, [1.0] * 3, [2.0] * 3, T)
        assert plain[5] == N <= T and [x.shape for x in plain[6]] == [(0, 6), (0, 5), (0,), (0,)]
        assert PackedEcho(T=T).run_packed_raw(plain)[2].shape == (0,)
        names = names_for(3)
        for fastq in (False, True):
            p = _full_form(plain, bases, fastq, names)
            _check_capacities(p, T, N, 3, fastq, sum(len(x) for x in names))
            assert p[11][0].size == N and p[14].size == 1
            z = np.zeros(0, np.int8)
            merged = hs.emit_calls(bases, ev, z, z, np.zeros(0, np.uint8) if fastq else None, T)
            assert np.array_equal(merged[0], bases) and (not fastq or merged[1].tobytes() == b"#" * N)
            assert len(hs.pack_records(names, *merged)[0]) == p[18].size        # no window: the bound is met exactly
            rv = _reviser(T)
            rv.run_packed_raw(p)
            (name, args), = rv._lib.calls
            assert name == "nrv_revise_reads_raw_records" and args[5] == N and args[5] - rv.T <= 0
            _check_args(args, _want_args(rv, p))
