"""The twelve row doors of nrv_fit_* and the growth of the set (MI355X only, -m gpu).  No fit kernel runs here: the doors copy,
nrv_fit_add_reads_raw runs the frozen backbone and the depth's gather.
  1. every depth x every door: at its own depth a door round-trips bytes, sub-ranges too; at every other depth it is refused with
     NRV_E_INVALID and nrv_last_error is the WHOLE expected string, built here from (name, phrase, suffix) by the rule
     include/nanorev.h states; a call over the depth's row cap is refused with the whole cap message, through the door and
     through nrv_fit_add_reads_raw;
  2. growth: rows added before the set grows keep their bytes, and the rows added after it are what a handle gathers that sized
     the set for all of them in one call; once more on a poisoned handle."""
import os

import numpy as np
import pytest

from nanoreviser_amd.engine import NrvError
from test_gpu_fullfit import ENV, PATTERNS
from test_gpu_fullfit import short_reads  # noqa: F401 (a fixture)
from test_gpu_headfit import _labels_for, _pack

pytestmark = pytest.mark.gpu

T = 11
# name -> (NRV_FIT_* code, the "rows are ..." phrase, the door suffix, the trailing shapes of the door's float arrays)
DEPTHS = {
    "tail": (0, "main_out values", "", ((6 * T,), (6 * T,))),
    "head": (1, "lstm4 outputs", "_head", ((T, 128), (T, 128))),
    "lstm4": (4, "BatchNorm'd lstm3 outputs", "_lstm4", ((T, 256), (T, 256))),
    "lstm3": (8, "lstm3's inputs", "_lstm3", ((T, 192), (T, 192))),
    "signal": (16, "lstm2 outputs and samples", "_signal", ((T, 128), (T, 128), (T, 50))),
    "full": (32, "samples and read features", "_full", ((T, 50), (T, 6))),
}
CAP = 8


def other_depth(door, kind, at):
    """nrv_last_error of the `kind` ("set" / "get") door of depth `door` called while the set is at depth `at`."""
    who = f"nrv_fit_{kind}_rows{DEPTHS[door][2]}"
    if at == "tail" and kind == "set":
        return f"{who}: the set is at tail depth (call nrv_fit_set_depth(NRV_FIT_{door.upper()}) on an empty set first)"
    return f"{who}: the set is at {at} depth (rows are {DEPTHS[at][1]}: nrv_fit_{kind}_rows{DEPTHS[at][2]})"


def cap_words(depth):
    return "(NRV_FIT_MAX_ROWS)" if depth == "tail" else f"at {depth} depth (NRV_FIT_MAX_{depth.upper()}_ROWS)"


def _rows(depth, n, seed):
    rng = np.random.default_rng(seed)
    xs = tuple(rng.normal(0, 1, (n,) + sh).astype(np.float32) for sh in DEPTHS[depth][3])
    return xs + (rng.integers(0, 6, n).astype(np.uint8), rng.integers(0, 5, n).astype(np.uint8))


def _set(rv, depth, rows):
    getattr(rv, "fit_set_rows" + DEPTHS[depth][2])(*rows)


def _get(rv, depth, *rng):
    return getattr(rv, "fit_get_rows" + DEPTHS[depth][2])(*rng)


def _same(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


@pytest.fixture(scope="module")
def capped(species_models):
    """One f32 handle whose six row caps are all 8."""
    from nanoreviser_amd.engine import Reviser
    caps = [k for k in ENV if k.startswith("NRV_FIT_MAX_")]
    assert len(caps) == 6
    saved = {k: os.environ.pop(k, None) for k in ENV}
    try:
        os.environ.update({k: str(CAP) for k in caps})
        m1, m2 = species_models["ecoli"]
        rv = Reviser(m1.with_window(T), m2.with_window(T), precision="f32")
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    yield rv
    rv.close()


@pytest.mark.parametrize("at", list(DEPTHS))
def test_every_door_at_every_depth(capped, short_reads, at):  # noqa: F811
    rv = capped
    lib, h = rv._lib, rv._h

    def refused(call, want):
        with pytest.raises(NrvError) as e:
            call()
        err = lib.nrv_last_error(h).decode()
        assert e.value.code == -1 and err == want, (err, want)

    rv.fit_reset()
    rv.fit_set_depth(at)
    assert rv.fit_depth() == DEPTHS[at][0] and rv.fit_count() == 0
    for seed, door in enumerate(DEPTHS):
        rows = _rows(door, 3, 100 * DEPTHS[at][0] + seed)
        if door != at:
            refused(lambda: _set(rv, door, rows), other_depth(door, "set", at))
            refused(lambda: _get(rv, door), other_depth(door, "get", at))
            refused(lambda: _get(rv, door, 0, 0), other_depth(door, "get", at))
            continue
        _set(rv, door, rows)
        assert rv.fit_count() == 3
        assert _same(_get(rv, door), rows)
        assert _same(_get(rv, door, 1, 2), tuple(a[1:3] for a in rows))
    # one row over the cap: refused whole, by the depth's own words, and the set keeps its rows
    who = "nrv_fit_set_rows" + DEPTHS[at][2]
    refused(lambda: _set(rv, at, _rows(at, CAP + 1, 7)), f"{who}: more rows than the cap of the training set {cap_words(at)}")
    labels = _labels_for(short_reads)
    refused(lambda: rv.fit_add_packed(_pack(rv, short_reads), labels),
            f"nrv_fit_add_reads_raw: the call would pass the row cap of the training set {cap_words(at)}")
    assert rv.fit_count() == 3
    rv.fit_reset()


def _engine(monkeypatch, species_models, depth, poison):
    from nanoreviser_amd.engine import Reviser
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if poison is not None:
        monkeypatch.setenv("NRV_POISON", f"{PATTERNS[poison]:08x}")
    m1, m2 = species_models["ecoli"]
    rv = Reviser(m1.with_window(T), m2.with_window(T), precision="f32")
    monkeypatch.delenv("NRV_POISON", raising=False)
    rv.fit_set_depth(depth)
    return rv


@pytest.mark.parametrize("poison", [None, "qnan"])
@pytest.mark.parametrize("depth", list(DEPTHS))
def test_rows_survive_the_growth_of_the_set(species_models, short_reads, monkeypatch, depth, poison):  # noqa: F811
    labels = _labels_for(short_reads)
    cuts = np.cumsum([0] + [len(r.starts) for r in short_reads])
    rv = _engine(monkeypatch, species_models, depth, poison)
    try:
        n_first = rv.fit_add_packed(_pack(rv, short_reads[:1]), labels[:cuts[1]])
        assert n_first == rv.fit_count() > 0
        before = _get(rv, depth)
        cap = max(1024, n_first)                           # what the first call's reserve left
        used = 1
        while rv.fit_count() <= cap and used < len(short_reads):
            assert rv.fit_add_packed(_pack(rv, short_reads[used:used + 1]), labels[cuts[used]:cuts[used + 1]]) > 0
            used += 1
        n = rv.fit_count()
        assert n > cap                                     # the set has grown with rows in it
        after = _get(rv, depth)
    finally:
        rv.close()
    assert _same(tuple(a[:n_first] for a in after), before)
    fresh = _engine(monkeypatch, species_models, depth, poison)
    try:
        assert fresh.fit_add_packed(_pack(fresh, short_reads[:used]), labels[:cuts[used]]) == n
        want = _get(fresh, depth)
    finally:
        fresh.close()
    assert _same(tuple(a[n_first:] for a in after), tuple(a[n_first:] for a in want))
    assert _same(after, want)
    assert all(np.isfinite(a).all() for a in after[:-2])
