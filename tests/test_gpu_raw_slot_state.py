"""State an earlier raw-read call leaves in a slot of the handle (MI355X only, -m gpu): csrc/nrv_api.hip keeps per slot the merged
block's layout, where the results go, both threshold sets and the capacities of its buffers - a call must see nothing of the one
before it.  The two shortest fixture reads at T = 11, the shipped E. coli weights; everything BIT FOR BIT against the same packed
call run alone on a fresh handle:
  1. the forms 22 -> 20 -> 16 -> 14 -> 12 -> 9 -> 7 and back up on one handle, each with both reads and then with the first read
     only (a smaller call behind a larger one in the same slot: capacities unchanged, the old bytes behind it); FASTA and FASTQ,
     with and without device statistics alternate between the forms;
  2. two calls in flight with different forms - 22 and 7, then 16 without a report and 20 that hands back neither seq nor qual -
     ended in both orders;
  3. a form-22 call that trips the f16x2 range guard, then a clean form-12 and a clean form-7 call: one re-run, on the first;
  4. all of it once plainly and once on a handle created under NRV_POISON.
"""
import numpy as np
import pytest

from nanoreviser_amd import hoststage as hs

pytestmark = pytest.mark.gpu

POISON = 0x7FC00000
DOWN = [22, 20, 16, 14, 12, 9, 7]
# what each form carries besides its blocks: alternating, so that a call never inherits the quality or the statistics it needs
SPEC = {22: dict(fastq=True, stats=True), 20: dict(fastq=False, stats=False), 16: dict(fastq=True, stats=False),
        14: dict(fastq=False, stats=True), 12: dict(fastq=True, stats=False), 9: dict(stats=True), 7: dict()}


def _engine(monkeypatch, m1, m2, poison=False):
    from nanoreviser_amd.engine import Reviser
    monkeypatch.delenv("NRV_POISON", raising=False)
    if poison:
        monkeypatch.setenv("NRV_POISON", f"{POISON:08x}")
    for k in ("NRV_PRECISION", "NRV_COALESCE", "NRV_LANES", "NRV_RAW_STAGED"):
        monkeypatch.delenv(k, raising=False)
    rv = Reviser(m1, m2)
    monkeypatch.delenv("NRV_POISON", raising=False)
    return rv


@pytest.fixture(scope="module")
def short_reads(reads):
    """The two shortest fixture reads as (RawReadTensors, samples of the last base)."""
    out = []
    for k in reads.keys:
        _, rd, _ = reads(k)
        out.append((hs.read_tensors_raw(rd), int(rd.length[-1])))
    return sorted(out, key=lambda x: len(x[0].starts))[:2]


@pytest.fixture(scope="module")
def spiked(short_reads):
    """The spiked read of tests/test_gpu_device_profile.py::test_range_guard_rerun_counts_once behind a clean one: (arguments of
    pack_reads_raw, bases)."""
    other, _ = short_reads[0]
    rr, _ = short_reads[1]
    N = 1500
    starts = rr.starts[:N].copy()
    raw = rr.raw[: int(starts[-1]) + 60].copy()
    rng = np.random.default_rng(11)
    pos = rng.choice(len(raw), 30, replace=False)
    raw[pos] = rng.choice(np.array([-32768, 32767], np.int16), 30)
    sh, sc, c1, c2 = hs.stats_columns(raw, starts, 3)
    assert (32767 - sh) / sc > 250
    feat = rr.feat_ev[:N].copy()
    feat[:, 1], feat[:, 2] = c1, c2
    bases = np.concatenate([np.asarray(other.bases, "S1"), np.asarray(rr.bases, "S1")[:N]])
    return ([other.raw, raw], [other.starts, starts], [other.feat_ev, feat], [other.shift, sh], [other.scale, sc]), bases


def _bases(rrs):
    return np.concatenate([np.asarray(r.bases, "S1") for r in rrs]).view(np.uint8)


def _packed(rv, pairs, form, fastq=False, stats=False, report=True, hand_back=True):
    """A packed call of `form` (the length of its tuple) on the reads of `pairs`."""
    rrs, lds = [r for r, _ in pairs], [ld for _, ld in pairs]
    if stats:
        blind = []
        for r in rrs:
            f = r.feat_ev.copy()
            f[:, 1:3] = np.nan
            blind.append(f)
        p = rv.pack_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], blind, [np.nan] * len(rrs), [np.nan] * len(rrs), rv.T)
        p = rv.with_device_stats(p, lds, [1] * len(rrs))
    else:
        p = rv.pack_reads_raw([r.raw for r in rrs], [r.starts for r in rrs], [r.feat_ev for r in rrs], [r.shift for r in rrs],
                              [r.scale for r in rrs], rv.T)
    if form >= 12:
        p = rv.with_device_merge(p, _bases(rrs), fastq)
    if form >= 14 and report:
        p = rv.with_device_report(p)
    if form >= 16:
        p = rv.with_device_edits(p)
    if form >= 20:
        p = rv.with_device_records(p, [b"read_%d" % i for i in range(len(rrs))], hand_back=hand_back)
    if form >= 22:
        p = rv.with_device_profile(p)
    assert len(p) == form, (len(p), form)
    return p


def _packed_spiked(rv, spiked):
    args, bases = spiked
    p = rv.with_device_profile(rv.with_device_report(rv.with_device_merge(rv.pack_reads_raw(*args, rv.T), bases, True)))
    assert len(p) == 22
    return p


def _copy(out):
    return tuple(None if a is None else np.array(a, copy=True) for a in out)


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (what, i)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (what, i)


@pytest.fixture(scope="module")
def alone(species_models, short_reads, spiked):
    """key -> the result of that packed call run alone on a fresh handle (no NRV_POISON); computed once per key, never changed."""
    cache = {}

    def get(monkeypatch, key):
        if key not in cache:
            rv = _engine(monkeypatch, *species_models["ecoli"])
            if key == "spiked":
                cache[key] = _copy(rv.run_packed_raw(_packed_spiked(rv, spiked)))
                assert rv.saturated()[1] == 1
            else:
                form, n, opts = key
                cache[key] = _copy(rv.run_packed_raw(_packed(rv, short_reads[:n], form, **dict(opts))))
                assert rv.saturated() == (0, 0), key
            rv.close()
        return cache[key]
    return get


def _key(form, n, **opts):
    return form, n, tuple(sorted({**SPEC[form], **opts}.items()))


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
def test_a_call_sees_nothing_of_the_calls_before_it(species_models, short_reads, spiked, alone, monkeypatch, poison):
    rv = _engine(monkeypatch, *species_models["ecoli"], poison=poison)

    def pack(key):
        form, n, opts = key
        return _packed(rv, short_reads[:n], form, **dict(opts))

    # 1. descending, then ascending: both reads, then the first alone
    for form in DOWN + DOWN[-2::-1]:
        for n in (2, 1):
            key = _key(form, n)
            _same(rv.run_packed_raw(pack(key)), alone(monkeypatch, key), ("one handle", form, n))
    assert rv.saturated() == (0, 0)

    # 2. two calls in flight with different forms, ended in both orders
    pairs = ((_key(22, 2), _key(7, 2)), (_key(16, 2, report=False), _key(20, 2, hand_back=False)))
    for first in (0, 1):
        for ka, kb in pairs:
            t = [rv.begin_packed_raw(pack(ka)), rv.begin_packed_raw(pack(kb))]
            got = [None, None]
            for i in (first, 1 - first):
                got[i] = _copy(rv.end_packed_raw(t[i]))
            _same(got[0], alone(monkeypatch, ka), ("in flight", first, ka))
            _same(got[1], alone(monkeypatch, kb), ("in flight", first, kb))
    hb = alone(monkeypatch, _key(20, 2, hand_back=False))
    assert hb[0] is None and hb[1] is None and hb[6] is not None       # seq and qual stayed on the device, the records came back
    assert alone(monkeypatch, _key(16, 2, report=False))[3] is None
    assert rv.saturated() == (0, 0)

    # 3. the spiked read as a form-22 call, then two clean calls in the slot it re-ran in
    r0 = rv.saturated()[1]
    got = rv.run_packed_raw(_packed_spiked(rv, spiked))
    assert rv.saturated()[1] - r0 == 1
    _same(got, alone(monkeypatch, "spiked"), "spiked")
    for form in (12, 7):
        key = _key(form, 2)
        _same(rv.run_packed_raw(pack(key)), alone(monkeypatch, key), ("behind the re-run", form))
        assert rv.saturated()[1] - r0 == 1, form
    rv.close()
