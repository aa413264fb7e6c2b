"""The window lengths other than the shipped 11 and the calls cases built at them, shared by tests/test_window_lengths_host.py
and tests/test_gpu_window_lengths.py (no test here).

T_SET: 1 (o = (T - 1) // 2 = 0, no halo, a window is one event), 2 (the smallest even T: o = 0, one trailing event kept), 12 (the
even neighbour of the shipped T), 13 (the benchmark's T) and 32 (the maximum: the largest halo, most reads shorter than a window).
`calls_cases(T)` is built once per T and handed out read-only: `report_cases.report_case(T=T)` and the three
`edits_cases.density_case` on `density_lens(T)`, which puts reads of T - 1, T and T + 1 events between the long ones.
`case_facts` counts what a case holds by the definitions; `check_case_holds` asserts that a pass cannot come from an empty case."""
import functools

import numpy as np

from edits_cases import density_case
from report_cases import report_case

T_SET = (1, 2, 12, 13, 32)
DENSITIES = ("deletion", "insertion", "none")


def density_lens(T):
    """`density_case`'s default lengths with reads of T - 1, T (no window) and T + 1 (one window) events in the middle."""
    return (0, 300, max(T - 1, 0), T, T + 1, 0, T + 2, 256, 700, 0)


def _frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


@functools.lru_cache(maxsize=None)
def calls_cases(T):
    out = {"report": _frozen(report_case(T=T))}
    for what in DENSITIES:
        out[what] = _frozen(density_case(what, ev_len=density_lens(T), T=T))
    return out


def case_facts(c, T):
    """What a calls case holds, by the host definitions: events, windows of the call, windows that straddle two reads (or lie
    in a read shorter than T + 1) and belong to nobody, edit records, and the merge's per-window character counts that occur."""
    from nanoreviser_amd import hoststage as hs
    el = np.asarray(c["ev_len"], np.int64)
    owned = int(np.maximum(el - T, 0).sum())
    ev_off = np.cumsum(el) - el
    o = (T - 1) // 2
    counts = set()
    for e0, L in zip(ev_off.tolist(), el.tolist()):
        k = max(L - T, 0)
        if k:
            counts |= set(hs.merge_calls(c["bases"][e0 + o:e0 + o + k], c["a1"][e0:e0 + k], c["a2"][e0:e0 + k])[2].tolist())
    edits = int(hs.revision_edits(c["bases"], el, c["a1"], c["a2"], None, None, None, T)[1][-1])
    return {"events": int(el.sum()), "windows": int(len(c["a1"])), "straddling": int(len(c["a1"])) - owned, "owned": owned,
            "edits": edits, "counts": counts}


def check_case_holds(name, c, T):
    """A pass cannot come from an empty case.  Every case: reads of T - 1, T and T + 1 events, windows that belong to nobody,
    n = N - T.  `report`: every class of the merge (0, 1 and 2 characters per window) and a non-zero edit total.  A density
    case holds ONE class by construction - all windows deleted (0), inserted (2) or confirmed (1) - so there the edit total
    is every owned window (deletion, insertion) or none at all."""
    f = case_facts(c, T)
    lens = set(np.asarray(c["ev_len"]).tolist())
    assert {max(T - 1, 0), T, T + 1} <= lens, (name, T, sorted(lens))
    assert f["windows"] == f["events"] - T > 0 and f["owned"] > 0, (name, T, f)
    assert f["straddling"] > 0, (name, T, f)
    if name == "report":
        assert f["counts"] == {0, 1, 2} and 0 < f["edits"] < f["owned"], (name, T, f)
    else:
        assert f["counts"] == {{"deletion": 0, "insertion": 2, "none": 1}[name]}, (name, T, f)
        assert f["edits"] == (0 if name == "none" else f["owned"]), (name, T, f)
    return f
