"""Caller-owned memory and streams: the helpers of tests/test_caller_cases_host.py and tests/test_gpu_caller_contract.py (no test
here).

A BAND is one buffer laid out as [front guard | payload | back guard]: the payload is the array an entry point is handed, the
guards are what a caller who keeps one buffer for many calls has on both sides of it.  Each guard is GUARD_ROWS = 64 rows of the
array - the largest row granularity of any kernel (ROWS = 64 in the Bi-LSTM kernels), so the furthest a tile-shaped overrun could
reach - and the front guard is `offset_elems` elements longer, which moves the payload off the 16-byte grid: the buffer itself
starts on a multiple of `align` bytes, and 64 rows of any array here are a multiple of 64 bytes, so the payload's address modulo
16 is `offset_elems * itemsize` modulo 16.  `banded` builds a band in torch memory (any device), `banded_np` the same in NumPy;
`guards`, `fill_guards` and `guards_hold` take either.

ALIGNMENTS: the element offsets of the six arrays of a call.  0 is the aligned case; 1, 2, 3 put the float inputs at byte offsets
4, 8 and 12 modulo 16, p1 / p2 at 4 modulo 8 (an odd number of floats) and a1 / a2 at odd byte addresses.

The inputs: `windows(T)` / `events(T)` are the E. coli cases of tests/test_gpu_lstm4_resident.py (synth_windows(129, T, seed = 8100
+ T)) for T = 1 and 13, T = 32 with T32_SEED, each with a DECOY of the same shape from another seed: valid windows that give
other answers.  `reference` holds the fp64 arbiter, the f32 floor and the C port's outputs for them, computed once.

`slow_producer` is the stream-order instrument: matrix products that keep a stream busy, then the copies that put the real inputs
where the decoy was, then an event.  A call that did not wait for the producer read the decoy."""
import functools

import numpy as np

GUARD_ROWS = 64
GUARD_BYTE = 0xA5
MODES = ("f16x2", "bf16x3", "f32")
NS = (1, 33, 129)          # one row; a tile of one row behind a full one; the first row of a third 64-row workgroup
TS = (1, 13, 32)
N_MAX = max(NS)
T32_SEED = 8132            # the first seed tried: tests/test_caller_cases_host.py holds the C oracle to the bar on it
BIG = 3.0e38               # finite, and its square is not
ARRAYS = ("sig", "feat", "p1", "p2", "a1", "a2")
ALIGNMENTS = (0, 1, 2, 3)


def offsets(k):
    """Element offsets of the six arrays of a call in alignment case k."""
    if k == 0:
        return dict.fromkeys(ARRAYS, 0)
    return {"sig": k, "feat": k, "p1": 2 * k - 1, "p2": 2 * k - 1, "a1": 2 * k - 1, "a2": 2 * k + 1}


def case_seed(T):
    return T32_SEED if T == 32 else 8100 + T


def band_layout(shape, itemsize, offset_elems):
    """(front, payload, back) in bytes."""
    row = int(np.prod(shape[1:], dtype=np.int64)) * itemsize
    return GUARD_ROWS * row + offset_elems * itemsize, int(shape[0]) * row, GUARD_ROWS * row


def _addr(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def _nbytes(x):
    return x.nbytes if isinstance(x, np.ndarray) else x.numel() * x.element_size()


def _put(dst, src):
    """src (a scalar, an ndarray or a tensor) into dst (an ndarray or a tensor), element for element."""
    if isinstance(dst, np.ndarray):
        dst[...] = src
    elif isinstance(src, (int, float)):
        dst.fill_(src)
    else:
        import torch
        dst.copy_(torch.as_tensor(src).reshape(dst.shape))


def banded(shape, dtype, offset_elems=0, fill=None, device="cuda", align=64):
    """One torch buffer [front guard | payload | back guard] of uint8 and the payload view of `shape` and `dtype` (a torch
    dtype).  The guards hold GUARD_BYTE; fill: a scalar, an array of the payload's shape, or None (zeros)."""
    import torch
    front, pay, back = band_layout(shape, torch.empty(0, dtype=dtype).element_size(), offset_elems)
    raw = torch.zeros(front + pay + back + align, dtype=torch.uint8, device=device)
    skip = -raw.data_ptr() % align
    buf = raw[skip:skip + front + pay + back]
    buf[:front] = GUARD_BYTE
    buf[front + pay:] = GUARD_BYTE
    payload = buf[front:front + pay].view(dtype).view(*shape)
    if fill is not None:
        _put(payload, fill)
    return buf, payload


def banded_np(shape, dtype, offset_elems=0, fill=None, align=64):
    """`banded` in NumPy memory."""
    dtype = np.dtype(dtype)
    front, pay, back = band_layout(shape, dtype.itemsize, offset_elems)
    raw = np.zeros(front + pay + back + align, np.uint8)
    skip = -raw.ctypes.data % align
    buf = raw[skip:skip + front + pay + back]
    buf[:front] = GUARD_BYTE
    buf[front + pay:] = GUARD_BYTE
    payload = buf[front:front + pay].view(dtype).reshape(shape)
    if fill is not None:
        _put(payload, fill)
    return buf, payload


def guards(buf, payload):
    """(front, back): the uint8 views of a band's guards."""
    front = _addr(payload) - _addr(buf)
    end = front + _nbytes(payload)
    assert 0 <= front and end <= _nbytes(buf)
    return buf[:front], buf[end:]


def fill_guards(buf, payload, what):
    """Both guards of a band: an int is a byte value, a float a value of the payload's (float) type, an array a decoy of the
    payload's type whose flattened END lies in front of the payload and whose START behind it, so that whole decoy rows touch
    the payload on both sides."""
    front, back = guards(buf, payload)
    if isinstance(what, int):
        _put(front, what), _put(back, what)
        return
    dt = payload.dtype
    f, b = (front.view(dt), back.view(dt))
    if isinstance(what, float):
        _put(f, what), _put(b, what)
        return
    flat = what.reshape(-1)
    assert flat.shape[0] >= f.shape[0] and flat.shape[0] >= b.shape[0], "the decoy is shorter than a guard"
    _put(f, flat[flat.shape[0] - f.shape[0]:]), _put(b, flat[:b.shape[0]])


def guards_hold(buf, payload, byte=GUARD_BYTE):
    """True when every byte of both guards still is `byte`."""
    front, back = guards(buf, payload)
    return bool((front == byte).all()) and bool((back == byte).all())


@functools.lru_cache(maxsize=None)
def windows(T):
    """Window mode at T: {'sig' (129, T, 50), 'feat' (129, T, 6), 'decoy_sig', 'decoy_feat'}, read-only."""
    from oracle import nrv_oracle as O
    sig, rd = O.synth_windows(N_MAX, T, seed=case_seed(T))
    ds, dr = O.synth_windows(N_MAX, T, seed=case_seed(T) + 5000)
    out = {"sig": sig, "feat": rd, "decoy_sig": ds, "decoy_feat": dr}
    for v in out.values():
        v.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def events(T):
    """Read mode at T: per-event arrays of N_MAX + T events ('sig' (N, 50), 'feat' (N, 6)) and their decoys; the case n is the
    first n + T events."""
    from oracle import nrv_oracle as O
    s, f = O.synth_windows(N_MAX + T, 1, seed=8300 + T)
    ds, df = O.synth_windows(N_MAX + T, 1, seed=13300 + T)
    out = {"sig": np.ascontiguousarray(s[:, 0]), "feat": np.ascontiguousarray(f[:, 0]),
           "decoy_sig": np.ascontiguousarray(ds[:, 0]), "decoy_feat": np.ascontiguousarray(df[:, 0])}
    for v in out.values():
        v.flags.writeable = False
    return out


def inputs(kind, T, n):
    """The two input arrays of the case n ('window': n windows, 'read': n + T events), contiguous copies, and the WHOLE decoys
    (a decoy fills guards, or stands where the inputs will be: `inputs(...)['decoy_sig'][:rows]`)."""
    src = events(T) if kind == "read" else windows(T)
    rows = n + T if kind == "read" else n
    return {k: np.array(v if k.startswith("decoy") else v[:rows], order="C") for k, v in src.items()}


_REFERENCE = {}


def reference(species_models, T):
    """Window mode at T against the oracle, computed once: the models, the fp64 arbiter q, the f32 floor nf and the C port's
    (probabilities, calls) c, per model."""
    if T not in _REFERENCE:
        from oracle import c_oracle as CO
        from oracle import nrv_oracle as O
        from parity_policy import f32_floor
        m1, m2 = (m.with_window(T) for m in species_models["ecoli"])
        w = windows(T)
        q1, q2, _, _ = O.predict_pair(m1.tensors, m2.tensors, w["sig"], w["feat"], np.float64)
        nf = f32_floor(m1, m2, w["sig"], w["feat"], q1, q2, T)
        c = (CO.predict(m1.flat(), T, 6, w["sig"], w["feat"], threads=8), CO.predict(m2.flat(), T, 5, w["sig"], w["feat"], threads=8))
        _REFERENCE[T] = dict(m1=m1, m2=m2, q=(q1, q2), nf=nf, c=c)
    return _REFERENCE[T]


_SCRATCH = {}


def producer_scratch(side=4096):
    """The operands of `slow_producer`'s matrix products, made once on the current stream, with one product run and waited for
    (so that the library behind torch.matmul is loaded before a case begins)."""
    import torch
    if side not in _SCRATCH:
        g = torch.Generator(device="cuda").manual_seed(side)
        a = torch.rand(side, side, device="cuda", generator=g)
        b = torch.rand(side, side, device="cuda", generator=g)
        c = torch.empty(side, side, device="cuda")
        torch.matmul(a, b, out=c)
        torch.cuda.synchronize()
        _SCRATCH[side] = (a, b, c)
    return _SCRATCH[side]


def slow_producer(stream, dst_pairs, k):
    """Enqueues on `stream`, in this order: k large matrix products into a scratch tensor, one copy_ per (dst, src) pair, an
    event record.  Returns the event.  Nothing here waits for anything: the caller has made the tensors visible to `stream`."""
    import torch
    a, b, c = producer_scratch()
    with torch.cuda.stream(stream):
        for _ in range(k):
            torch.matmul(a, b, out=c)
        for dst, src in dst_pairs:
            dst.copy_(src, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev
