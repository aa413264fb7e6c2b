"""ctypes binding of libnanorev_hip.so + the Keras-shaped facade the reference would call.

The reference builds two Keras models per read (NanoReviser.py:129-130,
output_handeler.py:206-307) whose public use is `model.predict([signal_x, read_x])`
-> (B, C) softmax.  `Reviser` keeps that call shape:

    rv = Reviser.from_species("ecoli")            # model/<S>/<S>_win13_50ep_model{1,2}
    p1 = rv.model1.predict([signal_x, read_x])    # (B,6)   == get_model1().predict(...)
    p2 = rv.model2.predict([signal_x, read_x])    # (B,5)   == get_model2().predict(...)
    p1, p2, a1, a2 = rv.predict_pair(signal_x, read_x)

There is no CPU fallback: if the shared library is missing or no HIP device is
usable, construction raises (the caller's "fall back to the original bases" path of
NanoReviser.py:146-152 is then what fires).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import fitdepth
from .weights import ModelWeights, load_species

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libnanorev_hip.so")
N_KERNELS = 6

SYMBOLS = [
    "nrv_create", "nrv_destroy", "nrv_predict", "nrv_predict_read", "nrv_predict_device",
    "nrv_predict_read_device", "nrv_set_batch", "nrv_get_batch", "nrv_set_stream", "nrv_sync",
    "nrv_prof_enable", "nrv_prof_read", "nrv_kernel_name", "nrv_last_error", "nrv_backend",
    "nrv_window", "nrv_set_precision", "nrv_get_precision", "nrv_predict_reads_raw", "nrv_reads_raw_begin", "nrv_reads_raw_end", "nrv_segment_reads",
    "nrv_device_count", "nrv_saturated", "nrv_prof_overhead",
    "nrv_reads_raw_stats_begin", "nrv_predict_reads_raw_stats", "nrv_read_stats",
    "nrv_revise_reads_raw_begin", "nrv_revise_reads_raw", "nrv_merge_calls",
    "nrv_revise_reads_raw_report_begin", "nrv_revise_reads_raw_report", "nrv_merge_calls_report",
    "nrv_revise_reads_raw_edits_begin", "nrv_revise_reads_raw_edits", "nrv_merge_calls_edits",
    "nrv_revise_reads_raw_records_begin", "nrv_revise_reads_raw_records", "nrv_pack_records",
    "nrv_revise_reads_raw_profile_begin", "nrv_revise_reads_raw_profile", "nrv_merge_calls_profile",
    "nrv_revise_reads_raw_trim_begin", "nrv_revise_reads_raw_trim", "nrv_merge_calls_trim", "nrv_trim_reads", "nrv_pack_records_trim",
    "nrv_revise_reads_raw_accuracy_begin", "nrv_revise_reads_raw_accuracy", "nrv_merge_calls_accuracy", "nrv_edit_distance",
    "nrv_revise_reads_raw_errclass_begin", "nrv_revise_reads_raw_errclass", "nrv_merge_calls_errclass", "nrv_edit_classes",
    "nrv_revise_reads_raw_infix_begin", "nrv_revise_reads_raw_infix", "nrv_merge_calls_infix", "nrv_infix_classes",
    "nrv_align_labels",
    "nrv_revise_reads_raw_score_begin", "nrv_revise_reads_raw_score", "nrv_merge_calls_score",
    "nrv_fit_reset", "nrv_fit_count", "nrv_fit_add_reads_raw", "nrv_fit_set_rows", "nrv_fit_get_rows", "nrv_fit_begin",
    "nrv_fit_grad", "nrv_fit_epoch", "nrv_fit_eval", "nrv_fit_params",
    "nrv_fit_set_depth", "nrv_fit_depth", "nrv_fit_set_rows_head", "nrv_fit_get_rows_head",
    "nrv_fit_set_rows_lstm4", "nrv_fit_get_rows_lstm4",
    "nrv_fit_set_rows_lstm3", "nrv_fit_get_rows_lstm3",
    "nrv_fit_set_rows_signal", "nrv_fit_get_rows_signal",
    "nrv_fit_set_rows_full", "nrv_fit_get_rows_full",
    "nrv_fit_bn_reestimate", "nrv_fit_bn_count", "nrv_fit_bn_get",
    "nrv_fit_set_bn_affine", "nrv_fit_bn_affine",
    "nrv_fit_set_dropout", "nrv_fit_dropout", "nrv_fit_set_dropout_draw", "nrv_fit_dropout_mask",
]
FIT_TAIL, FIT_HEAD, FIT_LSTM4, FIT_LSTM3, FIT_SIGNAL, FIT_FULL = (d.code for d in fitdepth.DEPTHS)   # NRV_FIT_*: 0, 1, 4, 8, 16, 32
FIT_MAX_BATCH = 65536               # NRV_FIT_MAX_BATCH
REPORT_COLS = 24                    # NRV_REPORT_COLS
PROFILE_COLS = 48                   # NRV_PROFILE_COLS
ACCURACY_COLS = 4                   # NRV_ACCURACY_COLS
ERRCLASS_COLS = 6                   # NRV_ERRCLASS_COLS
INFIX_COLS = 18                     # NRV_INFIX_COLS
INFIX_MAX_LEN = (1 << 21) - 1       # NRV_INFIX_MAX_LEN
INFIX_R = 16                        # kInfixR of csrc/nrv_infix.h: region characters per lane; a stripe is 64 of them
LABEL_COLS = 7                      # NRV_LABEL_COLS
LABELS_MAX_LEN = 65536              # NRV_LABELS_MAX_LEN: of a read and of end - start
SCORE_COLS = 248                    # NRV_SCORE_COLS
ERRCLASS_R = 16                     # kErrclassR of csrc/nrv_errclass.h: truth characters per lane; a stripe is 64 of them

PRECISIONS = {"f32": 0, "bf16x3": 1, "f16x2": 2}


class NrvError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libnanorev_hip: error {code}: {msg}")
        self.code = code


class _Weights(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_float)), ("n_f32", C.c_int64)]


class _ReadDesc(C.Structure):
    _fields_ = [("raw_off", C.c_int64), ("raw_len", C.c_int64), ("ev_off", C.c_int64), ("ev_len", C.c_int64),
                ("shift", C.c_double), ("scale", C.c_double)]


_FP, _DP = C.POINTER(C.c_float), C.POINTER(C.c_double)
_I8P, _U8P, _I16P, _I32P = C.POINTER(C.c_int8), C.POINTER(C.c_uint8), C.POINTER(C.c_int16), C.POINTER(C.c_int32)
_I64P, _U64P = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)


def _ptr(a, typ):
    """The C pointer to a NumPy array's data; None (NULL) for None."""
    return None if a is None else a.ctypes.data_as(typ)


def _marshal(values, types):
    """Python values -> C arguments of `types`: arrays (or None) to pointers, a float to c_float, the rest as it is."""
    return [_ptr(v, typ) if issubclass(typ, C._Pointer) else (typ(v) if typ is C.c_float else v) for v, typ in zip(values, types)]


# The raw-read family (include/nanorev.h).  Every entry point takes the head, then some of the blocks below in this order; its
# *_begin form ends with the ticket.  A block is (C types, where a packed tuple holds the values).  `load_library` declares the
# signatures and `Reviser._raw_call` marshals the calls from the same table, so neither two signatures nor a signature and its
# call can drift apart.
_RAW_HEAD_T = [C.c_void_p, _I16P, C.c_int64, _I32P, _FP, C.c_int64, C.POINTER(_ReadDesc), C.c_int]
_CALLS = ([_FP, _FP, _I8P, _I8P], lambda p: p[6])                                        # p1, p2, a1, a2
_STATS = ([_I32P, _U8P], lambda p: p[7:9])                                               # last_dur, on_device
_MERGE = ([_U8P, _FP, _U8P, _U8P, _I64P], lambda p: (p[9], p[10]) + tuple(p[11]))        # bases, q_thr, seq, qual, off
_REPORT = ([C.c_float, _U64P], lambda p: p[12:14])                                       # tie_eps, report
_EDITS = ([C.c_void_p, _I64P], lambda p: (None if p[14] is None else p[14].ctypes.data, p[15]))   # edits (nrv_edit records), edit_off
_RECORDS = ([_U8P, _I64P, _U8P, _I64P], lambda p: p[16:20])                              # names, name_off, blob, rec_off
_PROFILE = ([_FP, _U64P], lambda p: p[20:22])                                            # prof_thr, profile
_TRIM = ([_FP, C.c_int, C.c_int, C.c_int64, _I64P], lambda p: p[22:27])                   # trim_thr, Q, W, min_len, trim
_TRUTH = ([_U8P, _I64P, _U64P], lambda p: p[27:30])                                      # truth, truth_off, accuracy
_ERRCLASS = ([_U64P], lambda p: p[30:31])                                                # errclass
_INFIX = ([C.c_int, _U64P], lambda p: p[31:33])                                          # strands, infix
_SCORE = ([_U8P, _FP, _U64P], lambda p: p[33:36])                                        # labels, score_thr, score
# len(packed) -> (synchronous symbol, begin symbol, blocks, whether the call returns merged reads: (seq, qual, off[, report]
# [, edits, edit_off][, blob, rec_off][, profile][, trim][, accuracy][, errclass][, errclass | None, infix][, score]))
_RAW_FORMS = {
    7: ("nrv_predict_reads_raw", "nrv_reads_raw_begin", (_CALLS,), False),
    9: ("nrv_predict_reads_raw_stats", "nrv_reads_raw_stats_begin", (_STATS, _CALLS), False),
    12: ("nrv_revise_reads_raw", "nrv_revise_reads_raw_begin", (_STATS, _MERGE), True),
    14: ("nrv_revise_reads_raw_report", "nrv_revise_reads_raw_report_begin", (_STATS, _MERGE, _REPORT), True),
    16: ("nrv_revise_reads_raw_edits", "nrv_revise_reads_raw_edits_begin", (_STATS, _MERGE, _REPORT, _EDITS), True),
    20: ("nrv_revise_reads_raw_records", "nrv_revise_reads_raw_records_begin", (_STATS, _MERGE, _REPORT, _EDITS, _RECORDS), True),
    22: ("nrv_revise_reads_raw_profile", "nrv_revise_reads_raw_profile_begin", (_STATS, _MERGE, _REPORT, _EDITS, _RECORDS, _PROFILE), True),
    27: ("nrv_revise_reads_raw_trim", "nrv_revise_reads_raw_trim_begin", (_STATS, _MERGE, _REPORT, _EDITS, _RECORDS, _PROFILE, _TRIM), True),
}
# ... and the forms that carry a truth set, in a table of their own (`_raw_call` consults it after the first)
_RAW_FORMS_TRUTH = {
    30: ("nrv_revise_reads_raw_accuracy", "nrv_revise_reads_raw_accuracy_begin",
         (_STATS, _MERGE, _REPORT, _EDITS, _RECORDS, _PROFILE, _TRIM, _TRUTH), True),
    31: ("nrv_revise_reads_raw_errclass", "nrv_revise_reads_raw_errclass_begin",
         (_STATS, _MERGE, _REPORT, _EDITS, _RECORDS, _PROFILE, _TRIM, _TRUTH, _ERRCLASS), True),
}
# ... and the form that places the reads inside truth REGIONS, in a table of its own (tests/test_errclass_host.py pins the one above)
_RAW_FORMS_INFIX = {
    33: ("nrv_revise_reads_raw_infix", "nrv_revise_reads_raw_infix_begin",
         (_STATS, _MERGE, _REPORT, _EDITS, _RECORDS, _PROFILE, _TRIM, _TRUTH, _ERRCLASS, _INFIX), True),
}
# ... and the form that scores both classifiers against per-base labels (tests/test_infix_host.py pins the one above)
_RAW_FORMS_SCORE = {
    36: ("nrv_revise_reads_raw_score", "nrv_revise_reads_raw_score_begin",
         (_STATS, _MERGE, _REPORT, _EDITS, _RECORDS, _PROFILE, _TRIM, _TRUTH, _ERRCLASS, _INFIX, _SCORE), True),
}
_PACK_RECORDS_T = [C.c_void_p, _U8P, _U8P, _I64P, C.c_int, _U8P, _I64P, _U8P, _I64P]         # nrv_pack_records
_READS_HEAD_T = _RAW_HEAD_T[:4] + [C.c_int64, C.POINTER(_ReadDesc), C.c_int]     # nrv_segment_reads, nrv_read_stats: no features
_MERGE_CALLS_T = [C.c_void_p, _U8P, _I64P, C.c_int, _I8P, _I8P, _FP, _FP, C.c_int64] + _MERGE[0][1:]   # nrv_merge_calls
_TRIM_READS_T = [C.c_void_p, _U8P, _I64P, C.c_int, C.c_int, C.c_int, _I64P]                  # nrv_trim_reads
_PACK_RECORDS_TRIM_T = _PACK_RECORDS_T[:7] + [_I64P, C.c_int64] + _PACK_RECORDS_T[7:]        # nrv_pack_records_trim
_EDIT_DISTANCE_T = [C.c_void_p, _U8P, _I64P, _U8P, _I64P, C.c_int, _I64P]                    # nrv_edit_distance
_EDIT_CLASSES_T = _EDIT_DISTANCE_T + [_I64P]                                                 # nrv_edit_classes
_INFIX_CLASSES_T = _EDIT_DISTANCE_T[:6] + [C.c_int, _I64P, _I64P, _I64P, _I64P]              # nrv_infix_classes
_ALIGN_LABELS_T = _EDIT_DISTANCE_T[:6] + [_U8P, _I64P, _I64P, _U8P, _I64P]                   # nrv_align_labels
_U32P = C.POINTER(C.c_uint32)


class _FitOpts(C.Structure):                                                                 # nrv_fit_opts
    _fields_ = [("B", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("lam", C.c_float), ("cw", C.c_float * 6)]


class _FitStats(C.Structure):                                                                # nrv_fit_stats
    _fields_ = [("rows", C.c_int64), ("correct", C.c_int64), ("steps", C.c_int64), ("nonfinite", C.c_int64),
                ("ce_sum", C.c_double), ("center_sum", C.c_double)]


class _FitBnInfo(C.Structure):                                                               # nrv_fit_bn_info
    _fields_ = [("tensor_base", C.c_int), ("channels", C.c_int), ("n", C.c_int64)]


_FIT_T = {                                                                                   # the nrv_fit_* family
    "nrv_fit_reset": [C.c_void_p],
    "nrv_fit_count": [C.c_void_p],
    "nrv_fit_add_reads_raw": _RAW_HEAD_T + _STATS[0] + [_U8P, _I64P],
    "nrv_fit_begin": [C.c_void_p, C.c_int, _FP, C.POINTER(_FitOpts)],
    "nrv_fit_grad": [C.c_void_p, C.c_int, _U32P, C.c_int, _FP, C.POINTER(_FitStats)],
    "nrv_fit_epoch": [C.c_void_p, C.c_int, _U32P, C.c_int64, C.POINTER(_FitStats)],
    "nrv_fit_eval": [C.c_void_p, C.c_int, _U32P, C.c_int64, _FP, C.POINTER(_FitStats)],
    "nrv_fit_params": [C.c_void_p, C.c_int, _FP, _I64P],
    "nrv_fit_set_depth": [C.c_void_p, C.c_int],
    "nrv_fit_depth": [C.c_void_p],
    "nrv_fit_bn_reestimate": [C.c_void_p, C.c_int, _U32P, C.c_int64],
    "nrv_fit_bn_count": [C.c_void_p],
    "nrv_fit_set_bn_affine": [C.c_void_p, C.c_int],
    "nrv_fit_bn_affine": [C.c_void_p],
    "nrv_fit_set_dropout": [C.c_void_p, C.c_double, C.c_uint64],
    "nrv_fit_dropout": [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)],
    "nrv_fit_set_dropout_draw": [C.c_void_p, C.c_int, C.c_int64],
    "nrv_fit_dropout_mask": [C.c_void_p, C.c_int, _U32P, C.c_int, C.c_int64, C.POINTER(C.c_uint8)],
    "nrv_fit_bn_get": [C.c_void_p, C.c_int, C.c_int, C.POINTER(_FitBnInfo), _FP, _FP, _DP, _DP],
}
for _d in fitdepth.DEPTHS:                                                                   # the row doors of every depth
    _FIT_T["nrv_fit_set_rows" + _d.suffix] = [C.c_void_p] + [_FP] * len(_d.door_args()) + [_U8P, _U8P, C.c_int64]
    _FIT_T["nrv_fit_get_rows" + _d.suffix] = [C.c_void_p, C.c_int64, C.c_int64] + [_FP] * len(_d.door_args()) + [_U8P, _U8P]


_lib = None


def _one_hip_runtime() -> str:
    """One HIP runtime per process, without importing torch.

    PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7, with its own HSA runtime
    next to it); libnanorev_hip.so needs the same SONAME and would otherwise resolve it to /opt/rocm's.
    Two HIP/HSA runtimes in one process do not share the GPU (the second sees no device), so whichever
    copy a process is going to use must be the one that is mapped FIRST:
      * a libamdhip64 is already mapped (torch was imported, or the caller linked HIP): nothing to do,
        the dynamic linker resolves our NEEDED entry to it by SONAME;
      * else, if torch is installed (found on sys.path, NOT imported), its bundled runtime is mapped
        now (RTLD_GLOBAL), so a later `import torch` in this process finds its own copy already there;
      * else (or NRV_NO_TORCH=1: a process that will never import torch, e.g. the command line) the
        system runtime is found through the library's RUNPATH.
    NRV_HIP_RUNTIME=/path/to/libamdhip64.so overrides all of it."""
    try:
        with open("/proc/self/maps") as fp:
            if any("libamdhip64" in ln for ln in fp):
                return "already mapped"
    except OSError:
        pass
    cand = os.environ.get("NRV_HIP_RUNTIME")
    if not cand and os.environ.get("NRV_NO_TORCH") != "1":
        import importlib.util
        try:
            spec = importlib.util.find_spec("torch")
        except (ImportError, ValueError):
            spec = None
        if spec is not None and spec.origin:
            c = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            cand = c if os.path.exists(c) else None
    if cand:
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
        return cand
    return "system (RUNPATH)"


def load_library(path: Optional[str] = None):
    """dlopen the engine.  Raises OSError loudly when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("NRV_LIB") or LIB_PATH        # NRV_LIB: another build of the same ABI
    if not os.path.exists(p):
        raise OSError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    _one_hip_runtime()
    lib = C.CDLL(p)
    fp, i8p, vp = _FP, _I8P, C.c_void_p
    lib.nrv_create.argtypes = [C.POINTER(_Weights), C.POINTER(_Weights), C.c_int, C.c_int, C.c_int,
                               C.POINTER(vp)]
    lib.nrv_create.restype = C.c_int
    lib.nrv_destroy.argtypes = [vp]
    lib.nrv_destroy.restype = None
    for name in ("nrv_predict", "nrv_predict_read"):
        f = getattr(lib, name)
        f.argtypes = [vp, fp, fp, C.c_int64, fp, fp, i8p, i8p]
        f.restype = C.c_int
    for name in ("nrv_predict_device", "nrv_predict_read_device"):
        f = getattr(lib, name)
        f.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, vp]
        f.restype = C.c_int
    lib.nrv_set_batch.argtypes = [vp, C.c_int]
    lib.nrv_get_batch.argtypes = [vp]
    lib.nrv_set_stream.argtypes = [vp, vp]
    lib.nrv_sync.argtypes = [vp]
    lib.nrv_prof_enable.argtypes = [vp, C.c_int]
    lib.nrv_prof_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.nrv_kernel_name.argtypes = [C.c_int]
    lib.nrv_kernel_name.restype = C.c_char_p
    lib.nrv_last_error.argtypes = [vp]
    lib.nrv_last_error.restype = C.c_char_p
    lib.nrv_backend.argtypes = [vp]
    lib.nrv_window.argtypes = [vp]
    lib.nrv_device_count.argtypes = []
    have_report = hasattr(lib, "nrv_merge_calls_report")   # by presence: NRV_LIB may name an older build of the same ABI
    have_edits = hasattr(lib, "nrv_merge_calls_edits")
    have_records = hasattr(lib, "nrv_pack_records")
    have_profile = hasattr(lib, "nrv_merge_calls_profile")
    have_trim = hasattr(lib, "nrv_merge_calls_trim")
    have_truth = hasattr(lib, "nrv_merge_calls_accuracy")
    have_errclass = hasattr(lib, "nrv_merge_calls_errclass")
    have_infix = hasattr(lib, "nrv_merge_calls_infix")
    have_score = hasattr(lib, "nrv_merge_calls_score")
    for sync, begin, blocks, _ in list(_RAW_FORMS.values()) + list(_RAW_FORMS_TRUTH.values()) + list(_RAW_FORMS_INFIX.values()) + list(_RAW_FORMS_SCORE.values()):  # (every restype is ctypes' default, int: the nrv_* status)
        if (have_score or _SCORE not in blocks) and (have_infix or _INFIX not in blocks) and (have_errclass or _ERRCLASS not in blocks) and (have_truth or _TRUTH not in blocks) and (have_trim or _TRIM not in blocks) and (have_profile or _PROFILE not in blocks) and (have_records or _RECORDS not in blocks) \
                and (have_edits or _EDITS not in blocks) and (have_report or _REPORT not in blocks):
            getattr(lib, sync).argtypes = _RAW_HEAD_T + [t for types, _ in blocks for t in types]
            getattr(lib, begin).argtypes = getattr(lib, sync).argtypes + [C.POINTER(C.c_int)]
    lib.nrv_merge_calls.argtypes = _MERGE_CALLS_T
    if have_report:
        lib.nrv_merge_calls_report.argtypes = _MERGE_CALLS_T + _REPORT[0]
    if have_edits:
        lib.nrv_merge_calls_edits.argtypes = _MERGE_CALLS_T + _REPORT[0] + _EDITS[0]
    if have_records:
        lib.nrv_pack_records.argtypes = _PACK_RECORDS_T
    if have_profile:
        lib.nrv_merge_calls_profile.argtypes = _MERGE_CALLS_T + _PROFILE[0]
    if have_trim:
        lib.nrv_merge_calls_trim.argtypes = _MERGE_CALLS_T + _TRIM[0] + _RECORDS[0]
        lib.nrv_trim_reads.argtypes = _TRIM_READS_T
        lib.nrv_pack_records_trim.argtypes = _PACK_RECORDS_TRIM_T
    if have_truth:
        lib.nrv_merge_calls_accuracy.argtypes = _MERGE_CALLS_T + _TRUTH[0]
        lib.nrv_edit_distance.argtypes = _EDIT_DISTANCE_T
    if have_errclass:
        lib.nrv_merge_calls_errclass.argtypes = _MERGE_CALLS_T + _TRUTH[0]
        lib.nrv_edit_classes.argtypes = _EDIT_CLASSES_T
    if have_infix:
        lib.nrv_merge_calls_infix.argtypes = _MERGE_CALLS_T + _TRUTH[0][:2] + _INFIX[0]
        lib.nrv_infix_classes.argtypes = _INFIX_CLASSES_T
    if hasattr(lib, "nrv_align_labels"):
        lib.nrv_align_labels.argtypes = _ALIGN_LABELS_T
    if have_score:
        lib.nrv_merge_calls_score.argtypes = _MERGE_CALLS_T + _SCORE[0]
    if hasattr(lib, "nrv_fit_begin"):
        for name, types in _FIT_T.items():
            getattr(lib, name).argtypes = types
        lib.nrv_fit_count.restype = C.c_int64
    lib.nrv_reads_raw_end.argtypes = [vp, C.c_int]
    lib.nrv_segment_reads.argtypes = _READS_HEAD_T + [fp]
    lib.nrv_read_stats.argtypes = _READS_HEAD_T + [_I32P, _DP, _DP, _DP, _DP, fp]
    lib.nrv_prof_overhead.argtypes = [vp, C.POINTER(C.c_double)]
    lib.nrv_saturated.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.nrv_set_precision.argtypes = [vp, C.c_int]
    lib.nrv_get_precision.argtypes = [vp]
    if path is None:
        _lib = lib
    return lib


def device_count() -> int:
    """HIP devices visible to this process, asked of the engine library itself (no torch needed)."""
    return int(load_library().nrv_device_count())


def _as_f32(a, shape_tail):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim >= 1 and tuple(a.shape[-len(shape_tail):]) != tuple(shape_tail):
        raise ValueError(f"expected trailing shape {shape_tail}, got {a.shape}")
    return a


def _empty_calls(n):
    """The output arrays of a call over n windows: (p1, p2, a1, a2)."""
    return np.empty((n, 6), np.float32), np.empty((n, 5), np.float32), np.empty(n, np.int8), np.empty(n, np.int8)


class _ModelFacade:
    """`.predict([signal, read])` of one of the two Keras models (output_handeler.py:250-251)."""

    def __init__(self, owner: "Reviser", which: int):
        self._o, self._w = owner, which

    def predict(self, inputs: Sequence, batch_size: Optional[int] = None, verbose=0):
        signal_x, read_x = inputs
        return self._o._cached_pair(signal_x, read_x, batch_size)[self._w]


class Reviser:
    def __init__(self, model1: ModelWeights, model2: ModelWeights, device: int = 0,
                 recurrent_activation: str = "hard_sigmoid", batch: int = 4096,
                 lib_path: Optional[str] = None, precision: Optional[str] = None):
        if model1.T != model2.T:
            raise ValueError("model1/model2 window lengths differ")
        if recurrent_activation not in ("hard_sigmoid", "sigmoid"):
            raise ValueError("recurrent_activation must be 'hard_sigmoid' or 'sigmoid'")
        self._lib = load_library(lib_path)
        self.T = int(model1.T)
        self._h = C.c_void_p()
        f1, f2 = model1.flat(), model2.flat()
        w1 = _Weights(f1.ctypes.data_as(C.POINTER(C.c_float)), f1.size)
        w2 = _Weights(f2.ctypes.data_as(C.POINTER(C.c_float)), f2.size)
        rc = self._lib.nrv_create(C.byref(w1), C.byref(w2), self.T, int(device),
                                  0 if recurrent_activation == "hard_sigmoid" else 1,
                                  C.byref(self._h))
        if rc != 0:
            raise NrvError(rc, self._lib.nrv_last_error(None).decode())
        self.device = int(device)
        if batch != 4096:
            self.set_batch(batch)
        if precision is not None:
            self.set_precision(precision)
        self.model1 = _ModelFacade(self, 0)
        self.model2 = _ModelFacade(self, 1)
        self._cache_key = None
        self._cache_val = None

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_species(cls, species: str = "ecoli", model_dir: Optional[str] = None, T: Optional[int] = None,
                     **kw) -> "Reviser":
        """NanoReviser.py:191-193: ./model/<S>/<S>_win13_50ep_model{1,2}.h5 (or the .f32 form)."""
        m1, m2 = load_species(species, model_dir)
        if T is not None and T != m1.T:
            m1, m2 = m1.with_window(T), m2.with_window(T)
        return cls(m1, m2, **kw)

    def _check(self, rc: int):
        if rc != 0:
            raise NrvError(rc, self._lib.nrv_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.nrv_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ host-array API
    def predict_pair(self, signal_x, read_x, batch_size: Optional[int] = None):
        """Both models on n independent windows.  signal_x (n,T,50[,1]), read_x (n,T,6)."""
        read_x = _as_f32(read_x, (self.T, 6))
        n = read_x.shape[0]
        signal_x = np.ascontiguousarray(signal_x, dtype=np.float32).reshape(n, self.T, 50)
        if batch_size:
            self.set_batch(int(batch_size))
        out = _empty_calls(n)
        self._check(self._lib.nrv_predict(self._h, _ptr(signal_x, _FP), _ptr(read_x, _FP), n, *_marshal(out, _CALLS[0])))
        return out

    def predict_read(self, sig_ev, feat_ev):
        """Whole read: per-event arrays (N,50), (N,6) -> outputs for the N-T sliding windows."""
        sig_ev = _as_f32(sig_ev, (50,))
        feat_ev = _as_f32(feat_ev, (6,))
        N = feat_ev.shape[0]
        if sig_ev.shape[0] != N:
            raise ValueError("sig_ev / feat_ev length mismatch")
        n = max(N - self.T, 0)
        out = _empty_calls(n)
        self._check(self._lib.nrv_predict_read(self._h, _ptr(sig_ev, _FP), _ptr(feat_ev, _FP), N, *_marshal(out, _CALLS[0])))
        return out

    # ------------------------------------------------------------------ raw reads (device-side segmentation)
    @staticmethod
    def _pack_raw(raws, starts, shifts, scales):
        """Concatenate per-read int16 samples / int32 starts and build the nrv_read_desc array."""
        raws = [np.ascontiguousarray(r, dtype=np.int16) for r in raws]
        starts = [np.ascontiguousarray(s, dtype=np.int32) for s in starts]
        if not (len(raws) == len(starts) == len(shifts) == len(scales)):
            raise ValueError("raws / starts / shifts / scales must have one entry per read")
        descs = (_ReadDesc * max(len(raws), 1))()
        ro = eo = 0
        for i, (r, s) in enumerate(zip(raws, starts)):
            descs[i] = _ReadDesc(ro, r.size, eo, s.size, float(shifts[i]), float(scales[i]))
            ro += r.size
            eo += s.size
        raw = np.concatenate(raws) if raws else np.zeros(0, np.int16)
        st = np.concatenate(starts) if starts else np.zeros(0, np.int32)
        return raw, st, descs, len(raws)

    @classmethod
    def pack_reads_raw(cls, raws, starts, feats, shifts, scales, T: int):
        """Host-side preparation of a `predict_reads_raw` call (concatenation, descriptors, output arrays): pure
        NumPy, needs no engine - the command line does it in one thread while the engine thread is inside the
        previous batch's device call.  Returns the tuple `run_packed_raw` takes."""
        raw, st, descs, nr = cls._pack_raw(raws, starts, shifts, scales)
        feat = _as_f32(np.concatenate([np.asarray(f, np.float32).reshape(-1, 6) for f in feats])
                       if len(feats) else np.zeros((0, 6), np.float32), (6,))
        N = feat.shape[0]
        if st.size != N:
            raise ValueError("starts / feats length mismatch")
        n = max(N - T, 0)
        out = (np.empty((n, 6), np.float32), np.empty((n, 5), np.float32), np.empty(n, np.int8), np.empty(n, np.int8))
        return raw, st, feat, descs, nr, N, out

    @staticmethod
    def pack_bundle(raw, starts, feat, meta, T: int):
        """`pack_reads_raw` for arrays that are ALREADY concatenated (the command line's worker processes do that):
        meta is one row (raw_len, ev_len, shift, scale) per read.  Builds the descriptors and the output arrays."""
        nr = len(meta)
        descs = (_ReadDesc * max(nr, 1))()
        ro = eo = 0
        for i, (rl, el, sh, sc) in enumerate(meta):
            descs[i] = _ReadDesc(ro, int(rl), eo, int(el), float(sh), float(sc))
            ro += int(rl)
            eo += int(el)
        raw = np.ascontiguousarray(raw, dtype=np.int16)
        st = np.ascontiguousarray(starts, dtype=np.int32)
        feat = _as_f32(feat, (6,))
        if ro != raw.size or eo != st.size or eo != feat.shape[0]:
            raise ValueError("bundle arrays do not match their read table")
        n = max(eo - T, 0)
        out = (np.empty((n, 6), np.float32), np.empty((n, 5), np.float32), np.empty(n, np.int8), np.empty(n, np.int8))
        return raw, st, feat, descs, nr, eo, out

    @staticmethod
    def with_device_stats(packed, last_dur, on_device):
        """The packed form of a call whose read statistics are computed on the device (include/nanorev.h
        nrv_reads_raw_stats_begin): what `pack_reads_raw` / `pack_bundle` returned, plus per read the samples of its last
        base and a flag - non-zero: the read's shift / scale and feature columns 1 - 2 are produced on the device and the
        values in `packed` ignored; zero: the read is used as given.  `run_packed_raw` / `begin_packed_raw` take either form."""
        nr = packed[4]
        ld = np.ascontiguousarray(last_dur, dtype=np.int32).reshape(-1)
        on = np.ascontiguousarray(on_device, dtype=np.uint8).reshape(-1)
        if ld.size != nr or on.size != nr:
            raise ValueError("last_dur / on_device must have one entry per read")
        return tuple(packed[:7]) + (ld, on)

    @staticmethod
    def with_device_merge(packed, bases, fastq, q_thr=None):
        """The packed form of a call whose merge runs on the device as well (include/nanorev.h nrv_revise_reads_raw_begin):
        what `pack_reads_raw` / `pack_bundle` returned, with or without `with_device_stats`, plus the reads' original bases
        (S1 or uint8 [N], concatenated like the per-event arrays) and, for fastq, the 39 Phred thresholds (default:
        cli.phred_thresholds()).  `run_packed_raw` / `begin_packed_raw` + `end_packed_raw` then return (seq uint8[total],
        qual uint8[total] | None, off int64[n_reads + 1]) - read r is seq[off[r]:off[r + 1]] - instead of (p1, p2, a1, a2):
        the bytes of hoststage.emit_calls on the call's outputs."""
        from .hostlib import bases_u8
        nr, N = packed[4], packed[5]
        b = bases_u8(bases)
        if b.size != N:
            raise ValueError("bases must have one entry per event")
        thr = None
        if fastq:
            if q_thr is None:
                from .cli import phred_thresholds
                q_thr = phred_thresholds()
            thr = np.ascontiguousarray(q_thr, dtype=np.float32).reshape(-1)
            if thr.size != 39:
                raise ValueError("q_thr must have 39 entries")
        n = packed[6][2].shape[0]
        cap = max(N + n, 1)
        out = (np.empty(cap, np.uint8), np.empty(cap, np.uint8) if fastq else None, np.zeros(nr + 1, np.int64))
        ld, on = (packed[7], packed[8]) if len(packed) == 9 else (None, None)
        return tuple(packed[:7]) + (ld, on, b, thr, out)

    @staticmethod
    def with_device_report(packed, tie_eps=None):
        """A `with_device_merge` tuple whose call also returns the per-read revision report (include/nanorev.h
        nrv_revise_reads_raw_report_begin; hoststage.revision_report is the definition): `run_packed_raw` /
        `begin_packed_raw` + `end_packed_raw` then return (seq, qual | None, off, report uint64[n_reads][24])."""
        if len(packed) != 12:
            raise ValueError("with_device_report extends a with_device_merge tuple")
        if tie_eps is None:
            from .hoststage import REPORT_TIE_EPS
            tie_eps = REPORT_TIE_EPS
        return tuple(packed) + (float(tie_eps), np.zeros((packed[4], REPORT_COLS), np.uint64))

    @staticmethod
    def with_device_edits(packed):
        """A `with_device_merge` (12 elements) or `with_device_report` (14) tuple whose call also returns the per-read edit list
        (include/nanorev.h nrv_revise_reads_raw_edits_begin; hoststage.revision_edits is the definition): `run_packed_raw` /
        `begin_packed_raw` + `end_packed_raw` then return (seq, qual | None, off, report | None, edits[:total], edit_off) -
        edits a hoststage.EDIT_DTYPE array, read r owning edits[edit_off[r]:edit_off[r + 1]].  Without a report (a 12-tuple) none
        is counted."""
        from .hoststage import EDIT_DTYPE
        if len(packed) not in (12, 14):
            raise ValueError("with_device_edits extends a with_device_merge or a with_device_report tuple")
        if len(packed) == 12:
            packed = tuple(packed) + (0.0, None)
        n = packed[6][2].shape[0]
        return tuple(packed) + (np.zeros(max(n, 1), EDIT_DTYPE), np.zeros(packed[4] + 1, np.int64))

    @staticmethod
    def _names_block(names):
        """R byte strings -> (names uint8[], name_off int64[R + 1]): the name arguments of the record calls."""
        names = [bytes(n) for n in names]
        lens = np.array([len(n) for n in names], np.int64).reshape(-1)
        joined = np.frombuffer(b"".join(names), np.uint8)
        return (joined.copy() if joined.size else np.zeros(1, np.uint8)), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

    @classmethod
    def with_device_records(cls, packed, names, hand_back=True):
        """A `with_device_merge` (12 elements), `with_device_report` (14) or `with_device_edits` (16) tuple whose call also lays
        the reads out as FASTA / FASTQ records (include/nanorev.h nrv_revise_reads_raw_records_begin; hoststage.pack_records is
        the definition).  names: one byte string per read (hoststage.record_name).  `run_packed_raw` / `begin_packed_raw` +
        `end_packed_raw` then return (seq, qual | None, off, report | None, edits[:total] | None, edit_off | None,
        blob[:rec_off[-1]], rec_off) - read r owns blob[rec_off[r]:rec_off[r + 1]].  hand_back=False: seq and qual are left on
        the device (both None in the result); off is still filled.  FASTQ or FASTA is what `with_device_merge` was given."""
        if len(packed) not in (12, 14, 16):
            raise ValueError("with_device_records extends a with_device_merge, a with_device_report or a with_device_edits tuple")
        packed = tuple(packed)
        if len(packed) == 12:
            packed += (0.0, None)
        if len(packed) == 14:
            packed += (None, None)
        nr, N = packed[4], packed[5]
        if len(names) != nr:
            raise ValueError("names must have one entry per read")
        nm, name_off = cls._names_block(names)
        q = 2 if packed[10] is not None else 1
        cap = int(name_off[-1]) + q * (N + packed[6][2].shape[0]) + 3 * q * nr
        if not hand_back:
            packed = packed[:11] + ((None, None, packed[11][2]),) + packed[12:]
        return packed + (nm, name_off, np.empty(max(cap, 1), np.uint8), np.zeros(nr + 1, np.int64))

    @staticmethod
    def with_device_profile(packed, q_thr=None):
        """A `with_device_merge` (12 elements), `with_device_report` (14), `with_device_edits` (16) or `with_device_records` (20)
        tuple whose call also returns the per-read quality and base profile (include/nanorev.h
        nrv_revise_reads_raw_profile_begin; hoststage.read_profile is the definition).  q_thr: the 39 thresholds the profile's
        qualities are computed with (default: cli.phred_thresholds()) - its own, whether the call writes a quality or not.
        `run_packed_raw` / `begin_packed_raw` + `end_packed_raw` then return (seq, qual | None, off, report | None,
        edits[:total] | None, edit_off | None, blob[:rec_off[-1]] | None, rec_off | None, profile uint64[n_reads][48]): what
        the tuple's own call returns, None for the blocks it does not carry, and the profile last."""
        if len(packed) not in (12, 14, 16, 20):
            raise ValueError("with_device_profile extends a with_device_merge, a with_device_report, a with_device_edits or a "
                             "with_device_records tuple")
        packed = tuple(packed)
        if len(packed) == 12:
            packed += (0.0, None)
        if len(packed) == 14:
            packed += (None, None)
        if len(packed) == 16:
            packed += (None, None, None, None)
        if q_thr is None:
            from .cli import phred_thresholds
            q_thr = phred_thresholds()
        thr = np.ascontiguousarray(q_thr, dtype=np.float32).reshape(-1)
        if thr.size != 39:
            raise ValueError("q_thr must have 39 entries")
        return packed + (thr, np.zeros((packed[4], PROFILE_COLS), np.uint64))

    @staticmethod
    def _trim_rule(Q, W, min_len, q_thr):
        """The arguments of the trim, checked: (thr float32[39], Q, W, min_len)."""
        Q, W, min_len = int(Q), int(W), int(min_len)
        if not (1 <= Q <= 40 and 1 <= W <= 64 and min_len >= 0):
            raise ValueError("the trim needs Q in 1 .. 40, W in 1 .. 64 and min_len >= 0")
        if q_thr is None:
            from .cli import phred_thresholds
            q_thr = phred_thresholds()
        thr = np.ascontiguousarray(q_thr, dtype=np.float32).reshape(-1)
        if thr.size != 39:
            raise ValueError("q_thr must have 39 entries")
        return thr, Q, W, min_len

    @classmethod
    def with_device_trim(cls, packed, Q, W=10, min_len=1, q_thr=None):
        """A `with_device_merge` (12 elements), `with_device_report` (14), `with_device_edits` (16), `with_device_records` (20) or
        `with_device_profile` (22) tuple whose call also finds, per read, the part a sliding quality window keeps (include/nanorev.h
        nrv_revise_reads_raw_trim_begin; hoststage.trim_bounds is the definition): Q in 1 .. 40, W in 1 .. 64; q_thr: the 39
        thresholds the trim's qualities are computed with (default: cli.phred_thresholds()) - its own, whether the call writes a
        quality or not.  `run_packed_raw` / `begin_packed_raw` + `end_packed_raw` then return what a `with_device_profile` call
        returns - None for the blocks the tuple does not carry, the profile included - and trim int64[n_reads][2] last.  seq,
        qual, off, report, edits and profile describe the untrimmed reads; the blob of a `with_device_records` tuple is the
        exception: hoststage.pack_records with this trim and min_len (a read whose kept part is shorter has no record)."""
        if len(packed) not in (12, 14, 16, 20, 22):
            raise ValueError("with_device_trim extends a with_device_merge, a with_device_report, a with_device_edits, a "
                             "with_device_records or a with_device_profile tuple")
        packed = tuple(packed)
        if len(packed) == 12:
            packed += (0.0, None)
        if len(packed) == 14:
            packed += (None, None)
        if len(packed) == 16:
            packed += (None, None, None, None)
        if len(packed) == 20:
            packed += (None, None)
        thr, Q, W, min_len = cls._trim_rule(Q, W, min_len, q_thr)
        return packed + (thr, Q, W, min_len, np.zeros((packed[4], 2), np.int64))

    @staticmethod
    def _truth_block(truth, truth_off, n_reads):
        """A truth set, checked: (truth uint8 - one byte where there is none, so that its pointer is not NULL -, truth_off
        int64[n_reads + 1])."""
        toff = np.ascontiguousarray(truth_off, dtype=np.int64).reshape(-1)
        if toff.size != n_reads + 1 or toff[0] != 0 or np.any(np.diff(toff) < 0):
            raise ValueError("truth_off must have n_reads + 1 entries that ascend from 0")
        if isinstance(truth, (bytes, bytearray)):
            truth = np.frombuffer(bytes(truth), np.uint8)
        t = np.ascontiguousarray(truth, dtype=np.uint8).reshape(-1)
        if t.size < int(toff[-1]):
            raise ValueError("truth is shorter than truth_off[-1]")
        return (t if t.size else np.zeros(1, np.uint8)), toff

    @classmethod
    def with_device_accuracy(cls, packed, truth, truth_off):
        """A `with_device_merge` (12 elements), `with_device_report` (14), `with_device_edits` (16), `with_device_records` (20),
        `with_device_profile` (22) or `with_device_trim` (27) tuple whose call also finds, per read, the edit distance of the
        original and of the revised read to the true sequence truth[truth_off[r]:truth_off[r + 1]] (include/nanorev.h
        nrv_revise_reads_raw_accuracy_begin; hoststage.read_accuracy is the definition; an empty truth: the read has none).
        The result has 30 elements: blocks the tuple does not carry are padded with their "not asked for" values, a NULL trim
        included, and elements 27 - 29 are truth uint8, truth_off int64[n_reads + 1] and accuracy uint64[n_reads][4].
        `run_packed_raw` / `begin_packed_raw` + `end_packed_raw` then return what a `with_device_trim` call returns - None
        for the blocks not carried - and the accuracy block LAST."""
        if len(packed) not in (12, 14, 16, 20, 22, 27):
            raise ValueError("with_device_accuracy extends a with_device_merge, a with_device_report, a with_device_edits, a "
                             "with_device_records, a with_device_profile or a with_device_trim tuple")
        packed = tuple(packed)
        if len(packed) == 12:
            packed += (0.0, None)
        if len(packed) == 14:
            packed += (None, None)
        if len(packed) == 16:
            packed += (None, None, None, None)
        if len(packed) == 20:
            packed += (None, None)
        if len(packed) == 22:
            packed += (None, 0, 0, 0, None)
        t, toff = cls._truth_block(truth, truth_off, packed[4])
        return packed + (t, toff, np.zeros((packed[4], ACCURACY_COLS), np.uint64))

    @classmethod
    def with_device_error_classes(cls, packed):
        """A `with_device_accuracy` tuple (30 elements) whose call also finds, per read, the edits and the matched columns of
        the best alignments of its truth with the original and with the revised read (include/nanorev.h
        nrv_revise_reads_raw_errclass_begin; hoststage.read_error_classes is the definition).  The result has 31 elements;
        element 30 is errclass uint64[n_reads][6].  `run_packed_raw` / `begin_packed_raw` + `end_packed_raw` then return what
        the `with_device_accuracy` call returns and the error-class block LAST."""
        if len(packed) != 30:
            raise ValueError("with_device_error_classes extends a with_device_accuracy tuple")
        return tuple(packed) + (np.zeros((packed[4], ERRCLASS_COLS), np.uint64),)

    @classmethod
    def with_device_infix(cls, packed, strands=2):
        """A `with_device_accuracy` (30 elements) or `with_device_error_classes` (31) tuple whose call also places, per read,
        the original and the revised read inside its truth REGION, free ends on the region, on the forward strand (strands = 1)
        or on both (include/nanorev.h nrv_revise_reads_raw_infix_begin; hoststage.read_infix is the definition).  The result
        has 33 elements: element 30 is the error-class block or None, 31 strands, 32 infix uint64[n_reads][18].
        `run_packed_raw` / `begin_packed_raw` + `end_packed_raw` then return what the `with_device_error_classes` call returns
        - None for its block where the tuple had none - and the infix block LAST."""
        if len(packed) not in (30, 31):
            raise ValueError("with_device_infix extends a with_device_accuracy or a with_device_error_classes tuple")
        if strands not in (1, 2):
            raise ValueError("strands is 1 or 2")
        packed = tuple(packed) + ((None,) if len(packed) == 30 else ())
        return packed + (int(strands), np.zeros((packed[4], INFIX_COLS), np.uint64))

    @staticmethod
    def _score_inputs(labels, score_thr, N):
        """The label bytes and the thresholds of a score, checked: (labels uint8[max(N, 1)], thr float32[39])."""
        lab = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)
        if lab.size != N:
            raise ValueError("labels must have one byte per event")
        if score_thr is None:
            from .cli import phred_thresholds
            score_thr = phred_thresholds()
        thr = np.ascontiguousarray(score_thr, dtype=np.float32).reshape(-1)
        if thr.size != 39:
            raise ValueError("score_thr must have 39 entries")
        return (lab if lab.size else np.full(1, 0xFF, np.uint8)), thr

    @classmethod
    def with_device_score(cls, packed, labels, score_thr=None):
        """Any merged tuple - `with_device_merge` (12 elements) up to `with_device_infix` (33) - whose call also scores both
        classifiers against per-base labels (include/nanorev.h nrv_revise_reads_raw_score_begin; hoststage.score_calls is the
        definition).  labels: uint8 [N], one byte per event in `align_labels`' format, 0xFF = unlabelled; score_thr: the 39
        thresholds of the calibration bins (default: cli.phred_thresholds()).  The result has 36 elements: blocks the tuple does
        not carry are padded with their "not asked for" values - a NULL truth included: the score reads none - and elements
        33 - 35 are labels, score_thr and score uint64[n_reads][248].  `run_packed_raw` / `begin_packed_raw` + `end_packed_raw`
        then return what a `with_device_infix` call returns - None for the blocks not carried - and the score block LAST."""
        if len(packed) not in (12, 14, 16, 20, 22, 27, 30, 31, 33):
            raise ValueError("with_device_score extends a merged tuple of 12, 14, 16, 20, 22, 27, 30, 31 or 33 elements")
        packed = tuple(packed)
        for size, pad in ((12, (0.0, None)), (14, (None, None)), (16, (None, None, None, None)), (20, (None, None)),
                          (22, (None, 0, 0, 0, None)), (27, (None, None, None)), (30, (None,)), (31, (2, None))):
            if len(packed) == size:
                packed += pad
        lab, thr = cls._score_inputs(labels, score_thr, packed[5])
        return packed + (lab, thr, np.zeros((packed[4], SCORE_COLS), np.uint64))

    @staticmethod
    def _trim_merged(out):
        seq, qual, off = out[:3]
        total = int(off[-1])
        more, tail = tuple(out[3:]), ()
        if len(more) in (6, 7, 8, 9, 10, 11):         # (..., profile[, trim[, accuracy[, errclass[, infix[, score]]]]]): a `with_device_profile` / `with_device_trim` / `with_device_accuracy` / `with_device_error_classes` / `with_device_infix` / `with_device_score` call; blocks it does not carry are None
            more, tail = more[:5], more[5:]
        if len(more) in (3, 5) and more[1] is not None:   # (report | None, edits, edit_off, ...): the used prefix of the records
            more = (more[0], more[1][:int(more[2][-1])], more[2]) + more[3:]
        if len(more) == 5 and more[3] is not None:    # (..., blob, rec_off): the used prefix of the blob
            more = more[:3] + (more[3][:int(more[4][-1])], more[4])
        return ((seq[:total] if seq is not None else None), (qual[:total] if qual is not None else None), off) + more + tail

    def _raw_head(self, packed):
        """The leading C arguments every raw-read entry point shares: handle, raw, n_raw, starts, feat, N, descs, n_reads."""
        raw, st, feat, descs, nr, N = packed[:6]
        return [self._h, _ptr(raw, _I16P), raw.size, _ptr(st, _I32P), _ptr(feat, _FP), N, descs, nr]

    def _raw_call(self, packed, begin: bool):
        """One call of the raw-read family for a packed tuple of any form (`_RAW_FORMS`): its synchronous entry point, or its
        *_begin with the ticket behind the same arguments.  Returns (ticket number or None, outputs, merged)."""
        form = _RAW_FORMS.get(len(packed)) or _RAW_FORMS_TRUTH.get(len(packed)) or _RAW_FORMS_INFIX.get(len(packed)) or _RAW_FORMS_SCORE.get(len(packed))
        if form is None:
            raise ValueError(f"a packed raw-read call has 7, 9, 12, 14, 16, 20, 22, 27 or 30 elements - or 31, a 30 with the error classes, or 33, with the infix block, or 36, with the score -, not {len(packed)}")
        sync, beg, blocks, merged = form
        if not hasattr(self._lib, beg):               # the report, edits, records, profile, trim, accuracy, error-class and infix pairs are found by presence
            raise NrvError(-1, f"this build of libnanorev_hip.so has no {beg}")
        args = self._raw_head(packed)
        for types, pick in blocks:
            args += _marshal(pick(packed), types)
        t = C.c_int(-1)
        self._check(getattr(self._lib, beg)(*args, C.byref(t)) if begin else getattr(self._lib, sync)(*args))
        return (t.value if begin else None), (packed[11] + tuple(packed[13:14]) + tuple(packed[14:16]) + tuple(packed[18:20]) + tuple(packed[21:22]) + tuple(packed[26:27]) + tuple(packed[29:31]) + tuple(packed[32:33]) + tuple(packed[35:36]) if merged else packed[6]), merged

    def run_packed_raw(self, packed):
        """The device call of `predict_reads_raw` on what `pack_reads_raw` prepared (or `with_device_stats` /
        `with_device_merge` / `with_device_report` / `with_device_edits` / `with_device_records` / `with_device_profile` /
        `with_device_trim` / `with_device_accuracy` / `with_device_error_classes` / `with_device_infix` / `with_device_score`
        extended)."""
        _, out, merged = self._raw_call(packed, False)
        return self._trim_merged(out) if merged else out

    def begin_packed_raw(self, packed):
        """First half of `run_packed_raw` (nrv_reads_raw_begin): the inputs are copied and the whole call is enqueued; returns a
        ticket for `end_packed_raw`.  At most two calls in flight; the OUTPUT arrays of `packed` must stay alive until the end."""
        t, out, merged = self._raw_call(packed, True)
        return (t, out, "merged") if merged else (t, out)

    def end_packed_raw(self, ticket):
        """Second half: waits for the call `ticket` names and returns its (p1, p2, a1, a2) - or, for a `with_device_merge`
        call, its (seq, qual, off), with the report behind them for a `with_device_report` call, (report | None, edits,
        edit_off) for a `with_device_edits` call and (report | None, edits | None, edit_off | None, blob, rec_off) - the blob
        trimmed to rec_off[-1] - for a `with_device_records` call; a `with_device_profile` call returns the latter with the
        profile behind it, a `with_device_trim` call with (profile | None, trim) behind it, a `with_device_accuracy` call with
        (profile | None, trim | None, accuracy) behind it, a `with_device_error_classes` call with the error classes behind
        that, a `with_device_infix` call with (error classes | None, infix) behind the accuracy, a `with_device_score` call
        with (accuracy | None, error classes | None, infix | None, score) there."""
        t, out = ticket[:2]
        self._check(self._lib.nrv_reads_raw_end(self._h, t))
        return self._trim_merged(out) if len(ticket) == 3 else out

    def predict_reads_raw(self, raws, starts, feats, shifts, scales):
        """Reads given as raw int16 samples (from their first event on), int32 event starts, (N,6)
        event features and the read's shift / scale; the signal windows are cut on the device.
        Returns the outputs of `predict_read` on the concatenated per-event arrays (sum(N) - T rows)."""
        return self.run_packed_raw(self.pack_reads_raw(raws, starts, feats, shifts, scales, self.T))

    # ------------------------------------------------------------------ fitting the per-window tail (nrv_fit_*)
    # include/nanorev.h states the rule; nanoreviser_amd/tailfit.py is the definition.  `model` is 0 or 1.
    def _n_class(self, model):
        return 6 if model == 0 else 5

    def fit_reset(self):
        self._check(self._lib.nrv_fit_reset(self._h))

    def fit_count(self) -> int:
        n = int(self._lib.nrv_fit_count(self._h))
        if n < 0:
            self._check(n)
        return n

    def fit_add_packed(self, packed, labels) -> int:
        """The labelled windows of a packed raw-read call (`pack_reads_raw` / `pack_bundle`, with or without
        `with_device_stats`) appended to the training set; labels: one nrv_align_labels byte per event, 0xFF = unlabelled.
        Returns the rows added."""
        N = packed[5]
        lb = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)
        if lb.size != N:
            raise ValueError("labels must have one byte per event")
        stats = packed[7:9] if len(packed) >= 9 else (None, None)
        added = C.c_int64(0)
        self._check(self._lib.nrv_fit_add_reads_raw(*self._raw_head(packed), *_marshal(stats, _STATS[0]), _ptr(lb, _U8P),
                                                    C.byref(added)))
        return int(added.value)

    def _fit_set(self, depth, arrays, y1, y2):
        """The set door of `depth` (a name of fitdepth.DEPTHS): `arrays` are its float arrays in door order."""
        d = fitdepth.BY_NAME[depth]
        xs = [_as_f32(v, sh) for v, sh in zip(arrays, d.door_shapes(self.T))]
        a, b = (np.ascontiguousarray(v, dtype=np.uint8).reshape(-1) for v in (y1, y2))
        n = xs[0].shape[0]
        if any(v.shape[0] != n for v in xs) or a.size != n or b.size != n:
            raise ValueError(" / ".join(d.door_args() + ("y1", "y2")) + " must have one entry per row")
        self._check(getattr(self._lib, "nrv_fit_set_rows" + d.suffix)(self._h, *(_ptr(v, _FP) for v in xs), _ptr(a, _U8P), _ptr(b, _U8P), n))

    def _fit_get(self, depth, first, count):
        """The get door of `depth` -> (its float arrays in door order ..., y1, y2) of rows [first, first + count)."""
        d = fitdepth.BY_NAME[depth]
        count = self.fit_count() - first if count is None else count
        xs = tuple(np.empty((count,) + sh, np.float32) for sh in d.door_shapes(self.T))
        ys = (np.empty(count, np.uint8), np.empty(count, np.uint8))
        self._check(getattr(self._lib, "nrv_fit_get_rows" + d.suffix)(self._h, first, count, *(_ptr(v, _FP) for v in xs),
                                                                      *(_ptr(v, _U8P) for v in ys)))
        return xs + ys

    def fit_set_rows(self, flat1, flat2, y1, y2):
        self._fit_set("tail", (flat1, flat2), y1, y2)

    def fit_get_rows(self, first=0, count=None):
        """-> (flat1, flat2, y1, y2) of rows [first, first + count)."""
        return self._fit_get("tail", first, count)

    def fit_begin(self, model, params=None, opts=None):
        """opts: a tailfit.FitOpts (None: the engine's defaults); params: the vector [Wf | bf | Wo | bo | Ce] (None: the
        handle's own tail and zero centres)."""
        o = None
        if opts is not None:
            o = _FitOpts(int(opts.B), opts.lr, opts.beta1, opts.beta2, opts.eps, opts.lam, (C.c_float * 6)(*opts.cw6()))
        p = None if params is None else np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
        if p is not None and p.size != self.fit_n_params(model):
            raise ValueError(f"expected {self.fit_n_params(model)} parameters, got {p.size}")
        self._check(self._lib.nrv_fit_begin(self._h, model, _ptr(p, _FP), None if o is None else C.byref(o)))

    def fit_n_params(self, model) -> int:
        """The length of a model's parameter vector at the current depth."""
        c = self._n_class(model)
        at = fitdepth.DEPTHS.index(fitdepth.BY_CODE[self.fit_depth()])
        bn = fitdepth.DEPTHS[at].bn if self.fit_bn_affine() else 0
        return bn + sum(d.front for d in fitdepth.DEPTHS[:at + 1]) + 96 * self.T + 16 + 16 * c + c + 16 * c

    # ---- the second depth (nanoreviser_amd/headfit.py is the definition): the set holds lstm4 outputs [T][128] per window
    def fit_set_depth(self, depth):
        """FIT_TAIL / FIT_HEAD / FIT_LSTM4 / FIT_LSTM3 / FIT_SIGNAL / FIT_FULL (or "tail" / "head" / "lstm4" / "lstm3" / "signal" /
        "full"), on an empty set only; forgets any fit_begin."""
        depth = fitdepth.CODES.get(depth, depth)
        self._check(self._lib.nrv_fit_set_depth(self._h, int(depth)))

    def fit_depth(self) -> int:
        d = int(self._lib.nrv_fit_depth(self._h))
        if d < 0:
            self._check(d)
        return d

    def fit_set_rows_head(self, x1, x2, y1, y2):
        self._fit_set("head", (x1, x2), y1, y2)

    def fit_get_rows_head(self, first=0, count=None):
        """-> (x1, x2, y1, y2) of rows [first, first + count), x [count][T][128]."""
        return self._fit_get("head", first, count)

    # ---- the third depth (nanoreviser_amd/lstm4fit.py is the definition): the set holds BatchNorm'd lstm3 outputs [T][256]
    def fit_set_rows_lstm4(self, xb1, xb2, y1, y2):
        self._fit_set("lstm4", (xb1, xb2), y1, y2)

    def fit_get_rows_lstm4(self, first=0, count=None):
        """-> (xb1, xb2, y1, y2) of rows [first, first + count), xb [count][T][256]."""
        return self._fit_get("lstm4", first, count)

    # ---- the fourth depth (nanoreviser_amd/lstm3fit.py is the definition): the set holds lstm3's inputs [T][192]
    def fit_set_rows_lstm3(self, x1, x2, y1, y2):
        self._fit_set("lstm3", (x1, x2), y1, y2)

    def fit_get_rows_lstm3(self, first=0, count=None):
        """-> (x1, x2, y1, y2) of rows [first, first + count), x [count][T][192]."""
        return self._fit_get("lstm3", first, count)

    # ---- the fifth depth (nanoreviser_amd/signalfit.py is the definition): the set holds lstm2 outputs [T][128] per model and
    # ONE array of samples [T][50] for both
    def fit_set_rows_signal(self, x2_1, x2_2, sig, y1, y2):
        self._fit_set("signal", (x2_1, x2_2, sig), y1, y2)

    def fit_get_rows_signal(self, first=0, count=None):
        """-> (x2_1, x2_2, sig, y1, y2) of rows [first, first + count), x2 [count][T][128], sig [count][T][50]."""
        return self._fit_get("signal", first, count)

    # ---- the sixth depth (nanoreviser_amd/fullfit.py is the definition): the set holds ONE array of samples [T][50] and ONE of
    # read features [T][6] for both models
    def fit_set_rows_full(self, sig, feat, y1, y2):
        self._fit_set("full", (sig, feat), y1, y2)

    def fit_get_rows_full(self, first=0, count=None):
        """-> (sig, feat, y1, y2) of rows [first, first + count), sig [count][T][50], feat [count][T][6]."""
        return self._fit_get("full", first, count)

    @staticmethod
    def _fit_stats(s):
        from .tailfit import FitStats
        return FitStats(rows=s.rows, correct=s.correct, ce_sum=s.ce_sum, center_sum=s.center_sum, steps=s.steps, nonfinite=s.nonfinite)

    def fit_grad(self, model, rows):
        """-> (g [P], FitStats) of the batch `rows` at the current parameters; nothing is updated."""
        r = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        g, s = np.empty(self.fit_n_params(model), np.float32), _FitStats()
        self._check(self._lib.nrv_fit_grad(self._h, model, _ptr(r, _U32P), r.size, _ptr(g, _FP), C.byref(s)))
        return g, self._fit_stats(s)

    def fit_epoch(self, model, order):
        r = np.ascontiguousarray(order, dtype=np.uint32).reshape(-1)
        s = _FitStats()
        self._check(self._lib.nrv_fit_epoch(self._h, model, _ptr(r, _U32P), r.size, C.byref(s)))
        return self._fit_stats(s)

    def fit_eval(self, model, order, want_p=True):
        """-> (p [n][C] | None, FitStats): forward only."""
        r = np.ascontiguousarray(order, dtype=np.uint32).reshape(-1)
        p = np.empty((r.size, self._n_class(model)), np.float32) if want_p else None
        s = _FitStats()
        self._check(self._lib.nrv_fit_eval(self._h, model, _ptr(r, _U32P), r.size, _ptr(p, _FP), C.byref(s)))
        return p, self._fit_stats(s)

    def fit_bn_reestimate(self, model, rows):
        """Re-estimate the moving statistics of every BatchNorm inside the fitted section over `rows` of the set, at the
        current parameters (bnfit.py is the definition); the fit of this model runs on them from here on.  -> fit_bn_stats."""
        r = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        self._check(self._lib.nrv_fit_bn_reestimate(self._h, model, _ptr(r, _U32P), r.size))
        return self.fit_bn_stats(model)

    def fit_bn_stats(self, model):
        """-> {name: dict(tensor_base, n, mean, var f32, s1, s2 f64)} of the BatchNorms inside the fitted section; n = 0 and the
        loaded statistics before any re-estimation."""
        from .bnfit import BATCHNORMS
        names = {base: k for k, (base, _) in BATCHNORMS.items()}
        out = {}
        count = self._lib.nrv_fit_bn_count(self._h)
        if count < 0:
            self._check(count)
        for which in range(count):
            info = _FitBnInfo()
            self._check(self._lib.nrv_fit_bn_get(self._h, model, which, C.byref(info), None, None, None, None))
            mean, var = np.empty(info.channels, np.float32), np.empty(info.channels, np.float32)
            s1, s2 = np.empty(info.channels, np.float64), np.empty(info.channels, np.float64)
            self._check(self._lib.nrv_fit_bn_get(self._h, model, which, None, _ptr(mean, _FP), _ptr(var, _FP), _ptr(s1, _DP), _ptr(s2, _DP)))
            out[names[info.tensor_base]] = {"tensor_base": int(info.tensor_base), "n": int(info.n), "mean": mean, "var": var, "s1": s1, "s2": s2}
        return out

    def fit_set_bn_affine(self, on):
        """Fit gamma and beta of the BatchNorms inside the fitted section too (nanoreviser_amd/bnaffine.py is the definition):
        while it is on, every vector of fit_begin / fit_grad / fit_params has their block in front - fitdepth's `bn` floats.
        Forgets any fit_begin; fit_set_depth switches it off."""
        self._check(self._lib.nrv_fit_set_bn_affine(self._h, 1 if on else 0))

    def fit_bn_affine(self) -> bool:
        v = int(self._lib.nrv_fit_bn_affine(self._h))
        if v < 0:
            self._check(v)
        return bool(v)

    def fit_set_dropout(self, rate, seed=0):
        """The reference's Dropout behind the identity block (nanoreviser_amd/dropout.py is the definition): rate in [0, 1), 0
        switches it off; depths signal and full.  Resets both models' draw counters; fit_set_depth switches it off."""
        self._check(self._lib.nrv_fit_set_dropout(self._h, float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def fit_dropout(self):
        """-> (rate, seed, (draw of model 0, draw of model 1))."""
        rate, seed, draw = C.c_double(0), C.c_uint64(0), (C.c_int64 * 2)()
        self._check(self._lib.nrv_fit_dropout(self._h, C.byref(rate), C.byref(seed), draw))
        return float(rate.value), int(seed.value), (int(draw[0]), int(draw[1]))

    def fit_set_dropout_draw(self, model, draw):
        """The draw the model's next batch drops at (fit_begin sets it to 0, fit_epoch advances it by its batches)."""
        self._check(self._lib.nrv_fit_set_dropout_draw(self._h, model, int(draw)))

    def fit_dropout_mask(self, model, rows, draw):
        """-> uint8 [len(rows)][T][400], 1 = kept: dropout.keep_mask's bytes for these set rows, formed on the device."""
        r = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        mask = np.empty((r.size, self.T, 400), np.uint8)
        self._check(self._lib.nrv_fit_dropout_mask(self._h, model, _ptr(r, _U32P), r.size, int(draw), _ptr(mask, C.POINTER(C.c_uint8))))
        return mask

    def fit_params(self, model):
        """-> (the parameter vector, t)."""
        p, t = np.empty(self.fit_n_params(model), np.float32), C.c_int64(0)
        self._check(self._lib.nrv_fit_params(self._h, model, _ptr(p, _FP), C.byref(t)))
        return p, int(t.value)

    def segment_reads(self, raws, starts, shifts, scales):
        """The device-side signal segmentation alone: (sum(N), 50) float32."""
        raw, st, descs, nr = self._pack_raw(raws, starts, shifts, scales)
        out = np.empty((st.size, 50), np.float32)
        self._check(self._lib.nrv_segment_reads(self._h, _ptr(raw, _I16P), raw.size, _ptr(st, _I32P), st.size, descs, nr,
                                                _ptr(out, _FP)))
        return out

    def read_stats(self, raws, starts, last_durs):
        """The device-side read statistics alone (nrv_read_stats): per read the int16 samples from its first event on, its
        int32 event starts and the samples of its last base.  Returns (shift[R], scale[R], mean[sum N], std[sum N] float64,
        feat12 (sum N, 2) float32 = feature columns 1 and 2), bit for bit what the host stage computes."""
        nr = len(raws)
        raw, st, descs, _ = self._pack_raw(raws, starts, [0.0] * nr, [0.0] * nr)
        ld = np.ascontiguousarray(last_durs, dtype=np.int32).reshape(-1)
        if ld.size != nr:
            raise ValueError("last_durs must have one entry per read")
        N = st.size
        shift, scale = np.empty(nr, np.float64), np.empty(nr, np.float64)
        mean, std = np.empty(N, np.float64), np.empty(N, np.float64)
        f12 = np.empty((N, 2), np.float32)
        self._check(self._lib.nrv_read_stats(self._h, _ptr(raw, _I16P), raw.size, _ptr(st, _I32P), N, descs, nr, _ptr(ld, _I32P),
                                             *_marshal((shift, scale, mean, std, f12), [_DP, _DP, _DP, _DP, _FP])))
        return shift, scale, mean, std, f12

    @staticmethod
    def _merge_inputs(bases, ev_len, a1, a2, p1, p2, q_thr, with_p):
        """The inputs of nrv_merge_calls / nrv_merge_calls_report as contiguous arrays: (b, el, x1, x2, q1, q2, thr), the last
        three None where not given (q1 / q2: where not wanted)."""
        from .hostlib import bases_u8
        b = bases_u8(bases)
        el = np.ascontiguousarray(ev_len, dtype=np.int64).reshape(-1)
        x1, x2 = np.ascontiguousarray(a1, dtype=np.int8).reshape(-1), np.ascontiguousarray(a2, dtype=np.int8).reshape(-1)
        if int(el.sum()) != b.size or x2.size != x1.size:
            raise ValueError("bases / ev_len / a1 / a2 do not match")
        thr = None if q_thr is None else np.ascontiguousarray(q_thr, dtype=np.float32).reshape(-1)
        q1, q2 = (_as_f32(np.asarray(p1).reshape(-1, 6), (6,)), _as_f32(np.asarray(p2).reshape(-1, 5), (5,))) if with_p else (None, None)
        return b, el, x1, x2, q1, q2, thr

    def _merge_call(self, name, b, el, x1, x2, q1, q2, thr, *more):
        """`name` (nrv_merge_calls, or nrv_merge_calls_report with its two arguments in `more`) on checked inputs -> (seq, qual, off)."""
        n = x1.size
        cap = max(b.size + n, 1)
        out = (np.empty(cap, np.uint8), (np.empty(cap, np.uint8) if thr is not None else None), np.zeros(el.size + 1, np.int64))
        self._check(getattr(self._lib, name)(*_marshal((self._h, b, el, el.size, x1, x2, q1, q2, n, thr) + out, _MERGE_CALLS_T), *more))
        return self._trim_merged(out)

    def merge_calls_device(self, bases, ev_len, a1, a2, p1=None, p2=None, q_thr=None):
        """The device-side merge alone (nrv_merge_calls) on calls the host supplies: bases S1 / uint8 [sum ev_len], ev_len per
        read, a1 / a2 int8 [max(sum ev_len - T, 0)], and for a quality p1 (n, 6), p2 (n, 5) float32 with the 39 thresholds
        q_thr.  Returns (seq, qual | None, off) - the bytes of hoststage.emit_calls."""
        ins = self._merge_inputs(bases, ev_len, a1, a2, p1, p2, q_thr, q_thr is not None)     # p1 / p2 count only with q_thr
        n, (q1, q2, thr) = ins[2].size, ins[4:]
        if thr is not None and (thr.size != 39 or q1.shape[0] != n or q2.shape[0] != n):
            raise ValueError("q_thr / p1 / p2 do not match")
        return self._merge_call("nrv_merge_calls", *ins)

    def merge_calls_report_device(self, bases, ev_len, a1, a2, p1=None, p2=None, q_thr=None, tie_eps=None):
        """`merge_calls_device` with the per-read revision report (nrv_merge_calls_report): p1 / p2 may be given without q_thr
        (near_tie filled, q_sum 0).  Returns (seq, qual | None, off, report uint64[n_reads][24]) - the report is
        hoststage.revision_report's, bit for bit."""
        from .hoststage import REPORT_TIE_EPS
        if not hasattr(self._lib, "nrv_merge_calls_report"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_merge_calls_report")
        ins = self._merge_inputs(bases, ev_len, a1, a2, p1, p2, q_thr, p1 is not None and p2 is not None)
        n, (q1, q2, thr) = ins[2].size, ins[4:]
        if q1 is not None and (q1.shape[0] != n or q2.shape[0] != n):
            raise ValueError("p1 / p2 do not match")
        if thr is not None and (thr.size != 39 or q1 is None):
            raise ValueError("q_thr needs 39 entries and p1 / p2")
        rep = np.zeros((ins[1].size, REPORT_COLS), np.uint64)
        more = _marshal((REPORT_TIE_EPS if tie_eps is None else tie_eps, rep), _REPORT[0])
        return self._merge_call("nrv_merge_calls_report", *ins, *more) + (rep,)

    def merge_calls_edits_device(self, bases, ev_len, a1, a2, p1=None, p2=None, q_thr=None, tie_eps=None, report=True):
        """`merge_calls_report_device` with the per-read edit list (nrv_merge_calls_edits): p1 / p2 may be given without q_thr
        (conf filled, qual 0).  report=False: no report is counted.  Returns (seq, qual | None, off, report | None,
        edits[:total], edit_off) - edits and edit_off are hoststage.revision_edits', bit for bit."""
        from .hoststage import EDIT_DTYPE, REPORT_TIE_EPS
        if not hasattr(self._lib, "nrv_merge_calls_edits"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_merge_calls_edits")
        ins = self._merge_inputs(bases, ev_len, a1, a2, p1, p2, q_thr, p1 is not None and p2 is not None)
        n, (q1, q2, thr) = ins[2].size, ins[4:]
        if q1 is not None and (q1.shape[0] != n or q2.shape[0] != n):
            raise ValueError("p1 / p2 do not match")
        if thr is not None and (thr.size != 39 or q1 is None):
            raise ValueError("q_thr needs 39 entries and p1 / p2")
        rep = np.zeros((ins[1].size, REPORT_COLS), np.uint64) if report else None
        edits, edit_off = np.zeros(max(n, 1), EDIT_DTYPE), np.zeros(ins[1].size + 1, np.int64)
        more = _marshal((REPORT_TIE_EPS if tie_eps is None else tie_eps, rep, edits.ctypes.data, edit_off), _REPORT[0] + _EDITS[0])
        return self._merge_call("nrv_merge_calls_edits", *ins, *more) + (rep, edits[:int(edit_off[-1])], edit_off)

    def merge_calls_profile_device(self, bases, ev_len, a1, a2, p1, p2, q_thr=None, prof_thr=None):
        """`merge_calls_device` with the per-read quality and base profile (nrv_merge_calls_profile): p1 / p2 are required, q_thr
        may be None (a FASTA merge whose profile is still filled), prof_thr defaults to cli.phred_thresholds().  Returns
        (seq, qual | None, off, profile uint64[n_reads][48]) - the profile is hoststage.read_profile's, bit for bit."""
        if not hasattr(self._lib, "nrv_merge_calls_profile"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_merge_calls_profile")
        if p1 is None or p2 is None:
            raise ValueError("the profile needs p1 / p2")
        if prof_thr is None:
            from .cli import phred_thresholds
            prof_thr = phred_thresholds()
        pthr = np.ascontiguousarray(prof_thr, dtype=np.float32).reshape(-1)
        ins = self._merge_inputs(bases, ev_len, a1, a2, p1, p2, q_thr, True)
        n, (q1, q2, thr) = ins[2].size, ins[4:]
        if q1.shape[0] != n or q2.shape[0] != n or pthr.size != 39 or (thr is not None and thr.size != 39):
            raise ValueError("p1 / p2 / q_thr / prof_thr do not match")
        prof = np.zeros((ins[1].size, PROFILE_COLS), np.uint64)
        return self._merge_call("nrv_merge_calls_profile", *ins, *_marshal((pthr, prof), _PROFILE[0])) + (prof,)

    def merge_calls_accuracy_device(self, bases, ev_len, a1, a2, truth, truth_off, p1=None, p2=None, q_thr=None):
        """`merge_calls_device` with the accuracy block (nrv_merge_calls_accuracy): truth uint8 and truth_off int64[n_reads + 1]
        as `with_device_accuracy` takes them.  Returns (seq, qual | None, off, accuracy uint64[n_reads][4]) - the block is
        hoststage.read_accuracy's, bit for bit."""
        if not hasattr(self._lib, "nrv_merge_calls_accuracy"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_merge_calls_accuracy")
        ins = self._merge_inputs(bases, ev_len, a1, a2, p1, p2, q_thr, q_thr is not None)
        n, (q1, q2, thr) = ins[2].size, ins[4:]
        if thr is not None and (thr.size != 39 or q1.shape[0] != n or q2.shape[0] != n):
            raise ValueError("q_thr / p1 / p2 do not match")
        nr = ins[1].size
        t, toff = self._truth_block(truth, truth_off, nr)
        acc = np.zeros((nr, ACCURACY_COLS), np.uint64)
        return self._merge_call("nrv_merge_calls_accuracy", *ins, *_marshal((t, toff, acc), _TRUTH[0])) + (acc,)

    def edit_distance_device(self, truths, reads):
        """align_kernel alone (nrv_edit_distance): truths and reads are equally long lists of byte strings (or uint8 arrays);
        returns int64[n_pairs], hoststage.edit_distance(truths[k], reads[k]) - and -1 where truths[k] is empty."""
        if not hasattr(self._lib, "nrv_edit_distance"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_edit_distance")
        if len(truths) != len(reads):
            raise ValueError("one read per truth")
        a, a_off = self._names_block(truths)
        b, b_off = self._names_block(reads)
        return self.edit_distance_offsets(a, a_off, b, b_off)

    def edit_distance_offsets(self, a, a_off, b, b_off):
        """`edit_distance_device` on the arrays as nrv_edit_distance takes them; the offsets are passed on unchecked."""
        a_off = np.ascontiguousarray(a_off, dtype=np.int64).reshape(-1)
        b_off = np.ascontiguousarray(b_off, dtype=np.int64).reshape(-1)
        a, b = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1), np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
        n = a_off.size - 1
        dist = np.zeros(max(n, 1), np.int64)
        self._check(self._lib.nrv_edit_distance(*_marshal((self._h, a if a.size else np.zeros(1, np.uint8), a_off,
                                                           b if b.size else np.zeros(1, np.uint8), b_off, n, dist), _EDIT_DISTANCE_T)))
        return dist[:n]

    def merge_calls_errclass_device(self, bases, ev_len, a1, a2, truth, truth_off, p1=None, p2=None, q_thr=None):
        """`merge_calls_accuracy_device` with the error-class block in the accuracy's place (nrv_merge_calls_errclass).  Returns
        (seq, qual | None, off, errclass uint64[n_reads][6]) - the block is hoststage.read_error_classes', bit for bit."""
        if not hasattr(self._lib, "nrv_merge_calls_errclass"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_merge_calls_errclass")
        ins = self._merge_inputs(bases, ev_len, a1, a2, p1, p2, q_thr, q_thr is not None)
        n, (q1, q2, thr) = ins[2].size, ins[4:]
        if thr is not None and (thr.size != 39 or q1.shape[0] != n or q2.shape[0] != n):
            raise ValueError("q_thr / p1 / p2 do not match")
        nr = ins[1].size
        t, toff = self._truth_block(truth, truth_off, nr)
        ec = np.zeros((nr, ERRCLASS_COLS), np.uint64)
        return self._merge_call("nrv_merge_calls_errclass", *ins, *_marshal((t, toff, ec), _TRUTH[0])) + (ec,)

    def edit_classes_device(self, truths, reads):
        """errclass_kernel alone (nrv_edit_classes): truths and reads are equally long lists of byte strings (or uint8 arrays);
        returns (dist, match), int64[n_pairs] each, hoststage.edit_classes(truths[k], reads[k]) - and -1 / -1 where truths[k] is
        empty."""
        if not hasattr(self._lib, "nrv_edit_classes"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_edit_classes")
        if len(truths) != len(reads):
            raise ValueError("one read per truth")
        a, a_off = self._names_block(truths)
        b, b_off = self._names_block(reads)
        return self.edit_classes_offsets(a, a_off, b, b_off)

    def edit_classes_offsets(self, a, a_off, b, b_off):
        """`edit_classes_device` on the arrays as nrv_edit_classes takes them; the offsets are passed on unchecked."""
        if not hasattr(self._lib, "nrv_edit_classes"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_edit_classes")
        a_off = np.ascontiguousarray(a_off, dtype=np.int64).reshape(-1)
        b_off = np.ascontiguousarray(b_off, dtype=np.int64).reshape(-1)
        a, b = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1), np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
        n = a_off.size - 1
        dist, match = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        self._check(self._lib.nrv_edit_classes(*_marshal((self._h, a if a.size else np.zeros(1, np.uint8), a_off,
                                                          b if b.size else np.zeros(1, np.uint8), b_off, n, dist, match), _EDIT_CLASSES_T)))
        return dist[:n], match[:n]

    def merge_calls_infix_device(self, bases, ev_len, a1, a2, truth, truth_off, strands=2, p1=None, p2=None, q_thr=None):
        """`merge_calls_errclass_device` with the infix block in the error classes' place (nrv_merge_calls_infix).  Returns
        (seq, qual | None, off, infix uint64[n_reads][18]) - the block is hoststage.read_infix's, bit for bit."""
        if not hasattr(self._lib, "nrv_merge_calls_infix"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_merge_calls_infix")
        ins = self._merge_inputs(bases, ev_len, a1, a2, p1, p2, q_thr, q_thr is not None)
        n, (q1, q2, thr) = ins[2].size, ins[4:]
        if thr is not None and (thr.size != 39 or q1.shape[0] != n or q2.shape[0] != n):
            raise ValueError("q_thr / p1 / p2 do not match")
        nr = ins[1].size
        t, toff = self._truth_block(truth, truth_off, nr)
        blk = np.zeros((nr, INFIX_COLS), np.uint64)
        return self._merge_call("nrv_merge_calls_infix", *ins, *_marshal((t, toff, int(strands), blk), _TRUTH[0][:2] + _INFIX[0])) + (blk,)

    def merge_calls_score_device(self, bases, ev_len, a1, a2, labels, p1=None, p2=None, q_thr=None, score_thr=None):
        """`merge_calls_device` with the score of both classifiers against per-base labels (nrv_merge_calls_score): labels uint8
        [sum ev_len], 0xFF = unlabelled; p1 / p2 may be given without q_thr (a FASTA merge whose calibration and loss columns are
        still filled) or left out (those columns stay 0); score_thr defaults to cli.phred_thresholds().  Returns (seq,
        qual | None, off, score uint64[n_reads][248]) - the block is hoststage.score_calls', bit for bit."""
        if not hasattr(self._lib, "nrv_merge_calls_score"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_merge_calls_score")
        have_p = p1 is not None and p2 is not None
        ins = self._merge_inputs(bases, ev_len, a1, a2, p1, p2, q_thr, have_p)
        n, (q1, q2, thr) = ins[2].size, ins[4:]
        if (thr is not None and (thr.size != 39 or not have_p)) or (have_p and (q1.shape[0] != n or q2.shape[0] != n)):
            raise ValueError("q_thr / p1 / p2 do not match")
        lab, sthr = self._score_inputs(labels, score_thr, ins[0].size)
        blk = np.zeros((ins[1].size, SCORE_COLS), np.uint64)
        return self._merge_call("nrv_merge_calls_score", *ins, *_marshal((lab, sthr, blk), _SCORE[0])) + (blk,)

    def infix_classes_device(self, truths, reads, reverse=False):
        """infix_kernel alone (nrv_infix_classes): truths (the regions) and reads are equally long lists of byte strings (or
        uint8 arrays); returns (dist, match, start, end), int64[n_pairs] each, hoststage.infix_classes(truths[k], reads[k],
        reverse) - and -1 in all four where truths[k] is empty."""
        if not hasattr(self._lib, "nrv_infix_classes"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_infix_classes")
        if len(truths) != len(reads):
            raise ValueError("one read per truth")
        a, a_off = self._names_block(truths)
        b, b_off = self._names_block(reads)
        return self.infix_classes_offsets(a, a_off, b, b_off, reverse)

    def infix_classes_offsets(self, a, a_off, b, b_off, reverse=False):
        """`infix_classes_device` on the arrays as nrv_infix_classes takes them; the offsets and `reverse` are passed on unchecked."""
        if not hasattr(self._lib, "nrv_infix_classes"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_infix_classes")
        a_off = np.ascontiguousarray(a_off, dtype=np.int64).reshape(-1)
        b_off = np.ascontiguousarray(b_off, dtype=np.int64).reshape(-1)
        a, b = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1), np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
        n = a_off.size - 1
        outs = tuple(np.zeros(max(n, 1), np.int64) for _ in range(4))
        self._check(self._lib.nrv_infix_classes(*_marshal((self._h, a if a.size else np.zeros(1, np.uint8), a_off,
                                                           b if b.size else np.zeros(1, np.uint8), b_off, n, int(reverse)) + outs, _INFIX_CLASSES_T)))
        return tuple(x[:n] for x in outs)

    def align_labels_device(self, regions, reads, reverse, start, end):
        """labels_kernel and labels_walk_kernel (nrv_align_labels): regions and reads are equally long lists of byte strings (or
        uint8 arrays), reverse / start / end one value per pair; returns (a list of uint8 arrays, one label byte per read base,
        and summary int64[n_pairs][7]) - hoststage.align_labels(regions[k], reads[k], reverse[k], start[k], end[k]) bit for bit.
        The call runs on a stream of its own: it may be made while a `begin_packed_raw` call is in flight."""
        if not hasattr(self._lib, "nrv_align_labels"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_align_labels")
        if not len(regions) == len(reads) == len(reverse) == len(start) == len(end):
            raise ValueError("one read, one strand and one pair of bounds per region")
        a, a_off = self._names_block(regions)
        b, b_off = self._names_block(reads)
        labels, summary = self.align_labels_arrays(a, a_off, b, b_off, reverse, start, end)
        return [labels[int(b_off[k]):int(b_off[k + 1])] for k in range(len(reads))], summary

    def align_labels_arrays(self, a, a_off, b, b_off, reverse, start, end):
        """`align_labels_device` on the arrays as nrv_align_labels takes them: returns (labels uint8[b_off[-1]], summary
        int64[n_pairs][7]); the offsets, strands and bounds are passed on unchecked."""
        if not hasattr(self._lib, "nrv_align_labels"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_align_labels")
        a_off = np.ascontiguousarray(a_off, dtype=np.int64).reshape(-1)
        b_off = np.ascontiguousarray(b_off, dtype=np.int64).reshape(-1)
        a, b = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1), np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
        n = a_off.size - 1
        rev, st, en = (np.ascontiguousarray(x, dtype=t).reshape(-1) for x, t in ((reverse, np.uint8), (start, np.int64), (end, np.int64)))
        if not rev.size == st.size == en.size == n:
            raise ValueError("one strand and one pair of bounds per pair")
        labels, summary = np.zeros(max(b.size, 1), np.uint8), np.zeros((max(n, 1), LABEL_COLS), np.int64)
        pad = lambda x: x if x.size else np.zeros(1, x.dtype)   # noqa: E731
        self._check(self._lib.nrv_align_labels(*_marshal((self._h, pad(a), a_off, pad(b), b_off, n, pad(rev), pad(st), pad(en), labels, summary),
                                                         _ALIGN_LABELS_T)))
        return labels[:min(max(int(b_off[-1]), 0), b.size) if b_off.size else 0], summary[:max(n, 0)]

    def merge_calls_trim(self, bases, ev_len, a1, a2, p1, p2, Q, W=10, q_thr=None, trim_thr=None, names=None, min_len=1):
        """`merge_calls_device` with the sliding-window trim (nrv_merge_calls_trim): p1 / p2 are required, q_thr may be None (a
        FASTA merge whose trim is still computed), trim_thr defaults to cli.phred_thresholds().  Returns (seq, qual | None, off,
        trim int64[n_reads][2]) - the trim is cli.trim_rows', bit for bit - and with names (one byte string per read) the
        trimmed records (blob, rec_off) of hoststage.pack_records behind them."""
        if not hasattr(self._lib, "nrv_merge_calls_trim"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_merge_calls_trim")
        if p1 is None or p2 is None:
            raise ValueError("the trim needs p1 / p2")
        tthr, Q, W, min_len = self._trim_rule(Q, W, min_len, trim_thr)
        ins = self._merge_inputs(bases, ev_len, a1, a2, p1, p2, q_thr, True)
        n, (q1, q2, thr) = ins[2].size, ins[4:]
        if q1.shape[0] != n or q2.shape[0] != n or (thr is not None and thr.size != 39):
            raise ValueError("p1 / p2 / q_thr do not match")
        nr = ins[1].size
        trim = np.zeros((nr, 2), np.int64)
        rec = (None, None, None, None)
        if names is not None:
            if len(names) != nr:
                raise ValueError("names must have one entry per read")
            nm, name_off = self._names_block(names)
            q = 2 if thr is not None else 1
            rec = (nm, name_off, np.empty(max(int(name_off[-1]) + q * (ins[0].size + n) + 3 * q * nr, 1), np.uint8), np.zeros(nr + 1, np.int64))
        out = self._merge_call("nrv_merge_calls_trim", *ins, *_marshal((tthr, Q, W, min_len, trim) + rec, _TRIM[0] + _RECORDS[0])) + (trim,)
        return out if names is None else out + (rec[2][:int(rec[3][-1])], rec[3])

    def trim_reads(self, qual, off, Q, W=10):
        """The window and finish kernels alone (nrv_trim_reads) on quality characters the host supplies: the arguments and the
        result int64[n_reads][2] of hoststage.trim_bounds, bit for bit."""
        if not hasattr(self._lib, "nrv_trim_reads"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_trim_reads")
        _, Q, W, _ = self._trim_rule(Q, W, 0, np.zeros(39, np.float32))
        off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
        nr = off.size - 1
        ql = np.ascontiguousarray(qual, dtype=np.uint8).reshape(-1)
        if ql.size < int(off[-1]):
            raise ValueError("qual is shorter than off[-1]")
        if ql.size == 0:
            ql = np.zeros(1, np.uint8)
        trim = np.zeros((nr, 2), np.int64)
        self._check(self._lib.nrv_trim_reads(*_marshal((self._h, ql, off, nr, Q, W, trim), _TRIM_READS_T)))
        return trim

    def pack_records_trim(self, names, seq, qual, off, trim, min_len=1, blob=None):
        """`pack_records_device` with a trim (nrv_pack_records_trim): the arguments and the result of hoststage.pack_records with
        trim / min_len, byte for byte; trim None: `pack_records_device`'s bytes."""
        if not hasattr(self._lib, "nrv_pack_records_trim"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_pack_records_trim")
        if trim is not None:
            trim = np.ascontiguousarray(trim, dtype=np.int64).reshape(-1, 2)
            if trim.shape[0] != np.asarray(off).size - 1:
                raise ValueError("trim must have one row per read")
        return self.pack_records_device(names, seq, qual, off, blob, _trim=(trim, int(min_len)))

    def pack_records_device(self, names, seq, qual, off, blob=None, _trim=None):
        """The device-side record layout alone (nrv_pack_records) on merged reads the host supplies: the arguments and the
        result (blob, rec_off) of hoststage.pack_records, byte for byte.  blob: a uint8 array of at least the capacity to write
        into (the result is a view of its used prefix; nothing behind it is written)."""
        if not hasattr(self._lib, "nrv_pack_records"):
            raise NrvError(-1, "this build of libnanorev_hip.so has no nrv_pack_records")
        off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
        nr = off.size - 1
        if len(names) != nr:
            raise ValueError("names must have one entry per read")
        s = np.ascontiguousarray(seq, dtype=np.uint8).reshape(-1)
        ql = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8).reshape(-1)
        if s.size < int(off[-1]) or (ql is not None and ql.size < int(off[-1])):
            raise ValueError("seq / qual are shorter than off[-1]")
        nm, name_off = self._names_block(names)
        q = 2 if ql is not None else 1
        cap = max(int(name_off[-1]) + q * int(off[-1]) + 3 * q * nr, 1)
        if blob is None:
            blob = np.empty(cap, np.uint8)
        elif blob.dtype != np.uint8 or blob.ndim != 1 or blob.size < cap or not blob.flags.c_contiguous:
            raise ValueError(f"blob must be a contiguous uint8 array of at least {cap} bytes")
        rec_off = np.zeros(nr + 1, np.int64)
        if s.size == 0:
            s = np.zeros(1, np.uint8)
        if ql is not None and ql.size == 0:
            ql = np.zeros(1, np.uint8)
        if _trim is not None:                         # `pack_records_trim`
            self._check(self._lib.nrv_pack_records_trim(*_marshal((self._h, s, ql, off, nr, nm, name_off) + _trim + (blob, rec_off),
                                                                  _PACK_RECORDS_TRIM_T)))
            return blob[:int(rec_off[-1])], rec_off
        self._check(self._lib.nrv_pack_records(*_marshal((self._h, s, ql, off, nr, nm, name_off, blob, rec_off), _PACK_RECORDS_T)))
        return blob[:int(rec_off[-1])], rec_off

    @staticmethod
    def _fingerprint(a):
        """Identity + shape + a checksum of the WHOLE contents: the facade must not serve stale results when a
        caller edits the same array object in place between model1.predict and model2.predict (xxh3 runs at
        > 10 GB/s: ~20 ms for the 190 MB of a 64 k-window read, far below the prediction it guards)."""
        v = np.ascontiguousarray(np.asarray(a))
        raw = v.reshape(-1).view(np.uint8)
        try:
            import xxhash
            digest = xxhash.xxh3_64_intdigest(memoryview(raw))
        except ImportError:                                   # pragma: no cover
            import zlib
            digest = zlib.crc32(memoryview(raw))
        return (id(a), v.shape, v.dtype.str, digest)

    def _cached_pair(self, signal_x, read_x, batch_size):
        key = (self._fingerprint(signal_x), self._fingerprint(read_x))
        if self._cache_key != key:
            self._cache_val = self.predict_pair(signal_x, read_x, batch_size)
            self._cache_key = key
        return self._cache_val

    # ------------------------------------------------------------------ device-pointer API
    def predict_device(self, d_signal: int, d_read: int, n: int, d_p1: int = 0, d_p2: int = 0,
                       d_a1: int = 0, d_a2: int = 0):
        """Raw device pointers (ints), asynchronous on the handle's stream."""
        self._check(self._lib.nrv_predict_device(self._h, d_signal, d_read, int(n), d_p1 or None,
                                                 d_p2 or None, d_a1 or None, d_a2 or None))

    def predict_read_device(self, d_sig_ev: int, d_feat_ev: int, N: int, d_p1: int = 0, d_p2: int = 0,
                            d_a1: int = 0, d_a2: int = 0):
        self._check(self._lib.nrv_predict_read_device(self._h, d_sig_ev, d_feat_ev, int(N), d_p1 or None,
                                                      d_p2 or None, d_a1 or None, d_a2 or None))

    def saturated(self):
        """(pending, reruns) of the f16x2 range guard (include/nanorev.h nrv_saturated): `pending` != 0 means
        a device-pointer call since the last check left the f16 range of the signal branch and must be
        repeated in 'f32' precision; `reruns` counts the stages the host entry points already re-ran.
        Synchronises the handle's stream."""
        pend, rer = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.nrv_saturated(self._h, C.byref(pend), C.byref(rer)))
        return int(pend.value), int(rer.value)

    def predict_device_checked(self, d_signal: int, d_read: int, n: int, d_p1: int = 0, d_p2: int = 0,
                               d_a1: int = 0, d_a2: int = 0, read_mode: bool = False) -> bool:
        """`predict_device` / `predict_read_device` + the range guard: synchronises, and when the f16x2 signal
        branch left its range repeats the call on the f32 kernels (same outputs).  Returns True when it did."""
        call = self.predict_read_device if read_mode else self.predict_device
        call(d_signal, d_read, n, d_p1, d_p2, d_a1, d_a2)
        pend, _ = self.saturated()
        if not pend:
            return False
        mode = self.precision
        self.set_precision("f32")
        try:
            call(d_signal, d_read, n, d_p1, d_p2, d_a1, d_a2)
            self.sync()
        finally:
            self.set_precision(mode)
        return True

    def set_batch(self, batch: int):
        self._check(self._lib.nrv_set_batch(self._h, int(batch)))

    @property
    def batch(self) -> int:
        return int(self._lib.nrv_get_batch(self._h))

    def set_precision(self, precision: str):
        """'f16x2' (default: scaled two-term f16 split, three products per f32-grade product), 'bf16x3' (exact
        three-term bf16 split, six products) or 'f32' (plain f32 matrix instructions): include/nanorev.h."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self._check(self._lib.nrv_set_precision(self._h, PRECISIONS[precision]))
        self._cache_key = None

    @property
    def precision(self) -> str:
        v = int(self._lib.nrv_get_precision(self._h))
        return {b: a for a, b in PRECISIONS.items()}[v]

    def set_stream(self, hip_stream: int):
        self._check(self._lib.nrv_set_stream(self._h, hip_stream or None))

    def sync(self):
        self._check(self._lib.nrv_sync(self._h))

    def prof_enable(self, on=True):
        """True/1: every kernel; 2: only the dominant kernel (lstm3); 3: the same on every 8th launch
        group; False/0: off."""
        self._check(self._lib.nrv_prof_enable(self._h, int(on)))

    def prof_read(self):
        ms = (C.c_double * N_KERNELS)()
        cnt = (C.c_int64 * N_KERNELS)()
        self._check(self._lib.nrv_prof_read(self._h, ms, cnt))
        return {self._lib.nrv_kernel_name(k).decode(): (ms[k], int(cnt[k])) for k in range(N_KERNELS)}

    def prof_overhead_us(self) -> float:
        """Microseconds an EMPTY event bracket measures on the launch stream (include/nanorev.h nrv_prof_overhead)."""
        us = C.c_double(0)
        self._check(self._lib.nrv_prof_overhead(self._h, C.byref(us)))
        return float(us.value)

    @property
    def backend(self) -> str:
        return {1: "hip"}[int(self._lib.nrv_backend(self._h))]
