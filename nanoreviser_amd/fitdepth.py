"""The fit depths of nrv_fit_* in depth order: one table for the engine binding, the command line and the tools.  The
definitions stay where they are - tailfit.py .. fullfit.py; include/nanorev.h states the engine's side."""
from __future__ import annotations

import importlib
from typing import Callable, NamedTuple, Tuple

import numpy as np


class Rows(NamedTuple):
    """One float array of the set: the doors' arguments for it - two for a per-model array, one for an array both models
    share -, its shape behind the row index at window length T."""
    args: Tuple[str, ...]
    shape: Callable[[int], Tuple[int, ...]]
    shared: bool


class Depth(NamedTuple):
    name: str                 # as --fit_depth and Reviser.fit_set_depth take it
    code: int                 # NRV_FIT_*
    module: str               # the defining module
    suffix: str               # of the nrv_fit_set_rows* / nrv_fit_get_rows* doors
    rows: Tuple[Rows, ...]    # the float arrays of a row, in door order
    front: int                # parameters this depth puts in front of the depth before it
    bn: int = 0               # NRV_FIT_PARAMS_BN: the gamma / beta block in front of the vector while fit_set_bn_affine is on

    @property
    def fit(self):
        """The defining module."""
        return importlib.import_module("." + self.module, __package__)

    def door_args(self):
        return tuple(a for r in self.rows for a in r.args)

    def door_shapes(self, T):
        return tuple(r.shape(T) for r in self.rows for _ in r.args)


DEPTHS = (
    Depth("tail", 0, "tailfit", "", (Rows(("flat1", "flat2"), lambda T: (6 * T,), False),), 0),
    Depth("head", 1, "headfit", "_head", (Rows(("x1", "x2"), lambda T: (T, 128), False),), 20838),
    Depth("lstm4", 4, "lstm4fit", "_lstm4", (Rows(("xb1", "xb2"), lambda T: (T, 256), False),), 164352),
    Depth("lstm3", 8, "lstm3fit", "_lstm3", (Rows(("x1", "x2"), lambda T: (T, 192), False),), 328704, 512),
    Depth("signal", 16, "signalfit", "_signal",
          (Rows(("x2_1", "x2_2"), lambda T: (T, 128), False), Rows(("sig",), lambda T: (T, 50), True)), 25896, 544),
    Depth("full", 32, "fullfit", "_full", (Rows(("sig",), lambda T: (T, 50), True), Rows(("feat",), lambda T: (T, 6), True)), 52608, 864),
)
BY_NAME = {d.name: d for d in DEPTHS}
BY_CODE = {d.code: d for d in DEPTHS}
CODES = {d.name: d.code for d in DEPTHS}


def start_vector(depth, model, behind):
    """`behind`, a vector of the head depth's layout, with the front of every depth from lstm4 back to `depth` (a name) in front
    of it, each front the model's own tensors as that depth's params_from_model has them.  At tail and head depth: `behind`."""
    th = np.asarray(behind, np.float32)
    names = [d.name for d in DEPTHS]
    for d in DEPTHS[names.index("lstm4"):names.index(depth) + 1]:
        th = np.concatenate([d.fit.params_from_model(model)[:d.front], th])
    return th
