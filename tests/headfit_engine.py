"""A stand-in for engine.Reviser's nrv_fit_* surface at BOTH depths in the host-logic tests of train_cli (no device, no
backbone): at head depth a window's "lstm4 output" is a fixed function of its event features and the fit is
nanoreviser_amd/headfit.py at float32; at tail depth it is tests/tailfit_engine.py's FitEcho unchanged."""
import numpy as np

from nanoreviser_amd import headfit as hf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.fitdepth import CODES
from tailfit_engine import FitEcho


class HeadEcho(FitEcho):
    def __init__(self, T, depth=0):
        super().__init__(T)
        self.depth = depth
        self.x = np.zeros((0, self.T, 128), np.float32)
        self.depth_calls = []

    def fit_reset(self):
        calls = self.depth_calls
        self.__init__(self.T, self.depth)
        self.depth_calls = calls

    def fit_set_depth(self, depth):
        depth = CODES.get(depth, depth)
        assert self.fit_count() == 0, "nrv_fit_set_depth: the training set is not empty"
        self.depth = int(depth)
        self.depth_calls.append(self.depth)
        self.state = {}

    def fit_depth(self):
        return self.depth

    def fit_count(self):
        return self.x.shape[0] if self.depth else super().fit_count()

    def fit_n_params(self, model):
        return (hf if self.depth else tf).n_params(self.T, 6 - model)

    def fit_add_packed(self, packed, labels):
        if not self.depth:
            return super().fit_add_packed(packed, labels)
        raw, st, feat, descs, nr, N = packed[:6]
        w, y1, y2 = tf.labelled_windows(labels, [descs[i].ev_len for i in range(nr)], self.T)
        idx = w[:, None] + np.arange(self.T)[None, :]
        f = feat[idx].reshape(len(w), self.T, -1)                                # [rows][T][features of the event]
        k = np.arange(128)
        rows = np.tanh(f[:, :, k % f.shape[2]] * 0.01 * (1 + k % 7) - 0.2 * (k % 3)).astype(np.float32)
        self.x = np.concatenate([self.x, rows])
        self.y = [np.concatenate([self.y[0], y1]), np.concatenate([self.y[1], y2])]
        self.calls.append((nr, int(N), len(w)))
        return len(w)

    def fit_begin(self, model, params=None, opts=None):
        assert np.asarray(params).size == self.fit_n_params(model)
        super().fit_begin(model, params, opts)

    def fit_epoch(self, model, order):
        if not self.depth:
            return super().fit_epoch(model, order)
        return hf.epoch(self.x, self.y[model], self.state[model], order, self.T, 6 - model, self.opts[model], np.float32)

    def fit_eval(self, model, order, want_p=True):
        if not self.depth:
            return super().fit_eval(model, order, want_p)
        p, st = hf.evaluate(self.x, self.y[model], self.state[model].theta, order, self.T, 6 - model, self.opts[model], np.float32)
        return (p if want_p else None), st
