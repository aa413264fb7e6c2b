"""A stand-in for engine.Reviser's nrv_fit_* surface at depth NRV_FIT_LSTM4 in the host-logic tests of train_cli (no device, no
backbone), in the style of tests/headfit_engine.py: a window's "BatchNorm'd lstm3 output" is a fixed function of its event
features and the fit is nanoreviser_amd/lstm4fit.py at float32."""
import numpy as np

from nanoreviser_amd import lstm4fit as lf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.fitdepth import CODES
from tailfit_engine import FitEcho


class Lstm4Echo(FitEcho):
    def __init__(self, T):
        super().__init__(T)
        self.depth = 0
        self.xb = np.zeros((0, self.T, 256), np.float32)
        self.depth_calls = []

    def fit_reset(self):
        calls, depth = self.depth_calls, self.depth
        self.__init__(self.T)
        self.depth_calls, self.depth = calls, depth

    def fit_set_depth(self, depth):
        depth = CODES.get(depth, depth)
        assert self.fit_count() == 0, "nrv_fit_set_depth: the training set is not empty"
        assert depth == 4, "this stand-in only knows the lstm4 depth"
        self.depth = int(depth)
        self.depth_calls.append(self.depth)
        self.state = {}

    def fit_depth(self):
        return self.depth

    def fit_count(self):
        return self.xb.shape[0]

    def fit_n_params(self, model):
        return lf.n_params(self.T, 6 - model)

    def fit_add_packed(self, packed, labels):
        raw, st, feat, descs, nr, N = packed[:6]
        w, y1, y2 = tf.labelled_windows(labels, [descs[i].ev_len for i in range(nr)], self.T)
        idx = w[:, None] + np.arange(self.T)[None, :]
        f = feat[idx].reshape(len(w), self.T, -1)
        k = np.arange(256)
        rows = (2 * np.tanh(f[:, :, k % f.shape[2]] * 0.01 * (1 + k % 7) - 0.2 * (k % 3))).astype(np.float32)
        self.xb = np.concatenate([self.xb, rows])
        self.y = [np.concatenate([self.y[0], y1]), np.concatenate([self.y[1], y2])]
        self.calls.append((nr, int(N), len(w)))
        return len(w)

    def fit_begin(self, model, params=None, opts=None):
        assert np.asarray(params).size == self.fit_n_params(model)
        super().fit_begin(model, params, opts)

    def fit_epoch(self, model, order):
        return lf.epoch(self.xb, self.y[model], self.state[model], order, self.T, 6 - model, self.opts[model], 0, np.float32)

    def fit_eval(self, model, order, want_p=True):
        p, st = lf.evaluate(self.xb, self.y[model], self.state[model].theta, order, self.T, 6 - model, self.opts[model], 0, np.float32)
        return (p if want_p else None), st
