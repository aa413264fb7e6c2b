"""A stand-in for engine.Reviser's nrv_fit_* surface at depth NRV_FIT_FULL in the host-logic tests of train_cli (no device), in
the style of tests/signalfit_engine.py: a window's read features are its events' own (scaled into the range the shipped lstm1
sees), its "samples" a fixed function of them, and the fit is nanoreviser_amd/fullfit.py at float32 with the frozen BatchNorms
of the models it was made with."""
import numpy as np

from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import signalfit as sf
from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.fitdepth import CODES
from tailfit_engine import FitEcho


class FullEcho(FitEcho):
    def __init__(self, T, models=None):
        super().__init__(T)
        self.depth = 0
        self.models = models
        self.feat = np.zeros((0, self.T, 6), np.float32)
        self.sig = np.zeros((0, self.T, 50), np.float32)
        self.depth_calls = []

    def fit_reset(self):
        calls, depth = self.depth_calls, self.depth
        self.__init__(self.T, self.models)
        self.depth_calls, self.depth = calls, depth

    def fit_set_depth(self, depth):
        depth = CODES.get(depth, depth)
        assert self.fit_count() == 0, "nrv_fit_set_depth: the training set is not empty"
        assert depth == 32, "this stand-in only knows the full depth"
        self.depth = int(depth)
        self.depth_calls.append(self.depth)
        self.state = {}

    def fit_depth(self):
        return self.depth

    def fit_count(self):
        return self.feat.shape[0]

    def fit_n_params(self, model):
        return ff.n_params(self.T, 6 - model)

    def fit_add_packed(self, packed, labels):
        raw, st, feat, descs, nr, N = packed[:6]
        w, y1, y2 = tf.labelled_windows(labels, [descs[i].ev_len for i in range(nr)], self.T)
        idx = w[:, None] + np.arange(self.T)[None, :]
        f = feat[idx].reshape(len(w), self.T, -1)
        k, p = np.arange(6), np.arange(50)
        self.feat = np.concatenate([self.feat, np.tanh(f[:, :, k % f.shape[2]] * 0.01).astype(np.float32)])
        self.sig = np.concatenate([self.sig, np.sin(f[:, :, p % f.shape[2]] * 0.05 * (1 + p % 5) + 0.3 * p).astype(np.float32)])
        self.y = [np.concatenate([self.y[0], y1]), np.concatenate([self.y[1], y2])]
        self.calls.append((nr, int(N), len(w)))
        return len(w)

    def fit_begin(self, model, params=None, opts=None):
        assert np.asarray(params).size == self.fit_n_params(model)
        super().fit_begin(model, params, opts)

    def _frozen(self, model):
        m = self.models[model]
        return (ff.read_bn(m), sf.conv_bn(m)) + tuple(l4.bn_scale_shift(m))

    def fit_epoch(self, model, order):
        return ff.epoch(self.feat, self.sig, self.y[model], self.state[model], order, *self._frozen(model), self.T, 6 - model,
                        self.opts[model], 0, np.float32)

    def fit_eval(self, model, order, want_p=True):
        p, st = ff.evaluate(self.feat, self.sig, self.y[model], self.state[model].theta, order, *self._frozen(model), self.T,
                            6 - model, self.opts[model], 0, np.float32)
        return (p if want_p else None), st
