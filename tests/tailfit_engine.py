"""A stand-in for engine.Reviser's nrv_fit_* surface in the host-logic tests of train_cli (no device, no backbone): a window's
"main_out" is a fixed function of its event features, and the fit is nanoreviser_amd/tailfit.py at float32.  It follows
tests/echo_engine.py: host logic only."""
import numpy as np

from nanoreviser_amd import tailfit as tf
from nanoreviser_amd.engine import Reviser


class FitEcho:
    def __init__(self, T):
        self.T = int(T)
        self.flat, self.y = np.zeros((0, 6 * self.T), np.float32), [np.zeros(0, np.uint8), np.zeros(0, np.uint8)]
        self.state, self.opts, self.calls, self.closed = {}, {}, [], False

    pack_bundle = staticmethod(Reviser.pack_bundle)

    def fit_reset(self):
        self.__init__(self.T)

    def fit_count(self):
        return self.flat.shape[0]

    def fit_add_packed(self, packed, labels):
        raw, st, feat, descs, nr, N = packed[:6]
        ev_len = [descs[i].ev_len for i in range(nr)]
        w, y1, y2 = tf.labelled_windows(labels, ev_len, self.T)
        idx = w[:, None] + np.arange(self.T)[None, :]
        rows = np.maximum(np.tanh(feat[idx].reshape(len(w), -1)[:, :6 * self.T] * 0.01) + 0.1, 0).astype(np.float32)
        self.flat = np.concatenate([self.flat, rows])
        self.y = [np.concatenate([self.y[0], y1]), np.concatenate([self.y[1], y2])]
        self.calls.append((nr, int(N), len(w)))
        return len(w)

    def fit_begin(self, model, params=None, opts=None):
        self.state[model] = tf.FitState(np.array(params, np.float32))
        self.opts[model] = opts

    def fit_epoch(self, model, order):
        return tf.epoch(self.flat, self.y[model], self.state[model], order, self.T, 6 - model, self.opts[model], np.float32)

    def fit_eval(self, model, order, want_p=True):
        p, st = tf.evaluate(self.flat, self.y[model], self.state[model].theta, order, self.T, 6 - model, self.opts[model], np.float32)
        return (p if want_p else None), st

    def fit_params(self, model):
        return np.asarray(self.state[model].theta, np.float32), self.state[model].t

    def close(self):
        self.closed = True
