"""tests/bnfit_engine.py's stand-in with the nrv_fit_set_bn_affine surface, for the host-logic tests of train_cli --fit_bn_affine (no
device): while the switch is on the fit is nanoreviser_amd/bnaffine.py at float32 on the stand-in's own set, on the model's moving
statistics or the re-estimated ones."""
import numpy as np

from bnfit_engine import BnEcho
from nanoreviser_amd import bnaffine as ba


class AffineEcho(BnEcho):
    def __init__(self, T, models=None):
        super().__init__(T, models)
        self.affine = False
        self.affine_calls = []

    def fit_reset(self):
        on, calls = self.affine, self.affine_calls
        super().fit_reset()
        self.affine, self.affine_calls = on, calls

    def fit_set_depth(self, depth):
        super().fit_set_depth(depth)
        self.affine = False

    def fit_set_bn_affine(self, on):
        self.affine = bool(on)
        self.affine_calls.append((self.affine, self.fit_count()))
        self.state = {}

    def fit_bn_affine(self):
        return self.affine

    def fit_n_params(self, model):
        return super().fit_n_params(model) + (ba.n_block("full") if self.affine else 0)

    def _stats(self, model):
        st = ba.stats_of(self.models[model])
        for k, v in self.bn_stats.get(model, {}).items():
            st[k] = (v["mean"], v["var"])
        return st

    def fit_bn_reestimate(self, model, rows):
        if not self.affine:
            return super().fit_bn_reestimate(model, rows)
        from nanoreviser_amd import bnfit
        rows = np.asarray(rows, np.int64).reshape(-1)
        self.bn_calls.append((model, rows.copy(), self.state[model].t))
        gb, theta = ba.unpack("full", self.state[model].theta, self.T, 6 - model)
        bn = {k: (gb[k] if k in gb else v[:2]) + v[2:] for k, v in bnfit.bn_of(self.models[model]).items()}
        self.bn_stats[model] = bnfit.reestimate("full", self.feat, self.sig, theta, bn, rows, self.T, 6 - model, 0, np.float32)
        return self.bn_stats[model]

    def fit_epoch(self, model, order):
        if not self.affine:
            return super().fit_epoch(model, order)
        return ba.epoch("full", self.feat, self.sig, self.y[model], self.state[model], order, self._stats(model), self.T, 6 - model,
                        self.opts[model], 0, np.float32)

    def fit_eval(self, model, order, want_p=True):
        if not self.affine:
            return super().fit_eval(model, order, want_p)
        p, st = ba.evaluate("full", self.feat, self.sig, self.y[model], self.state[model].theta, order, self._stats(model), self.T,
                            6 - model, self.opts[model], 0, np.float32)
        return (p if want_p else None), st
