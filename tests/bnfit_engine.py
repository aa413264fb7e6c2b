"""tests/fullfit_engine.py's stand-in with the nrv_fit_bn_* surface, for the host-logic tests of train_cli --bn_reestimate (no
device): the re-estimation is nanoreviser_amd/bnfit.py at float32 on the stand-in's own set, and every epoch and evaluation behind
it runs on the re-estimated BatchNorms."""
import numpy as np

from fullfit_engine import FullEcho
from nanoreviser_amd import bnfit
from nanoreviser_amd import fullfit as ff
from nanoreviser_amd import lstm4fit as l4
from nanoreviser_amd import signalfit as sf


class BnEcho(FullEcho):
    def __init__(self, T, models=None):
        super().__init__(T, models)
        self.bn_stats = {}
        self.bn_calls = []

    def fit_reset(self):
        stats, calls = self.bn_stats, self.bn_calls
        super().fit_reset()
        self.bn_stats, self.bn_calls = stats, calls

    def fit_begin(self, model, params=None, opts=None):
        super().fit_begin(model, params, opts)
        self.bn_stats.pop(model, None)

    def fit_bn_reestimate(self, model, rows):
        rows = np.asarray(rows, np.int64).reshape(-1)
        assert model in self.state, "nrv_fit_bn_reestimate: no fit in progress for this model"
        assert rows.size > 0 and rows.max() < self.fit_count()
        self.bn_calls.append((model, rows.copy(), self.state[model].t))
        self.bn_stats[model] = bnfit.reestimate("full", self.feat, self.sig, self.state[model].theta, bnfit.bn_of(self.models[model]),
                                                rows, self.T, 6 - model, 0, np.float32)
        return self.bn_stats[model]

    def fit_bn_stats(self, model):
        return self.bn_stats[model]

    def _frozen(self, model):
        m = self.models[model]
        if model in self.bn_stats:
            m = bnfit.with_stats(m, self.bn_stats[model])
        return (ff.read_bn(m), sf.conv_bn(m)) + tuple(l4.bn_scale_shift(m))
