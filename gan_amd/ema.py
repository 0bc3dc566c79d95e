"""Exponential moving average of a generator's weights (no counterpart in the reference, off by default).

`WeightAverage` keeps `shadow`, a second fp32 arena beside `ParamSet.master`, and moves it towards the weights with one
gan_ema_update launch per step: shadow += (master - shadow) * (1 - d_t), d_t = decay or, with warm-up, min(decay, (1 + t) /
(10 + t)) with t the device-resident Adam step count (tf.train.ExponentialMovingAverage's num_updates form).  The launch is
enqueued behind the step (gan_amd/steps.py: after the step's graph, never inside a capture); `averaged()` lends the shadow to the
model for validation and prediction."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import _lib as L
from .checkpoint import tf_variable_key

DECAY_KEY = 'decay/.ATTRIBUTES/VARIABLE_VALUE'


class WeightAverage:
    def __init__(self, model, decay=0.999, warmup=True):
        """model: a GeneratorModel.  decay in [0, 1); warmup: d_t = min(decay, (1 + t) / (10 + t))."""
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"decay {decay!r} is outside [0, 1)")
        self.model, self.params = model, model.net.params
        self.decay, self.warmup = decay, bool(warmup)
        self.layers = model.layers                       # (the checkpoint names this object's variables as the model's)
        self.shadow = self.params.master.clone()
        self.loaded = False                              # load_state_dict found averaged weights
        self._lent = False

    def update(self):
        """One launch on the current stream, behind everything already queued there (the step's Adam launches)."""
        if self._lent:
            raise L.GanAmdError("WeightAverage.update() inside averaged(): master holds the averaged weights")
        ps = self.params
        rc = ps.ctx.lib.gan_ema_update(self.shadow.data_ptr(), ps.master.data_ptr(), ps.total, self.decay,
                                       ps.step.data_ptr() if self.warmup else None, None, ps.ctx.stream())
        L.check(rc, "ema_update")

    def _exchange(self):
        """master <-> shadow by contents: both tensors stay where they are, so captured graphs keep their pointers."""
        ps = self.params
        tmp = ps.master.clone()
        ps.master.copy_(self.shadow)
        self.shadow.copy_(tmp)
        ps.prepare()

    @contextlib.contextmanager
    def averaged(self):
        """Inside: the model's weights (master and the typed copies) ARE the averaged ones, so fold() / infer / infer_tiled /
        model(x, training=False) predict from the average; afterwards, also after an exception, the raw weights are back bit for
        bit.  BatchNorm's moving statistics are not averaged (they are moving averages already): the current ones are used."""
        if self._lent:
            raise L.GanAmdError("WeightAverage.averaged() is not re-entrant")
        self._exchange()
        self._lent = True
        try:
            yield self.model
        finally:
            self._lent = False
            self._exchange()

    # ---- checkpoint object (gan_amd/checkpoint.py): the model's own variable naming, trainable variables only ----------------
    def _key(self, name):
        return tf_variable_key('ema', self.layers, name).split('/', 1)[1]

    def _tensor(self, name):
        o, shape = self.params.entries[name]
        return self.shadow[o:o + int(np.prod(shape))].view(shape)

    def state_dict(self):
        out = {self._key(n): self._tensor(n).detach().cpu().numpy().copy() for n in self.params.entries}
        out[DECAY_KEY] = np.float32(self.decay)
        return out

    def load_state_dict(self, sd):
        """No averaged variable among `sd` (a checkpoint written without EMA): the average starts over from the model's current
        weights - restore the model first - and `loaded` is False.  The decay of this run, not the stored one, stays in force."""
        found = [n for n in self.params.entries if self._key(n) in sd]
        self.shadow.copy_(self.params.master)            # (also fills the alignment padding between the variables)
        for n in found:
            self._tensor(n).copy_(torch.from_numpy(np.array(sd[self._key(n)], dtype=np.float32)).view(self.params.entries[n][1]))
        self.loaded = bool(found)
