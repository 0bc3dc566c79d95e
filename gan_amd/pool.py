"""Image history pool of the CycleGAN discriminators (Zhu et al. 2017): the storage and the device state of
one pool, and the one launch that queries it (include/gan_amd.h, gan_pool_exchange)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

STREAM_Y, STREAM_X = 32, 33      # stream ids of pool_y (fake_y, for D_y) and pool_x (fake_x, for D_x)


class ImagePool:
    """`capacity` generated images of size x size x channels in the compute dtype, dense, allocated once, and the int32 state
    {stored, launches, ticket} the launches advance themselves.  A pool belongs to the model, not to a step: steps of different
    batch sizes (a last partial batch) query the same pool."""

    def __init__(self, ctx, size, channels, capacity, seed, stream_id):
        if int(capacity) < 1:
            raise ValueError(f"pool capacity {capacity!r}: at least 1")
        self.ctx, self.size, self.channels, self.capacity = ctx, int(size), int(channels), int(capacity)
        self.seed, self.stream_id = int(seed), int(stream_id)
        self.storage = torch.zeros((self.capacity, self.size, self.size, self.channels), dtype=ctx.tdtype, device=ctx.device)
        self.state = torch.zeros(3, dtype=torch.int32, device=ctx.device)

    def reset(self):
        """Empty again: the next `capacity` images fill it, the launch counter restarts the decision sequence."""
        self.storage.zero_()
        self.state.zero_()

    def tensors(self):
        """What a query changes (base_gan._step_state saves and restores it around a capture's warm-up pass)."""
        return [self.state, self.storage]

    def exchange(self, src_view, dst_view):
        """dst_view <- the images the discriminator sees for the current ones in src_view (GanTensor views of n images); one launch
        on the current stream."""
        if (src_view.h, src_view.w, src_view.c) != (self.size, self.size, self.channels):
            raise ValueError(f"pool of {self.size} x {self.size} x {self.channels} images queried with "
                             f"{src_view.h} x {src_view.w} x {src_view.c}")
        d = L.GanPoolDesc(self.ctx.dt, src_view, dst_view, self.storage.data_ptr(), self.capacity, self.stream_id, self.seed,
                          self.state.data_ptr())
        L.check(self.ctx.lib.gan_pool_exchange(C.byref(d), self.ctx.stream()), "pool_exchange")
