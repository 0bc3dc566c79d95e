"""Differentiable augmentation of the discriminator inputs (Zhao et al. 2020): the per-image parameter table,
the counter of its draws, and the launches that fill and apply it (include/gan_amd.h, gan_diffaug_draw / gan_diffaug_apply)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

POLICIES = ('translation', 'cutout', 'brightness', 'saturation')      # bit k of the policy mask (GAN_DIFFAUG_*)
STREAM = 48                       # stream id of the draws (the dropout masks use 0..5 / 16..21 / 40 times 8, the pools 32 and 33)
MAX_RECORDS = 128                 # of one gan_diffaug_draw launch


def parse_policies(text):
    """'translation,cutout' -> ('translation', 'cutout') in POLICIES order; '' or None -> ().  ValueError on an unknown name."""
    if text is None or isinstance(text, str) and not text.strip():
        return ()
    names = [n.strip() for n in text.split(',')] if isinstance(text, str) else [str(n) for n in text]
    bad = [n for n in names if n not in POLICIES]
    if bad:
        raise ValueError(f"unknown augmentation {bad[0]!r}: a comma-separated subset of {', '.join(POLICIES)}")
    return tuple(p for p in POLICIES if p in names)


def policy_mask(policies):
    return sum(1 << POLICIES.index(p) for p in parse_policies(policies))


class DiffAugment:
    """The policies of one step, the device table of GanDiffAugParams records (one per image a discriminator invocation sees) and
    the int32 launch counter the draw launch advances itself - its own, not an Adam step counter: the optimiser's counter moves in
    the middle of a step on another lane.  One draw() per step writes the table; every apply() of that step only reads it."""

    def __init__(self, ctx, policies, seed=123, stream_id=STREAM):
        self.ctx, self.policies = ctx, parse_policies(policies)
        if not self.policies:
            raise ValueError("DiffAugment without a policy: pass diffaug=None instead")
        self.mask = policy_mask(self.policies)
        seed = int(seed)
        try:        # data-parallel replicas draw differently (the hash mixes the rank in through the seed, as the dropout masks do)
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                seed = (seed + 0x9E3779B1 * dist.get_rank()) & 0x7FFFFFFFFFFFFFFF
        except Exception:
            pass
        self.seed, self.stream_id = seed, int(stream_id)
        self.table = torch.zeros((MAX_RECORDS, 8), dtype=torch.int32, device=ctx.device)       # 32-byte records
        self.launches = torch.zeros(1, dtype=torch.int32, device=ctx.device)

    def tensors(self):
        """What a step changes (base_gan._step_state saves and restores it around a capture's warm-up pass)."""
        return [self.launches, self.table]

    def draw(self, n, h, w):
        """Records 0 .. n-1 <- fresh draws for h x w images; one launch on the current stream."""
        if not 1 <= n <= MAX_RECORDS:
            raise ValueError(f"{n} records: 1 ..= {MAX_RECORDS} (a batch of at most {MAX_RECORDS // 2} with real and generated halves)")
        L.check(self.ctx.lib.gan_diffaug_draw(self.table.data_ptr(), n, h, w, self.mask, self.seed, self.stream_id,
                                              self.launches.data_ptr(), self.ctx.stream()), "diffaug_draw")

    def apply(self, src_view, dst_view, group_c, sample0, backward=False, stream=None):
        """dst_view <- T(src_view) (backward: the transpose) with records sample0 .. of the table; one launch."""
        d = L.GanDiffAugDesc(self.ctx.dt, src_view, dst_view, group_c, sample0, self.table.data_ptr(), int(bool(backward)))
        L.check(self.ctx.lib.gan_diffaug_apply(C.byref(d), stream.cuda_stream if stream is not None else self.ctx.stream()),
                "diffaug_apply")

    def records(self, n):
        """The first n records as a list of dicts (a synchronising read-back: tests and diagnostics)."""
        raw = self.table[:n].cpu()
        f = raw[:, 6:8].contiguous().view(torch.float32)
        keys = ('tx', 'ty', 'cut_x0', 'cut_y0', 'cut_w', 'cut_h')
        return [dict(zip(keys, (int(v) for v in raw[i, :6])), brightness=float(f[i, 0]), saturation=float(f[i, 1])) for i in range(n)]
