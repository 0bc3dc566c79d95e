"""Device-side train steps: the whole of `Pix2Pix.train_step` (pix2pix.py:190-218) and
`CycleGAN.train_step` (cycle_gan.py:206-276) as sequences of C-ABI kernel launches — forward, losses,
explicit backward and TF-form Adam all on the GPU, optionally captured once into a hipGraph and replayed.

Semantics kept from the reference: both gradients are taken at the pre-update weights from a single
forward (simultaneous update); D(real) and D(fake) are separate BatchNormalization invocations (separate
batch statistics, two moving-average updates); dropout is active in every generator call; `training=False`
computes forward + losses only (pix2pix.py:208, :291-292).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from enum import IntEnum
from typing import NamedTuple

import torch

from . import _lib as L
from .diffaug import MAX_RECORDS
from .nets import Buf, Ctx, DiscriminatorNet, GeneratorNet, LrSchedule


# Other threads of the process may call into the runtime while a step is being captured (the RCCL watchdog of
# torch.distributed polls its events): only calls of the CAPTURING thread may invalidate the capture.
CAPTURE_MODE = "thread_local"


class Phase(IntEnum):
    """Which part of the forward + backward pass one _forward_backward call enqueues.  The data-parallel schedules cut the step
    where a network's gradients become complete (ddp_phases) and capture one compute graph per phase."""
    FULL = 0            # the whole pass (one-GPU step, eager data-parallel step)
    GENS = 1            # everything but the discriminators' parameter passes: the generator(s) complete
    DISCS = 2           # the discriminators' parameter passes
    HEAD = 3            # Pix2Pix, bucketed: up to D's input-gradient pass; the caller stages G's backward itself
    SERIAL_GG = 11      # CycleGAN merged, one chain: up to G_g's second backward (G_g complete)
    SERIAL_GF = 12      # ... G_f's second backward
    SERIAL_DX = 13      # ... D_x's parameter pass
    SERIAL_DY = 14      # ... D_y's parameter pass
    CHAINS_GENS = 21    # CycleGAN merged, two chains: up to both generators' second backward
    CHAINS_DISCS = 22   # ... both discriminators' parameter passes, one per chain


class _Mode(NamedTuple):
    """What surrounds one _forward_backward call; _run decides it once.  The default is a bare call (tests, the data-parallel
    compute graphs): nothing is being captured and no part of the update is scheduled inside."""
    update: bool = False        # a full training step: parts of the Adam update may be scheduled inside the backward pass
    capturing: bool = False     # the call is being captured into the replayed graph
    fuse_adam: bool = False     # the wgrad launches carry Adam (GanAdamFuse): update and capturing and _wgrad_adam_ok() - such a
                                # schedule leaves no fp32 gradients behind, so it is for the replayed step only


class _InStepAdam:
    """What _forward_backward has already done to the optimiser in this step; _update() does the rest and clears the record."""

    def __init__(self):
        self.done = ()          # networks fully updated (at the end of their own backward chain)
        self.wfused = {}        # network -> the kernels that its wgrad launches updated themselves

    clear = __init__

    def __bool__(self):
        return bool(self.done or self.wfused)


class _StepBase:
    ddp_buckets = False          # data parallel: a step type with a bucketed schedule (_capture_bucketed) turns it on

    def __init__(self, ctx: Ctx, batch, size, channels, lam, lr, beta_1, beta_2, n_losses, gan_loss='bce'):
        if gan_loss not in ('bce', 'lsgan'):
            raise ValueError(f"gan_loss {gan_loss!r}: 'bce' or 'lsgan'")
        self.gan_loss = gan_loss     # the adversarial term: sigmoid cross-entropy, or least squares on the raw logits
        self.ctx, self.B, self.S, self.C = ctx, batch, size, channels
        self.lam, self.lr, self.b1, self.b2 = float(lam), lr, beta_1, beta_2
        self.losses = torch.zeros(n_losses, dtype=torch.float32, device=ctx.device)
        self.l1_ws = torch.zeros(4096, dtype=torch.float32, device=ctx.device)
        self.bce_ws = torch.zeros(1024, dtype=torch.float32, device=ctx.device)
        self.sync = None             # GradSync for data-parallel runs
        self.ema = ()                # WeightAverage objects (gan_amd/ema.py) a replayed training step moves, DESIGN.md section 15
        self._in_step = _InStepAdam()

    def _set_lr_schedule(self, schedule):
        """A linear decay of the Adam rate (nets.LrSchedule) for every network of the step: the launch that
        advances a network's step counter then evaluates it on the device, in the same place of every schedule of this file.  None
        leaves the networks as they are: objects shared with another step (nets=...) keep what that step gave them."""
        self.lr_schedule = None
        if schedule is None:
            return
        schedule = LrSchedule(*schedule).validate()
        if float(schedule.lr) != float(self.lr):
            raise ValueError(f"lr_schedule.lr {schedule.lr!r} differs from the step's lr {self.lr!r}")
        self.lr_schedule = schedule
        for net in self.nets():
            net.params.set_lr_schedule(schedule)

    def current_lr(self, net=0):
        """The rate of the last update network `net` (index into nets()) ran, read back from the device: a 4-byte copy that waits
        for the stream - once per epoch, not per step.  Without a schedule, or before the first update: the base rate."""
        P = self.nets()[net].params
        if P.lr_schedule is None:
            return float(self.lr)
        return float(P.lr_now.item())

    def _example_inputs(self):
        sh = (self.B, self.S, self.S, self.C)
        return [torch.zeros(sh, dtype=torch.float32, device=self.ctx.device) for _ in range(2)]

    def _bce(self, logits_ptr, count, target, loss_idx, loss_scale, acc, grad_scale, dx_ptr, ws=None):
        """One adversarial term against a constant target: gan_bce_logits, or (gan_loss 'lsgan') gan_lsq_logits - same arguments."""
        lib, ctx = self.ctx.lib, self.ctx
        fn, what = (lib.gan_lsq_logits, "lsq_logits") if self.gan_loss == 'lsgan' else (lib.gan_bce_logits, "bce_logits")
        rc = fn(logits_ptr, count, target, loss_scale, int(acc), self.losses.data_ptr() + 4 * loss_idx,
                grad_scale, ctx.dt, dx_ptr, 8, (ws if ws is not None else self.bce_ws).data_ptr(), ctx.ls_ptr, ctx.stream())
        L.check(rc, what)

    def _l1(self, a, b, loss_idx, loss_scale, acc, grad_scale, da, stream=None, ws=None):
        lib, ctx = self.ctx.lib, self.ctx
        rc = lib.gan_l1(ctx.dt, C.byref(a), C.byref(b), loss_scale, int(acc), self.losses.data_ptr() + 4 * loss_idx,
                        grad_scale, C.byref(da) if da is not None else None, (ws if ws is not None else self.l1_ws).data_ptr(), ctx.ls_ptr,
                        stream.cuda_stream if stream is not None else ctx.stream())
        L.check(rc, "l1")

    def _pack_multi(self, pairs):
        """[(src_f32, dst_view), ...] (<= 4, one shape) in a single launch."""
        n = len(pairs)
        srcs = (C.c_void_p * n)(*[s_.data_ptr() for s_, _ in pairs])
        dsts = (L.GanTensor * n)(*[d_ for _, d_ in pairs])
        L.check(self.ctx.lib.gan_pack_multi(self.ctx.dt, n, srcs, dsts, self.ctx.stream()), "pack_multi")

    def _copy(self, src_view, dst_view):
        L.check(self.ctx.lib.gan_copy_view(self.ctx.dt, C.byref(src_view), C.byref(dst_view), self.ctx.stream()), "copy_view")

    def _run(self, a, b, training=True, capturing=False):
        training = bool(training)
        mode = _Mode(update=training, capturing=capturing, fuse_adam=training and capturing and self._wgrad_adam_ok())
        self._forward_backward(a, b, training, mode=mode)
        if training:
            if self.sync is not None:
                self.sync(unpack=not self._wire_adam())    # data-parallel gradient exchange (RCCL)
            self._update()
        return self.losses

    def _wire_adam(self):
        """Data-parallel, bf16 wire: Adam reads the exchanged gradient from the wire buffers (no unpack pass).  Not with fp16
        loss scaling: its inf/nan check must see the EXCHANGED gradients (every rank takes the same skip decision), which
        the unpacked fp32 buffers hold."""
        s_ = self.sync
        return s_ is not None and getattr(s_, 'compress', False) and getattr(s_, 'wire', None) is not None and self.ctx.ls is None

    def _update(self):
        gs = self.sync.grad_scale if self.sync is not None else 1.0
        wire = self._wire_adam()
        if wire:
            gs = 1.0 / self.sync.world
        wp = lambda net: (self.sync.wire[self.nets().index(net)].data_ptr() if wire else None)
        ctx, did = self.ctx, self._in_step
        if ctx.ls is not None:        # fp16: a non-finite gradient anywhere skips the whole step (every network), then the scale adapts
            for net in self.nets():
                ctx.run(net.params.grads_check_ops())
        for net in self.nets():
            if net in did.done:        # updated at the end of its own backward chain
                continue
            if net in did.wfused:      # its big kernels were updated by their own wgrad launches (GanAdamFuse): the rest + the vectors
                ctx.run(net.params.adam_rest_ops(did.wfused[net], self.b1, self.b2))
            else:
                net.params.adam(self.lr, self.b1, self.b2, grad_scale=gs, wire_ptr=wp(net))
        if ctx.ls is not None:
            L.check(ctx.lib.gan_loss_scale_update(ctx.ls_ptr, ctx.ls_growth_interval, ctx.ls_max, ctx.stream()), "loss_scale_update")
        did.clear()

    def _wgrad_adam_ok(self):
        """GanAdamFuse schedules: one GPU, no loss scaling, 16-bit storage."""
        return bool(self.fused_wgrad_adam and self.sync is None and self.ctx.ls is None and self.ctx.dtype != 'f32')

    def _adam_in_chains(self, mode):
        """Nothing else is pending between the backward pass and the update (one GPU, no loss scaling): in a full step a
        network's Adam may run where its gradients complete, at the end of its own chain."""
        return mode.update and self.sync is None and self.ctx.ls is None

    def _prebuild_fused_adam(self):
        pass

    # ---- hipGraph capture of a whole step --------------------------------------------------------
    def _warm_up(self, fn):
        """fn() once eagerly on a side stream: lazy inits, func attributes, op lists, device tables and layer-stack plans are built
        (and uploaded) outside the captures."""
        main = torch.cuda.current_stream(self.ctx.device)
        s = torch.cuda.Stream(device=self.ctx.device)
        s.wait_stream(main)
        with torch.cuda.stream(s):
            fn()
        main.wait_stream(s)
        torch.cuda.synchronize()

    def _graph(self, fn):
        return self.ctx.capture_graph(fn, CAPTURE_MODE)      # (an exception inside leaves no forked lane behind: Ctx.capture_graph)

    def _replayer(self, body, training):
        """The callable that capture() returns: inputs -> the static buffers, body(), the losses.  A training step then moves the
        weight averages attached to it (self.ema): one launch each on the stream the graph(s) were launched on, which every
        schedule's body ends joined onto, so stream order puts it behind every Adam launch of the step - and outside every capture."""
        def replay(*inputs):
            for dst, src in zip(self._static_in, inputs):
                if src is not dst:
                    dst.copy_(src, non_blocking=True)
            body()
            if training:
                for e in self.ema:
                    e.update()
            return self.losses
        replay.inputs = self._static_in      # a caller that fills these buffers itself (and passes them back) skips the copies
        return replay

    def capture(self, training=True):
        """Capture one full step on static input buffers; returns a callable replaying it.  With a gradient
        exchange attached the step becomes graph(forward+backward) -> collectives -> graph(Adam)."""
        self._static_in = [torch.zeros_like(t) for t in self._example_inputs()]
        torch.cuda.synchronize()
        self._warm_up(lambda: self._run(*self._static_in, training=training))
        split = training and self.sync is not None and getattr(self.sync, 'active', self.sync.world > 1)
        if split and self.ddp_buckets and self.ctx.lanes and self.ctx.ls is None:
            return self._capture_bucketed()          # (fp16: the whole-step inf/nan check precedes every Adam -> phased schedule)
        if split:
            return self._capture_phased(training)
        if training:
            self._prebuild_fused_adam()         # (op lists and device tables of the captured schedule: no uploads inside the capture)
        g1 = self._graph(lambda: self._run(*self._static_in, training=training, capturing=True))
        self._graphs = (g1, None, None)
        return self._replayer(g1.replay, training)

    def _capture_phased(self, training):
        """Data-parallel schedule by PHASES (every step type has it; Pix2Pix bf16 prefers its finer bucketed schedule): the step is
        cut where a network's gradients become complete - ddp_phases() lists (Phase, networks complete after it) in the order
        the backward pass finishes them (cycle_gan.py:252-260 has four independent gradient sets) - one compute graph per phase;
        a finished network's exchange starts at once on the communicator's stream and runs beside the following phases; its Adam
        graph is replayed on a side stream as soon as the exchange has landed.  fp16: the inf/nan check must see every EXCHANGED
        gradient before any weight moves (all ranks take the same skip decision), so the exchanges still overlap the compute
        phases but one graph at the end checks, updates every network and adapts the loss scale."""
        ctx, sync = self.ctx, self.sync
        phases = self.ddp_phases()
        nets = self.nets()
        fp16 = ctx.ls is not None
        wire = self._wire_adam()
        lane4 = ctx.lane_stream(4)
        self._warm_up(lambda: [self._forward_backward(*self._static_in, training, phase=pid) for pid, _ in phases])
        G = [self._graph(lambda pid=pid: self._forward_backward(*self._static_in, training, phase=pid)) for pid, _ in phases]
        if fp16:
            A = [self._graph(self._update)]
        else:
            gs = 1.0 / sync.world if wire else sync.grad_scale
            wp = (lambda i: sync.wire[i].data_ptr()) if wire else (lambda i: None)
            A = [self._graph(lambda i=i, n=n: n.params.adam(self.lr, self.b1, self.b2, grad_scale=gs, wire_ptr=wp(i))) for i, n in enumerate(nets)]
        self._graphs = tuple(G + A)
        evs = [torch.cuda.Event() for _ in G]
        comm = torch.cuda.Stream(device=ctx.device)

        def boundary(k, pending):
            done = phases[k][1]
            if not done:
                return
            comm.wait_event(evs[k])
            with torch.cuda.stream(comm):
                for i in done:
                    sync.pack(i)                               # fp32 gradients -> wire format (no-op for the fp32 wire)
                started = [(i, sync.start(i)) for i in done]
            if fp16:
                pending += started
                return
            lane4.wait_event(evs[k])
            with torch.cuda.stream(lane4):
                for i, h in started:
                    sync.wait(h)                               # lane 4 waits for the collective; the host does not
                    if not wire:
                        sync.unpack(i)
                    A[i].replay()

        def body():
            cur = torch.cuda.current_stream(ctx.device)
            pending = []
            for k, gr in enumerate(G):
                gr.replay()
                evs[k].record(cur)
                if k > 0:
                    boundary(k - 1, pending)                   # issued behind the NEXT compute graph: the GPU never waits for the host
            boundary(len(G) - 1, pending)
            if fp16:
                for i, h in pending:
                    sync.wait(h)
                    sync.unpack(i)
                A[0].replay()
            else:
                ctx.join(cur, lane4)
        return self._replayer(body, training)


class Pix2PixStep(_StepBase):
    # schedule constants (measured); attributes so that an experiment can change them per object
    dreal_on_side_lane = True    # D(real)'s forward on lane 2 beside the generator's launch-bound inner layers (+0.8 %)
    fused_wgrad_adam = True      # captured one-GPU step: the un-split wgrad launches apply Adam to their kernels themselves (GanAdamFuse)
    wgrad_cuts = (4, 8, 12)      # G's wgrad GEMMs in four coarse stages: up7..up4 | up3..up0 | down7..4 | down3..0 (finer: -3 %)
    wgrad_alt = ('down3.kernel', 'down2.kernel', 'down1.kernel', 'down0.kernel')   # kernels of G whose wgrad launches run on a SECOND wgrad lane
                                 # (lane 4, own slab workspace): the last stage's GEMMs beside the optimiser-carrying (HBM-bound) launches of the
                                 # stage before instead of behind them: +1.0 % (5,363 -> 5,421 img/s, two interleaved pairs)
    adam_begin_early = True      # G's gan_adam_begin (step count, lr_t: one tiny launch) at the head of D(real)'s lane instead of on the main chain
                                 # in front of G's backward
    bias_grad_on_side = True     # the bias gradient of G's head (two launches that only feed Adam) as a side-stream op of the first wgrad stage,
                                 # off the dgrad chain
    ddp_buckets = True           # data parallel, bf16/f32: the bucketed schedule (False: the phased one)
    ddp_wire_direct = True       # bf16 all-reduce exchange: wgrad launches write their gradients straight into the wire buffer

    def __init__(self, ctx: Ctx, batch, size, channels=1, lam=100.0, lr=2e-4, beta_1=0.5, beta_2=0.999,
                 seed=123, dropout=True, nets=None, mask_stream=0, generator_loss='l1', gan_loss='bce', lr_schedule=None,
                 diffaug=None, edge_weight=0.0, msssim_alpha=0.84):
        if generator_loss not in ('l1', 'dssim', 'msssim', 'msssim_l1'):
            raise ValueError(f"generator_loss {generator_loss!r}: 'l1', 'dssim', 'msssim' or 'msssim_l1'")
        if not 0.0 < msssim_alpha <= 1.0:
            raise ValueError(f"msssim_alpha {msssim_alpha!r}: a mixing weight in (0, 1]")
        if not edge_weight >= 0.0:
            raise ValueError(f"edge_weight {edge_weight!r}: a weight >= 0")
        super().__init__(ctx, batch, size, channels, lam, lr, beta_1, beta_2, n_losses=8, gan_loss=gan_loss)
        self.generator_loss = generator_loss       # the secondary term (losses[2]): mean |target - gen|, or 1 - mean SSIM
        if generator_loss == 'dssim':
            need = ctx.lib.gan_dssim_workspace_bytes(batch, size, size, channels)
            if not need:
                raise ValueError(f"generator_loss 'dssim': unsupported shape {(batch, size, size, channels)}")
            self.dssim_ws = torch.zeros(need // 4, dtype=torch.float32, device=ctx.device)
        # 1 - mean MS-SSIM over five scales with tf.image.ssim_multiscale's power factors, alone ('msssim') or
        # mixed with L1 ('msssim_l1', Zhao et al. 2017): losses[2] = (1 - alpha) L1 + alpha (1 - MS-SSIM)
        self.msssim_alpha = float(msssim_alpha)
        if generator_loss in ('msssim', 'msssim_l1'):
            self.msssim_scales = len(L.MSSSIM_POWER)
            need = ctx.lib.gan_msssim_workspace_bytes(batch, size, size, channels, self.msssim_scales)
            if not need:
                raise ValueError(f"generator_loss {generator_loss!r}: unsupported shape {(batch, size, size, channels)} for "
                                 f"{self.msssim_scales} scales")
            self.msssim_ws = torch.zeros(need // 4, dtype=torch.float32, device=ctx.device)
        # a second term in the secondary slot: losses[2] = secondary + edge_weight * Sobel edge term, its
        # gradient added into g.dgen behind the secondary loss's; 0: the term's launches are not enqueued at all
        self.edge_weight = float(edge_weight)
        if self.edge_weight > 0.0:
            need = ctx.lib.gan_edge_workspace_bytes(batch, size, size, channels)
            if not need:
                raise ValueError(f"edge_weight: unsupported shape {(batch, size, size, channels)}")
            self.edge_ws = torch.zeros(need // 4, dtype=torch.float32, device=ctx.device)
        if nets is not None:          # share weights with an existing step / model objects
            self.G, self.D = nets
        else:
            self.G = GeneratorNet(ctx, channels, 'batchnorm', seed=seed)          # pix2pix.py:29
            self.D = DiscriminatorNet(ctx, channels, True, 'batchnorm', seed=seed + 1)   # pix2pix.py:30
        self.g = self.G.new_call(batch, size, dropout=dropout, seed=seed, stream_id=mask_stream,   # mask_stream: train / val steps draw different masks
                                 wgrads_on_side_lane=ctx.lanes)
        self.d = self.D.new_call(batch, size, calls=2)
        self._set_lr_schedule(lr_schedule)
        # differentiable augmentation of what D sees (gan_amd/diffaug.py): a training pass stages the raw
        # [input | target] images here, D's input buffer receives their augmented images, and D's input gradient arrives in
        # aug_dgen (D's own, otherwise unused, input-gradient buffer) on its way to the generator
        self.diffaug = diffaug
        if diffaug is not None:
            if 2 * batch > MAX_RECORDS:
                raise ValueError(f"diffaug: batch {batch} needs {2 * batch} records, at most {MAX_RECORDS}")
            self.aug_raw = Buf(ctx, 2 * batch, size, size, 8)
            self.aug_dgen = self.d.dxin

    def nets(self):
        return (self.G, self.D)

    def _dssim(self, a, b, loss_idx, loss_scale, acc, grad_scale, da, stream=None):
        """gan_dssim with _l1's contract: losses[loss_idx] (+)= loss_scale * (1 - mean SSIM(a, b)), da = grad_scale * d/da."""
        ctx = self.ctx
        d = L.GanDssimDesc(ctx.dt, ctx.dt, a, b, loss_scale, int(acc), self.losses.data_ptr() + 4 * loss_idx, grad_scale, ctx.dt,
                           da if da is not None else L.GanTensor(), self.dssim_ws.data_ptr(), self.dssim_ws.numel() * 4, ctx.ls_ptr)
        L.check(ctx.lib.gan_dssim(C.byref(d), stream.cuda_stream if stream is not None else ctx.stream()), "dssim")

    def _msssim(self, a, b, loss_idx, loss_scale, acc, grad_scale, da, stream=None, grad_acc=False):
        """gan_msssim with _l1's contract: losses[loss_idx] (+)= loss_scale * (1 - mean MS-SSIM(a, b)), da (+)= grad_scale * d/da."""
        ctx = self.ctx
        d = L.GanMsssimDesc(ctx.dt, ctx.dt, a, b, loss_scale, int(acc), self.losses.data_ptr() + 4 * loss_idx, grad_scale, ctx.dt,
                            da if da is not None else L.GanTensor(), self.msssim_ws.data_ptr(), self.msssim_ws.numel() * 4, ctx.ls_ptr,
                            self.msssim_scales, L.msssim_power(self.msssim_scales), None, int(grad_acc))
        L.check(ctx.lib.gan_msssim(C.byref(d), stream.cuda_stream if stream is not None else ctx.stream()), "msssim")

    def _msssim_l1(self, a, b, loss_idx, loss_scale, acc, grad_scale, da, stream=None):
        """(1 - alpha) * gan_l1, and directly behind it on the same stream alpha * gan_msssim added to the loss word and to da."""
        al = self.msssim_alpha
        self._l1(a, b, loss_idx, loss_scale * (1.0 - al), acc, grad_scale * (1.0 - al), da, stream=stream)
        self._msssim(a, b, loss_idx, loss_scale * al, True, grad_scale * al, da, stream=stream, grad_acc=da is not None)

    def _edge(self, a, b, loss_idx, loss_scale, acc, grad_scale, da, grad_acc, stream=None):
        """gan_edge_l1 with _l1's contract, and grad_acc: da += grad_scale * d/da instead of da = ..."""
        ctx = self.ctx
        d = L.GanEdgeDesc(ctx.dt, ctx.dt, a, b, loss_scale, int(acc), self.losses.data_ptr() + 4 * loss_idx, grad_scale, ctx.dt,
                          da if da is not None else L.GanTensor(), self.edge_ws.data_ptr(), self.edge_ws.numel() * 4, ctx.ls_ptr,
                          int(grad_acc))
        L.check(ctx.lib.gan_edge_l1(C.byref(d), stream.cuda_stream if stream is not None else ctx.stream()), "edge_l1")

    def _settle_gen_options(self):
        """The options of G's call that shape its backward op lists, taken from this object's switches when the first list is
        about to be built (not earlier: a caller may still set the switches after construction)."""
        if not self.g._bwd_cache:
            self.g.alt_wgrad = frozenset(self.wgrad_alt)
            self.g.bias_grad_on_side = bool(self.bias_grad_on_side and self.ctx.lanes)

    def _prebuild_fused_adam(self):
        if self._wgrad_adam_ok():         # (after the warm-up step: G's options are settled)
            adam = (self.b1, self.b2)
            self.g.bwd_stages(list(self.wgrad_cuts), use_dgen2=True, adam=adam)       # (op lists, layer-stack plans, device tables)
            self.G.params.adam_rest_ops(self.g.bwd_plan(use_dgen2=True, adam=adam).adam_fused, self.b1, self.b2)

    def ddp_phases(self):
        return [(Phase.GENS, [0]), (Phase.DISCS, [1])]          # (phase, indices into nets() complete after it)

    def _forward_backward(self, inp, tar, training=True, phase=Phase.FULL, mode=_Mode()):
        B, Cc, g, d = self.B, self.C, self.g, self.d
        self._settle_gen_options()
        if phase == Phase.DISCS:
            d.backward_params()
            return self.losses
        # inputs -> typed, channel-padded buffers.  D input = concat([inp, tar|gen]) (base_gan.py:139)
        aug = self.diffaug if training else None         # (validation: nothing is augmented, the launches of a step without it)
        xin = self.aug_raw if aug is not None else d.xin
        self._pack_multi([(inp, g.xin.view(0, Cc)), (inp, xin.view(0, Cc, 0, B)), (inp, xin.view(0, Cc, B, B)),
                          (tar, xin.view(Cc, Cc, 0, B))])
        if aug is not None:                               # records 0..B-1: the real samples, B..2B-1: the generated ones
            aug.draw(2 * B, self.S, self.S)
        # (the optimiser-carrying wgrad launches of G's backward need this step's lr_t: nothing before them reads it)
        dreal = bool(self.ctx.lanes and self.dreal_on_side_lane)
        adam_begun = bool(dreal and self.adam_begin_early and phase == Phase.FULL and mode.fuse_adam)
        self._forward_and_losses(dreal, adam_begun, aug)
        if training:
            if aug is not None:                           # ... of the augmented image, carried back through the transform's transpose
                d.backward_input(1, dst=self.aug_dgen.view(0, Cc), c0=Cc)
                aug.apply(self.aug_dgen.view(0, Cc), g.dgen2.view(0, Cc), Cc, B, backward=True)
            else:
                d.backward_input(1, dst=g.dgen2.view(0, Cc), c0=Cc)    # dL_G/d gen through D(fake), pre-update D: the `gen` channels only
            if phase != Phase.HEAD:                                   # (HEAD: the caller stages G's backward)
                self._backward(phase, mode, adam_begun)
        return self.losses                                            # Adam: _update() (pix2pix.py:213-216)

    def _forward_and_losses(self, dreal, begin_adam, aug=None):
        """G, D(real), D(fake) and the four losses with their gradients.  begin_adam: G's gan_adam_begin heads D(real)'s lane.
        aug: the DiffAugment whose table this step has drawn - D's input is the augmented image of the staged raw one (aug_raw)."""
        B, Cc, g, d, ctx = self.B, self.C, self.g, self.d, self.ctx
        main = ctx.lane_stream(0)
        side = ctx.lane_stream(2) if ctx.lanes else None
        raw = self.aug_raw if aug is not None else d.xin             # where the un-augmented [input | target] images are

        def augment_inputs(stream=None, real=True, fake=True):
            if aug is not None and real:      # [input | target] of the real samples: two images per sample, one record
                aug.apply(raw.view(0, 2 * Cc, 0, B), d.xin.view(0, 2 * Cc, 0, B), Cc, 0, stream=stream)
            if aug is not None and fake:      # the input channels of the generated samples (their records also serve the generated channels)
                aug.apply(raw.view(0, Cc, B, B), d.xin.view(0, Cc, B, B), Cc, B, stream=stream)
        if dreal:
            # D(real) does not depend on the generator: it starts on lane 2 when G reaches its inner layers (down3 on:
            # launch-bound layers that leave the chip idle; measured best start point, +0.8 %) and D(fake) follows G on the main chain.  Same
            # BatchNormalization call order (real, then fake) as pix2pix.py:202-203.
            def start_dreal():
                side.wait_stream(main)
                pre = self.G.params.adam_begin_ops(self.lr, self.b1, self.b2) if begin_adam else []
                ctx.run_on(pre, side)
                augment_inputs(side, fake=False)
                ctx.run_on(d.forward_part_ops(0, lane=2), side)
                augment_inputs(side, real=False)                      # (off the main chain; joined below, before D(fake))
            g.forward(inner_hook=start_dreal)                         # pix2pix.py:200
            ctx.join(main, side)                                      # D(real) done (its BatchNorm updates come first)
        else:
            augment_inputs()
            g.forward()                                               # pix2pix.py:200
        # generator loss (pix2pix.py:167-188): BCE(1, D(fake)) + lambda * mean|target - gen| (or, generator_loss 'dssim', lambda *
        # (1 - mean SSIM(gen, target)): same operands, stream and outputs); discriminator loss
        # (base_gan.py:233-245, factor 0.5 at pix2pix.py:206) - the L1 term (it only needs G's output: beside D's
        # forward when lanes are on), then all three BCE terms in one pass
        if side is not None:
            side.wait_stream(main)
        secondary = {'l1': self._l1, 'dssim': self._dssim, 'msssim': self._msssim, 'msssim_l1': self._msssim_l1}[self.generator_loss]
        secondary(g.out_view(), raw.view(Cc, Cc, 0, B), 2, 1.0, False, self.lam, g.dgen.view(0, Cc), stream=side)
        if self.edge_weight > 0.0:          # losses[2] += w * edge, g.dgen += lam * w * d edge / d gen: same stream, same operands
            self._edge(g.out_view(), raw.view(Cc, Cc, 0, B), 2, self.edge_weight, True, self.lam * self.edge_weight, g.dgen.view(0, Cc),
                       True, stream=side)
        if aug is not None:
            aug.apply(g.out_view(), d.xin.view(Cc, Cc, B, B), Cc, B)
        else:
            self._copy(g.out_view(), d.xin.view(Cc, Cc, B, B))
        if dreal:
            ctx.run(d.forward_part_ops(1))                            # pix2pix.py:203
        else:
            d.forward()                                               # pix2pix.py:202-203 (real ++ fake)
        if side is not None:
            ctx.join(main, side)
        real_ptr, cnt = d.logits_view(0)
        fake_ptr, _ = d.logits_view(1)
        lp = self.losses.data_ptr()
        three = ctx.lib.gan_patchgan_losses_lsq if self.gan_loss == 'lsgan' else ctx.lib.gan_patchgan_losses      # (same arguments)
        L.check(three(real_ptr, fake_ptr, cnt, ctx.dt, d.dlogits_b.t.data_ptr(), d.dlogits_ptr(0),
                      d.dlogits_ptr(1), 8, self.lam, lp + 8, lp, lp + 4, lp + 12,
                      self.bce_ws.data_ptr(), ctx.ls_ptr, ctx.stream()), "patchgan_losses")

    def _backward(self, phase, mode, adam_begun):
        """Two independent chains: D's parameter gradients (pix2pix.py:211) beside G's backward (:210)."""
        g, d, ctx = self.g, self.d, self.ctx
        main, lane2, lane3 = ctx.lane_stream(0), ctx.lane_stream(2), ctx.lane_stream(3)
        if phase == Phase.GENS:             # data-parallel, phased: D's parameter pass is the next phase (beside G's all-reduce)
            if ctx.lanes:
                g.wgrad_stream, g.wgrad_cuts, g.wgrad_stream2 = lane3, [8], None
                g.backward(use_dgen2=True, defer_wgrads='staged')
                ctx.join(main, lane3)
            else:
                g.backward(use_dgen2=True)
        elif ctx.lanes:                     # three chains: D params | G dgrad/norm chain | G wgrads in coarse stages
            lane2.wait_stream(main)
            ctx.run_on(d.params_ops(), lane2)
            if self._adam_in_chains(mode):
                # nothing else reads D's weights in this step: its (small) update runs at the end of its own chain
                self.D.params.adam(self.lr, self.b1, self.b2, stream=lane2)
                self._in_step.done = (self.D,)
            # the decoder's wgrad GEMMs start on lane 3 once the main chain has passed the decoder, the encoder's
            # at its end (+2.5 % over one stage at the end; per-op dependencies, mode 5, lose 9 %); a stage's wgrads start after
            # every dgrad of its layers has been enqueued (staged order), so a fused Adam may rewrite those layers' weights there
            g.wgrad_stream, g.wgrad_cuts = lane3, list(self.wgrad_cuts)
            g.wgrad_stream2 = ctx.lane_stream(4) if g.alt_wgrad else None
            self._g_backward(mode, adam_begun, lambda adam: g.backward(use_dgen2=True, defer_wgrads='staged', adam=adam))
            ctx.join(main, lane2)
            ctx.join(main, lane3)
            if g.wgrad_stream2 is not None:
                ctx.join(main, g.wgrad_stream2)
        else:                               # one stream (profiling runs): a stage's (fused-Adam) wgrads behind its dgrad chain
            def one_stream(adam):
                if adam is None:
                    return g.backward(use_dgen2=True)
                for ops, wops in g.bwd_stages(list(self.wgrad_cuts), use_dgen2=True, adam=adam):
                    ctx.run(ops + wops)
            self._g_backward(mode, False, one_stream)
            d.backward_params()

    def _g_backward(self, mode, adam_begun, run):
        """G's backward pass, run(adam).  mode.fuse_adam: its wgrad launches carry Adam (adam = the betas) - this step's lr_t must
        exist before the first of them (gan_adam_begin, unless D(real)'s lane has run it), and _update() is told which kernels
        are done."""
        if not mode.fuse_adam:
            return run(None)
        adam = (self.b1, self.b2)
        if not adam_begun:
            self.ctx.run(self.G.params.adam_begin_ops(self.lr, self.b1, self.b2))
        run(adam)
        self._in_step.wfused = {self.G: self.g.bwd_plan(use_dgen2=True, adam=adam).adam_fused}

    # ---- data-parallel schedule: bucketed exchange overlapped with the backward pass ---------------------------
    def _capture_bucketed(self):
        """Four compute graphs with gradient buckets leaving after each of them, and one Adam graph per
        bucket on a side stream as soon as that bucket's all-reduce has landed (the reference is
        single-device).  Stage k's wgrad GEMMs run beside stage k+1's dgrad/norm chain exactly as in the one-GPU
        schedule:

          G1  forward, losses, D's input-gradient pass, G backward stage 0 chain (decoder)
                                        ||  D's parameter-gradient pass -> bucket 4 = D (whole network)
          G2  stage 1 chain (down7..4)  ||  stage 0 wgrads              -> bucket 0 = decoder kernels
          G3  stage 2 chain (down3..0)  ||  stage 1 wgrads              -> bucket 1 = down7..4 kernels
          G4  stage 2 wgrads                                            -> bucket 2 = down3..0 kernels, 3 = G's vectors
        Weights are only rewritten by an Adam graph after every kernel that reads them in this step has been
        enqueued: a segment's NK copies feed the dgrads of its own stage, which precede its bucket."""
        ctx, g, d, sync = self.ctx, self.g, self.d, self.sync
        P, PD = self.G.params, self.D.params
        P.split_kernels_at('down4.kernel', 'up0.kernel')            # segments 0: down0..3 | 1: down4..7 | 2: up0..last
        o4, ou = P.entries['down4.kernel'][0], P.entries['up0.kernel'][0]
        self.buckets = [(0, ou, P.vec_start), (0, o4, ou), (0, 0, o4), (0, P.vec_start, P.total), (1, 0, PD.total)]
        # bf16 wire + all-reduce: the wgrad launches (their slab reduces / epilogues) write the wire format themselves - no fp32
        # gradient, no cast pass for those kernels; gan_grad_pack then covers only what is left of a bucket (the tap-folded first /
        # last layers and the vectors).  'rs_ag' reduces the fp32 gradients and keeps the cast of its own shard.
        direct = bool(self.ddp_wire_direct and sync.compress and getattr(sync, 'wire', None) is not None
                      and getattr(sync, 'exchange', 'allreduce') == 'allreduce')
        wG = sync.wire[0].data_ptr() if direct else None
        wD = sync.wire[1].data_ptr() if direct else None
        stages = g.bwd_stages([8, 12], use_dgen2=True, wire=wG)
        d_params = d.params_ops(wire=wD)
        assert len(stages) == 3
        skip = {0: set(g.bwd_plan(use_dgen2=True, wire=wG).wire_direct), 1: set(d_params.wire_direct)}      # (empty without a wire pointer)
        self._wire_direct_names = skip

        def pack_bucket(b):
            """Cast what the wgrad launches did not already write in the wire format: the bucket minus the direct kernels' ranges."""
            i, lo, hi = self.buckets[b]
            PS = (P, PD)[i]
            cuts = sorted((o, o + (int(torch.tensor(shape).prod()) + PS.ALIGN - 1) // PS.ALIGN * PS.ALIGN)
                          for n_, (o, shape) in PS.entries.items() if n_ in skip[i] and lo <= o < hi)
            a = lo
            for c0, c1 in cuts:
                if c0 > a:
                    sync.pack(i, a, c0)
                a = max(a, c1)
            if a < hi:
                sync.pack(i, a, hi)
        lane2, lane3, lane4 = ctx.lane_stream(2), ctx.lane_stream(3), ctx.lane_stream(4)

        def warm():
            self._forward_backward(*self._static_in, True, phase=Phase.GENS)
            self._forward_backward(*self._static_in, True, phase=Phase.DISCS)
            for b in range(len(self.buckets)):
                pack_bucket(b)
        self._warm_up(warm)

        def fork_join(side_ops, side_stream, main_fn, bucket=None):
            """side_ops (a stage's wgrad GEMMs) and then the cast of `bucket` to the wire format on the side stream,
            beside main_fn on the current one."""
            cur = torch.cuda.current_stream(ctx.device)
            side_stream.wait_stream(cur)
            ctx.run_on(side_ops, side_stream)
            if bucket is not None:
                with torch.cuda.stream(side_stream):
                    pack_bucket(bucket)
            main_fn()
            ctx.join(cur, side_stream)

        def g1():
            self._forward_backward(*self._static_in, True, phase=Phase.HEAD)          # everything up to G's backward
            # D's parameter-gradient pass runs on lane 2 beside the decoder chain, as in the one-GPU schedule; nothing
            # reads D's weights after this graph, so D's bucket is the first to leave
            cur = torch.cuda.current_stream(ctx.device)
            lane2.wait_stream(cur)
            ctx.run_on(d_params, lane2)
            with torch.cuda.stream(lane2):
                pack_bucket(4)
            ctx.run(stages[0][0])
            ctx.join(cur, lane2)

        def g2():
            fork_join(stages[0][1], lane3, lambda: ctx.run(stages[1][0]), bucket=0)

        def g3():
            fork_join(stages[1][1], lane3, lambda: ctx.run(stages[2][0]), bucket=1)

        def g4():
            ctx.run(stages[2][1])
            for b in (2, 3):
                pack_bucket(b)

        # Adam per bucket.  bf16 wire: Adam reads the exchanged gradient straight from the wire buffer (x 1/world) - no
        # unpack pass, and the fp32 gradient buffer keeps this rank's own gradient; fp32 wire: reduced in place, x 1/world
        gs = 1.0 / sync.world if sync.compress else sync.grad_scale
        wp = [w.data_ptr() for w in sync.wire] if sync.compress else [None, None]

        def a0():
            ctx.run(P.adam_begin_ops(self.lr, self.b1, self.b2) + P.adam_segment_ops(2, self.b1, self.b2, grad_scale=gs, wire_ptr=wp[0]))

        def a1():
            ctx.run(P.adam_segment_ops(1, self.b1, self.b2, grad_scale=gs, wire_ptr=wp[0]))

        def a2():
            ctx.run(P.adam_segment_ops(0, self.b1, self.b2, grad_scale=gs, vectors=True, wire_ptr=wp[0]))

        def a3():
            PD.adam(self.lr, self.b1, self.b2, grad_scale=gs, wire_ptr=wp[1])

        G = [self._graph(f) for f in (g1, g2, g3, g4)]
        A = [self._graph(f) for f in (a0, a1, a2, a3)]
        self._graphs = tuple(G + A)
        # after G_k: (the bucket that leaves, the Adam graph that follows it)
        leaving = [[(4, 3)], [(0, 0)], [(1, 1)], [(2, None), (3, 2)]]
        # Host order matters: a compute graph is enqueued BEFORE the collectives / Adam graphs of the boundary behind it are
        # issued (they hang off an event recorded at that boundary, on their own launcher stream), so the GPU never waits
        # for the host's communicator calls between two compute graphs (that was ~50 us of idle chip per boundary).
        evs = [torch.cuda.Event() for _ in G]
        comm = torch.cuda.Stream(device=ctx.device)

        def boundary(k):
            comm.wait_event(evs[k])
            with torch.cuda.stream(comm):
                started = [(sync.start(*self.buckets[b]), ai) for b, ai in leaving[k]]
            lane4.wait_event(evs[k])                       # (the Adam graphs also read what the compute graphs wrote)
            with torch.cuda.stream(lane4):
                for h, ai in started:
                    sync.wait(h)                           # lane 4 waits for the collective; the host does not
                    if ai is not None:
                        A[ai].replay()

        def body():
            cur = torch.cuda.current_stream(ctx.device)
            for k, gr in enumerate(G):
                gr.replay()
                evs[k].record(cur)
                if k > 0:
                    boundary(k - 1)
            boundary(len(G) - 1)
            ctx.join(cur, lane4)
        return self._replayer(body, True)

    def train_step(self, input_image, target, training=True):
        """(gen_total_loss, gen_gan_loss, gen_l1_loss, disc_loss) as a 4-element device tensor view."""
        return self._run(input_image, target, training)[:4]


class CycleGANStep(_StepBase):
    two_chains = True            # one-GPU step: the G_g-side and the G_f-side chains on two lanes (_forward_backward_merged)
    early_adam = True            # ... and every network's Adam where its gradients complete, inside the chains
    fused_wgrad_adam = True      # ... whose un-split launches apply Adam to their kernels themselves (captured step; GanAdamFuse)
    wide_wgrads = True           # ... one wgrad GEMM per layer over a generator's three invocations (host + guest call)

    def __init__(self, ctx: Ctx, batch, size, channels=1, lam=10.0, lr=2e-4, beta_1=0.5, beta_2=0.999,
                 seed=123, dropout=True, nets=None, mask_stream=0, merged=True, gan_loss='bce', lr_schedule=None, pools=None):
        """pools: (pool_y, pool_x), two gan_amd.pool.ImagePool objects of the MODEL (steps of other batch sizes query the same
        two) - the discriminators then learn from a history of generated images; None: from the current ones."""
        super().__init__(ctx, batch, size, channels, lam, lr, beta_1, beta_2, n_losses=12, gan_loss=gan_loss)     # [0..8] as below; [9] cycle term of chain B; [10] stays 0
        if pools is not None:
            if not merged:
                raise ValueError("pools: only the merged schedule queries an image pool (merged=False exists for one equivalence test)")
            pools = tuple(pools)
            if len(pools) != 2 or any((p.size, p.channels) != (size, channels) for p in pools):
                raise ValueError(f"pools: (pool_y, pool_x) of {size} x {size} x {channels} images")
        self.pools = pools
        # the discriminator's batch: [real ; fake], or with pools [real ; pooled ; current] - the parameter pass covers the first two
        # invocations, the generator's adversarial term goes through the last one
        self._fake_call = 2 if pools else 1
        n = 'instancenorm'                                                    # cycle_gan.py:30-33
        if nets is not None:
            self.Gg, self.Gf, self.Dx, self.Dy = nets
        else:
            self.Gg = GeneratorNet(ctx, channels, n, seed=seed)
            self.Gf = GeneratorNet(ctx, channels, n, seed=seed + 1)
            self.Dx = DiscriminatorNet(ctx, channels, False, n, seed=seed + 2)
            self.Dy = DiscriminatorNet(ctx, channels, False, n, seed=seed + 3)
        mk = lambda net, sid, lane=0: net.new_call(batch, size, dropout=dropout, seed=seed, stream_id=mask_stream + sid, lane=lane)
        # The step is launch- and small-grid-bound (~1,200 launches): G_g(x) and G_g(y) - likewise G_f(y), G_f(x) - use the same
        # weights and InstanceNormalization is per sample, so the two invocations run as ONE call of batch 2B (exactly the
        # same arithmetic per sample, a third fewer generator launches); the cycle calls depend on their outputs and stay.
        # Measured +30 % (B=1) ... +15 % (B=16) pairs/s; merged=False keeps the six separate calls (equivalence test, A/B runs).
        self.merged = bool(merged)
        # chain "A" (lane 0 workspaces): G_g([x ; y]) -> G_f(fake_y) -> D_y;  chain "B" (lane 2): G_f([y ; x]) -> G_g(fake_x) -> D_x
        if self.merged:
            # the cycle call of a generator is the GUEST of its batched call (shared, wider saved tensors): one wgrad GEMM per
            # layer then covers all three invocations of the generator instead of a write + accumulate pair
            self.gA = self.Gg.new_call(2 * batch, size, dropout=dropout, seed=seed, stream_id=mask_stream + 0, guest_batch=batch)   # [fake_y ; same_y]
            self.gB = self.Gf.new_call(2 * batch, size, dropout=dropout, seed=seed, stream_id=mask_stream + 2, lane=2, guest_batch=batch)   # [fake_x ; same_x]
            mkc = lambda net, sid, lane, host: net.new_call(batch, size, dropout=dropout, seed=seed, stream_id=mask_stream + sid, lane=lane, host=host)
            self.cx, self.cy = mkc(self.Gf, 1, 0, self.gB), mkc(self.Gg, 3, 2, self.gA)      # cycled_x = G_f(fake_y); cycled_y = G_g(fake_x)
        else:
            self.cx, self.cy = mk(self.Gf, 1), mk(self.Gg, 3)
        self._wide = None
        if self.merged and ctx.lanes:       # planner hint of the wgrad GEMMs: they run beside the mirror chain's
            for c_ in (self.gA, self.gB, self.cx, self.cy):
                c_._bd.wgrad_concurrent = 2
        if self.merged:
            self.fy, self.sy = self.gA.half(0, batch), self.gA.half(batch, batch)
            self.fx, self.sx = self.gB.half(0, batch), self.gB.half(batch, batch)
        else:
            self.fy, self.fx = mk(self.Gg, 0), mk(self.Gf, 2)  # fake_y = G_g(x); fake_x = G_f(y)
            self.sx, self.sy = mk(self.Gf, 4), mk(self.Gg, 5)  # same_x = G_f(x); same_y = G_g(y)
        if self.merged:
            # (own workspaces for the parameter passes: they run beside the generators' wgrad lanes)
            nc = self._fake_call + 1
            self.dx = self.Dx.new_call(batch, size, calls=nc, lane=2, params_lane=6, param_calls=2)       # D_x(real_x) ++ D_x(fake_x): chain B
            self.dy = self.Dy.new_call(batch, size, calls=nc, lane=0, params_lane=4, param_calls=2)
            if ctx.lanes:
                self.dx._bd2.wgrad_concurrent = self.dy._bd2.wgrad_concurrent = 2
        else:
            self.dx = self.Dx.new_call(batch, size, calls=2)
            self.dy = self.Dy.new_call(batch, size, calls=2)
        self.l1_ws_b = torch.zeros(4096, dtype=torch.float32, device=ctx.device)   # chain B's loss kernels run beside chain A's
        self.bce_ws_b = torch.zeros(1024, dtype=torch.float32, device=ctx.device)
        self._set_lr_schedule(lr_schedule)

    def nets(self):
        return (self.Gg, self.Gf, self.Dx, self.Dy)

    def capture(self, training=True):
        """The warm-up passes query the image pools: they are left as they were found, state and contents."""
        saved = [(t, t.clone()) for pool in self.pools or () for t in pool.tensors()]
        replay = super().capture(training)
        for t, v in saved:
            t.copy_(v)
        return replay

    def _prebuild_fused_adam(self):
        if self._wgrad_adam_ok() and self.merged and self.two_chains and self.early_adam and self.wide_wgrads and self._wide:
            wide = dict(use_dgen2=True, accumulate=True, wgrads='wide', adam=(self.b1, self.b2))
            for call, net in ((self.gA, self.Gg), (self.gB, self.Gf)):
                call.bwd_stages([8, 12], **wide)
                net.params.adam_rest_ops(call.bwd_plan(**wide).adam_fused, self.b1, self.b2)

    def gen_calls(self):
        return dict(fake_y=self.fy, cycled_x=self.cx, fake_x=self.fx, cycled_y=self.cy, same_x=self.sx, same_y=self.sy)

    def ddp_phases(self):
        """Gradient sets in the order the backward pass completes them (cycle_gan.py:252-260): G_g | G_f | D_x | D_y."""
        if self.merged and self.ctx.lanes and self.two_chains:
            # the two chains complete both generators together, then both discriminators: two phases (the four-phase serial
            # schedule costs twice the compute per step: 8.5 against 4.7 ms at batch 4 in the one-rank rehearsal)
            return [(Phase.CHAINS_GENS, [0, 1]), (Phase.CHAINS_DISCS, [2, 3])]
        if self.merged:
            return [(Phase.SERIAL_GG, [0]), (Phase.SERIAL_GF, [1]), (Phase.SERIAL_DX, [2]), (Phase.SERIAL_DY, [3])]
        return [(Phase.GENS, [0, 1]), (Phase.DISCS, [2, 3])]

    def _forward_backward(self, real_x, real_y, training=True, phase=Phase.FULL, mode=_Mode()):
        B, Cc, lam = self.B, self.C, self.lam
        if phase == Phase.DISCS:
            self.dx.backward_params(); self.dy.backward_params()
            return self.losses
        if phase == Phase.SERIAL_GF:
            self.gB.backward(use_dgen2=True, accumulate=True)          # G_f complete
            return self.losses
        if phase in (Phase.SERIAL_DX, Phase.SERIAL_DY):
            (self.dx if phase == Phase.SERIAL_DX else self.dy).backward_params()
            return self.losses
        if phase == Phase.CHAINS_DISCS:                                                # both discriminators' parameter passes, one per chain
            main, l2 = self.ctx.lane_stream(0), self.ctx.lane_stream(2)
            l2.wait_stream(main)
            self.dy.backward_params()
            with torch.cuda.stream(l2):
                self.dx.backward_params()
            self.ctx.join(main, l2)
            return self.losses
        if self.merged:
            return self._forward_backward_merged(real_x, real_y, training, phase, mode)
        fy, cx, fx, cy, sx, sy, dx, dy = self.fy, self.cx, self.fx, self.cy, self.sx, self.sy, self.dx, self.dy
        self._pack_multi([(real_x, fy.xin.view(0, Cc)), (real_x, sx.xin.view(0, Cc)), (real_y, fx.xin.view(0, Cc)), (real_y, sy.xin.view(0, Cc))])
        self._pack_multi([(real_x, dx.xin.view(0, Cc, 0, B)), (real_y, dy.xin.view(0, Cc, 0, B))])
        fy.forward()                                                  # cycle_gan.py:220
        self._copy(fy.out_view(), cx.xin.view(0, Cc)); self._copy(fy.out_view(), dy.xin.view(0, Cc, B, B))
        cx.forward()                                                  # :221
        fx.forward()                                                  # :223
        self._copy(fx.out_view(), cy.xin.view(0, Cc)); self._copy(fx.out_view(), dx.xin.view(0, Cc, B, B))
        cy.forward()                                                  # :224
        sx.forward(); sy.forward()                                    # :227-228
        dx.forward(); dy.forward()                                    # :230-234
        rx_ptr, cnt = dx.logits_view(0); fxl_ptr, _ = dx.logits_view(1)
        ry_ptr, _ = dy.logits_view(0); fyl_ptr, _ = dy.logits_view(1)
        xv, yv = fy.xin.view(0, Cc), fx.xin.view(0, Cc)               # typed real_x / real_y
        self._bce(fyl_ptr, cnt, 1.0, 0, 1.0, False, 1.0, dy.dlogits_b.t.data_ptr())      # gen_g_loss :237
        self._bce(fxl_ptr, cnt, 1.0, 1, 1.0, False, 1.0, dx.dlogits_b.t.data_ptr())      # gen_f_loss :238
        self._l1(cx.out_view(), xv, 2, lam, False, lam, cx.dgen.view(0, Cc))              # total_cycle_loss :240
        self._l1(cy.out_view(), yv, 2, lam, True, lam, cy.dgen.view(0, Cc))
        self._l1(sy.out_view(), yv, 7, lam * 0.5, False, lam * 0.5, sy.dgen.view(0, Cc))  # identity :243
        self._l1(sx.out_view(), xv, 8, lam * 0.5, False, lam * 0.5, sx.dgen.view(0, Cc))  # identity :244
        lp = self.losses.data_ptr()               # total_gen_g / total_gen_f (:243-244): gen + cycle + identity, one tiny launch
        L.check(self.ctx.lib.gan_sum3(lp, lp + 8, lp + 28, lp + 12, 1, self.ctx.stream()), "sum3")      # [3] = [0] + [2] + [7]
        L.check(self.ctx.lib.gan_sum3(lp + 4, lp + 8, lp + 32, lp + 16, 1, self.ctx.stream()), "sum3")  # [4] = [1] + [2] + [8]
        self._bce(rx_ptr, cnt, 1.0, 5, 0.5, False, 0.5, dx.dlogits_ptr(0))                # disc_x_loss :246
        self._bce(fxl_ptr, cnt, 0.0, 5, 0.5, True, 0.5, dx.dlogits_ptr(1))
        self._bce(ry_ptr, cnt, 1.0, 6, 0.5, False, 0.5, dy.dlogits_ptr(0))                # disc_y_loss :247
        self._bce(fyl_ptr, cnt, 0.0, 6, 0.5, True, 0.5, dy.dlogits_ptr(1))
        if training:
            # cycle terms: backward through the second generator of each cycle yields BOTH its parameter
            # gradients and the gradient w.r.t. fake_y / fake_x (computed once, used twice)
            cx.backward(need_dx=True, accumulate=False)               # G_f grads (cycle_x), d/d fake_y
            cy.backward(need_dx=True, accumulate=False)               # G_g grads (cycle_y), d/d fake_x
            dy.backward_input(1, dst=fy.dgen.view(0, Cc))             # adversarial term through D_y(fake_y)
            self._copy(cx.dxin.view(0, Cc), fy.dgen2.view(0, Cc))
            fy.backward(use_dgen2=True, accumulate=True)              # G_g
            dx.backward_input(1, dst=fx.dgen.view(0, Cc))
            self._copy(cy.dxin.view(0, Cc), fx.dgen2.view(0, Cc))
            fx.backward(use_dgen2=True, accumulate=True)              # G_f
            sy.backward(accumulate=True)                              # identity_y -> G_g
            sx.backward(accumulate=True)                              # identity_x -> G_f
            if phase != Phase.GENS:
                dx.backward_params(); dy.backward_params()            # :257-260
        return self.losses                                            # four Adam applies: _update() (:263-273)

    def _forward_backward_merged(self, real_x, real_y, training, phase, mode):
        """The same step with [fake_y ; same_y] = G_g([x ; y]) and [fake_x ; same_x] = G_f([y ; x]) as two batch-2B calls."""
        B, Cc, lam = self.B, self.C, self.lam
        gA, gB, cx, cy, dx, dy = self.gA, self.gB, self.cx, self.cy, self.dx, self.dy
        fy, sy, fx, sx = self.fy, self.sy, self.fx, self.sx
        # Two independent halves until the losses and again in the backward pass (cycle_gan.py:220-234 lists them interleaved):
        # chain A = G_g([x ; y]) -> G_f(fake_y) -> D_y, chain B = G_f([y ; x]) -> G_g(fake_x) -> D_x.  The step is launch- and
        # small-grid-bound at the reference's batch sizes, so the chains run on two lanes of the captured graph.
        two = bool(self.ctx.lanes and self.two_chains and phase in (Phase.FULL, Phase.CHAINS_GENS))
        main, l2 = self.ctx.lane_stream(0), self.ctx.lane_stream(2)
        chain_b = (lambda: torch.cuda.stream(l2)) if two else contextlib.nullcontext
        self._pack_multi([(real_x, fy.xin_view()), (real_y, sy.xin_view()), (real_y, fx.xin_view()), (real_x, sx.xin_view())])
        self._pack_multi([(real_x, dx.xin.view(0, Cc, 0, B)), (real_y, dy.xin.view(0, Cc, 0, B))])
        fc, pools = self._fake_call, self.pools
        if pools and not training:
            raise ValueError("a step with image pools is a training step (validation judges the current fakes)")
        rx_ptr, cnt = dx.logits_view(0); fxl_ptr, _ = dx.logits_view(fc)       # generator side: D(current fakes)
        ry_ptr, _ = dy.logits_view(0); fyl_ptr, _ = dy.logits_view(fc)
        pxl_ptr, _ = dx.logits_view(1); pyl_ptr, _ = dy.logits_view(1)        # discriminator side: D(pooled), = D(current) without pools
        xv, yv = fy.xin_view(), sy.xin_view()                         # typed real_x / real_y
        lp = self.losses.data_ptr()
        if two:
            l2.wait_stream(main)
        gA.forward()                                                  # cycle_gan.py:220 and :228
        self._copy(fy.out_view(), cx.xin.view(0, Cc)); self._copy(fy.out_view(), dy.xin.view(0, Cc, fc * B, B))
        if pools:
            pools[0].exchange(fy.out_view(), dy.xin.view(0, Cc, B, B))
        cx.forward()                                                  # :221
        dy.forward()                                                  # :233-234
        if two:
            # each chain takes the loss terms (and their gradients) of its own outputs; only the reported totals need both
            # chains and are summed after the final join - no join between the forward and the backward pass
            self._bce(fyl_ptr, cnt, 1.0, 0, 1.0, False, 1.0, dy.dlogits_b.t.data_ptr())      # gen_g_loss :237
            self._l1(cx.out_view(), xv, 2, lam, False, lam, cx.dgen.view(0, Cc))              # cycle term of x :240
            self._l1(sy.out_view(), yv, 7, lam * 0.5, False, lam * 0.5, sy.dgen_view())       # identity :243
            self._bce(ry_ptr, cnt, 1.0, 6, 0.5, False, 0.5, dy.dlogits_ptr(0))                # disc_y_loss :247
            self._bce(pyl_ptr, cnt, 0.0, 6, 0.5, True, 0.5, dy.dlogits_ptr(1))
        with chain_b():
            gB.forward()                                              # :223 and :227
            self._copy(fx.out_view(), cy.xin.view(0, Cc)); self._copy(fx.out_view(), dx.xin.view(0, Cc, fc * B, B))
            if pools:
                pools[1].exchange(fx.out_view(), dx.xin.view(0, Cc, B, B))
            cy.forward()                                              # :224
            dx.forward()                                              # :230-231
            if two:
                wl, wb = self.l1_ws_b, self.bce_ws_b
                self._bce(fxl_ptr, cnt, 1.0, 1, 1.0, False, 1.0, dx.dlogits_b.t.data_ptr(), ws=wb)      # gen_f_loss :238
                self._l1(cy.out_view(), yv, 9, lam, False, lam, cy.dgen.view(0, Cc), ws=wl)              # cycle term of y
                self._l1(sx.out_view(), xv, 8, lam * 0.5, False, lam * 0.5, sx.dgen_view(), ws=wl)       # identity :244
                self._bce(rx_ptr, cnt, 1.0, 5, 0.5, False, 0.5, dx.dlogits_ptr(0), ws=wb)                # disc_x_loss :246
                self._bce(pxl_ptr, cnt, 0.0, 5, 0.5, True, 0.5, dx.dlogits_ptr(1), ws=wb)
        if not two:
            self._bce(fyl_ptr, cnt, 1.0, 0, 1.0, False, 1.0, dy.dlogits_b.t.data_ptr())      # gen_g_loss :237
            self._bce(fxl_ptr, cnt, 1.0, 1, 1.0, False, 1.0, dx.dlogits_b.t.data_ptr())      # gen_f_loss :238
            self._l1(cx.out_view(), xv, 2, lam, False, lam, cx.dgen.view(0, Cc))              # total_cycle_loss :240
            self._l1(cy.out_view(), yv, 2, lam, True, lam, cy.dgen.view(0, Cc))
            self._l1(sy.out_view(), yv, 7, lam * 0.5, False, lam * 0.5, sy.dgen_view())       # identity :243
            self._l1(sx.out_view(), xv, 8, lam * 0.5, False, lam * 0.5, sx.dgen_view())       # identity :244
            self._totals(False)
            self._bce(rx_ptr, cnt, 1.0, 5, 0.5, False, 0.5, dx.dlogits_ptr(0))                # disc_x_loss :246
            self._bce(pxl_ptr, cnt, 0.0, 5, 0.5, True, 0.5, dx.dlogits_ptr(1))
            self._bce(ry_ptr, cnt, 1.0, 6, 0.5, False, 0.5, dy.dlogits_ptr(0))                # disc_y_loss :247
            self._bce(pyl_ptr, cnt, 0.0, 6, 0.5, True, 0.5, dy.dlogits_ptr(1))
        elif not training:
            self.ctx.join(main, l2)
            self._totals(True)
        if training:
            if two:
                # A: cycle_x through G_f, D_y's input gradient, then G_g's own backward and D_y's parameter pass;  B: the mirror
                # image.  The second backward of each generator ACCUMULATES onto what the OTHER chain's first one wrote: one
                # cross-wait.  With nothing else pending (one GPU, no loss scaling) each network's Adam runs where its gradients
                # complete: the generators' kernel segments inside their chain as soon as the backward pass has left them
                # (HBM-bound, beside the other chain's launch-bound kernels), the discriminators' after their parameter pass.
                fused_adam = bool(self._adam_in_chains(mode) and self.early_adam)

                if self._wide is None:       # host and guest must keep down0's output gradient in the same buffer (plan dependent)
                    self._wide = all(h.bwd_plan(use_dgen2=True, accumulate=True, wgrads='wide').dy0_in_dA ==
                                     g_.bwd_plan(need_dx=True, wgrads='none').dy0_in_dA for h, g_ in ((gA, cy), (gB, cx)))
                wide = self._wide and self.wide_wgrads
                w1, w2 = ('none', 'wide') if wide else ('own', 'own')

                wf = bool(fused_adam and wide and mode.fuse_adam)

                def second_backward(gen, net):
                    """gen.backward(use_dgen2, accumulate) with the network's Adam inside the chain: HBM-bound work of one chain
                    beside the launch-bound kernels of the other.  With wide wgrads in the captured step the un-split wgrad
                    launches apply Adam to their kernels themselves (GanAdamFuse; a stage's wgrads follow every dgrad of its
                    layers) and one small launch pair updates the rest; otherwise a kernel segment (decoder | down7..4 | down3..0)
                    is updated right behind its last wgrad GEMM.  Returns True when the vectors have been updated too.
                    (Side lanes forked from lane 2 end the capture with "unjoined work" on this runtime, and wgrad GEMMs on side
                    lanes lose here: profiles/r03_experiments_not_kept.txt.)"""
                    if not fused_adam:
                        gen.backward(use_dgen2=True, accumulate=True, wgrads=w2)
                        return False
                    P = net.params
                    if wf:
                        fused = dict(use_dgen2=True, accumulate=True, wgrads='wide', adam=(self.b1, self.b2))
                        self.ctx.run(P.adam_begin_ops(self.lr, self.b1, self.b2))
                        for ops, wops in gen.bwd_stages([8, 12], **fused):
                            self.ctx.run(ops + wops)
                        self.ctx.run(P.adam_rest_ops(gen.bwd_plan(**fused).adam_fused, self.b1, self.b2))
                        return True
                    if P._segments is None or len(P._segments) != 3:
                        P.split_kernels_at('down4.kernel', 'up0.kernel')
                    for k, (ops, wops) in enumerate(gen.bwd_stages([8, 12], use_dgen2=True, accumulate=True, wgrads=w2)):
                        self.ctx.run(ops + wops)
                        self.ctx.run((P.adam_begin_ops(self.lr, self.b1, self.b2) if k == 0 else []) +
                                     P.adam_segment_ops(2 - k, self.b1, self.b2, vectors=False))
                    return False

                cx.backward(need_dx=True, accumulate=False, wgrads=w1)    # G_f grads (cycle_x), d/d fake_y
                dy.backward_input(fc, dst=fy.dgen_view())             # adversarial term through D_y(fake_y)
                self._copy(cx.dxin.view(0, Cc), fy.dgen_view(second=True))
                with chain_b():
                    cy.backward(need_dx=True, accumulate=False, wgrads=w1)    # G_g grads (cycle_y), d/d fake_x
                    dx.backward_input(fc, dst=fx.dgen_view())
                    self._copy(cy.dxin.view(0, Cc), fx.dgen_view(second=True))
                ea, eb = torch.cuda.Event(), torch.cuda.Event()
                ea.record(main); eb.record(l2)
                main.wait_event(eb); l2.wait_event(ea)
                vdone = second_backward(gA, self.Gg)      # G_g
                if phase == Phase.CHAINS_GENS:                         # data-parallel: the generators' exchange starts here
                    with chain_b():
                        second_backward(gB, self.Gf)
                    self.ctx.join(main, l2)
                    self._totals(True)
                    return self.losses
                dy.backward_params()
                if fused_adam:
                    self.Dy.params.adam(self.lr, self.b1, self.b2, stream=main)
                    if not vdone:
                        self.ctx.run(self.Gg.params.adam_segment_ops(0, self.b1, self.b2, vectors=True, kernels=False))
                with chain_b():
                    vdone = second_backward(gB, self.Gf)      # G_f
                    dx.backward_params()
                    if fused_adam:
                        self.Dx.params.adam(self.lr, self.b1, self.b2, stream=l2)
                        if not vdone:
                            self.ctx.run(self.Gf.params.adam_segment_ops(0, self.b1, self.b2, vectors=True, kernels=False))
                if fused_adam:
                    self._in_step.done = self.nets()
                self.ctx.join(main, l2)
                self._totals(True)
                return self.losses
            cx.backward(need_dx=True, accumulate=False)               # G_f grads (cycle_x), d/d fake_y
            cy.backward(need_dx=True, accumulate=False)               # G_g grads (cycle_y), d/d fake_x
            dy.backward_input(fc, dst=fy.dgen_view())                 # adversarial term through D_y(fake_y)
            self._copy(cx.dxin.view(0, Cc), fy.dgen_view(second=True))
            dx.backward_input(fc, dst=fx.dgen_view())
            self._copy(cy.dxin.view(0, Cc), fx.dgen_view(second=True))
            # second upstream slot of the identity halves stays zero (never written); one backward per generator covers the
            # adversarial + cycle gradient of fake_* and the identity gradient of same_*
            gA.backward(use_dgen2=True, accumulate=True)              # G_g
            if phase == Phase.SERIAL_GG:                                           # phased data-parallel schedule: G_g's exchange starts here
                return self.losses
            gB.backward(use_dgen2=True, accumulate=True)              # G_f
            if phase != Phase.GENS:
                dx.backward_params(); dy.backward_params()
        return self.losses

    def _totals(self, split_cycle):
        """total_cycle_loss and total_gen_g / total_gen_f (cycle_gan.py:240-244): [3] = [0] + [2] + [7], [4] = [1] + [2] + [8];
        split_cycle: the two chains left the cycle terms of x and y in [2] and [9] ([10] is never written: 0)."""
        lp, lib, st_ = self.losses.data_ptr(), self.ctx.lib, self.ctx.stream()
        if split_cycle:
            L.check(lib.gan_sum3(lp + 8, lp + 36, lp + 40, lp + 8, 1, st_), "sum3")         # [2] += [9]
        L.check(lib.gan_sum3(lp, lp + 8, lp + 28, lp + 12, 1, st_), "sum3")
        L.check(lib.gan_sum3(lp + 4, lp + 8, lp + 32, lp + 16, 1, st_), "sum3")

    def train_step(self, real_x, real_y, training=True):
        """7 losses in the reference's order (cycle_gan.py:275-276)."""
        return self._run(real_x, real_y, training)[:7]
