"""`GAN` base class with the reference's surface (base_gan.py:21-292) on top of the MI355X kernels.

`Generator(...)` / `Discriminator(...)` return callable model objects (`model(x, training=True)`), like the
Keras models of the reference; their weights live in `gan_amd.nets.ParamSet` buffers shared with the fused
train-step objects.  As in the reference, `training=True` is the default and what every call site of the
training loop uses (batch statistics, dropout on, moving statistics updated — pix2pix.py:200-203,228).
`training=False` is Keras inference mode: BatchNormalization normalises with its moving statistics and Dropout
is the identity, so the output is deterministic and independent of the rest of the batch.  BatchNorm layers
then run as one convolution each on weights folded with the moving statistics (gan_bn_fold_multi); the fold is
refreshed on every such call, so it always reflects the current weights.  InstanceNorm has no inference-time
state: for CycleGAN only the dropout differs."""
from __future__ import annotations

import ctypes as C
import os
from abc import ABC, abstractmethod

import numpy as np
import torch

from . import _lib as L
from . import data as D
from . import ddp
from . import tiling
from .checkpoint import DISC_LAYERS, GEN_LAYERS, tf_variable_key
from .ema import WeightAverage
from .nets import Ctx, DiscriminatorNet, GeneratorNet, workspace_mb_for
from .pool import STREAM_X, STREAM_Y
from .runner import lr_schedule_for, run_epochs
from .train_state import TrainState


def _to_dev(x, ctx):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return x.to(device=ctx.device, dtype=torch.float32).contiguous()


class _Model:
    """Common: state_dict()/load_state_dict() with TF object-graph style keys (checkpoint.py)."""
    layers = GEN_LAYERS
    obj_name = 'model'

    def state_dict(self):
        P = self.net.params.to_numpy()
        return {tf_variable_key(self.obj_name, self.layers, k).split('/', 1)[1]: v for k, v in P.items()}

    def load_state_dict(self, sd):
        P = self.net.params.to_numpy()
        for k in list(P):
            key = tf_variable_key(self.obj_name, self.layers, k).split('/', 1)[1]
            if key in sd:
                P[k] = sd[key].astype(np.float32).reshape(P[k].shape)
        self.net.params.load_numpy(P)

    def param_names(self):
        return list(self.net.params.entries) + list(self.net.params.state)

    @property
    def trainable_variables(self):
        return [self.net.params.tensor(n) for n in self.net.params.names]

    def count_params(self):
        return self.net.params.trainable_count()


class GeneratorModel(_Model):
    layers = GEN_LAYERS

    def __init__(self, net: GeneratorNet, obj_name='generator'):
        self.net, self.obj_name, self._calls, self._eval_calls = net, obj_name, {}, {}
        self._restored_draws = {}      # (batch, size) -> dropout draw counters of a restored train_state, for calls not built yet

    def __call__(self, x, training=True):
        if not training:
            return self.infer(x, fold=True)
        ctx = self.net.ctx
        x = _to_dev(x, ctx)
        B, S = x.shape[0], x.shape[1]
        key = (B, S)
        if key not in self._calls:
            self._calls[key] = self.net.new_call(B, S, dropout=True, stream_id=40)     # (ids 0..5 / 16..21: the train / validation steps' generator calls)
            if key in self._restored_draws:
                self._calls[key].mask_draws.copy_(torch.from_numpy(self._restored_draws.pop(key).astype(np.int32)))
        call = self._calls[key]
        call.set_input(x)
        call.forward()
        return call.output_f32()

    def fold(self):
        """Fold the current weights and moving statistics into the inference-mode weights (BatchNorm; nothing for InstanceNorm)."""
        if self.net.norm == 'batchnorm':
            self.net.folded().fold()

    def infer(self, x, fold=True):
        """`model(x, training=False)`.  fold=False: skip the fold launch - only right if fold() ran after the last change of the
        weights or moving statistics (a train step, load_state_dict, a checkpoint restore)."""
        return self.infer_call(x, fold).output_f32()

    def infer_call(self, x, fold=True):
        """infer() up to the forward: -> the eval call, whose typed output view (out_view()) holds the prediction until the next
        call of this batch size (gan_amd.quality reads it there, without the unpack)."""
        x = _to_dev(x, self.net.ctx)
        call = self.eval_call(x.shape[0], x.shape[1])
        call.set_input(x)
        call.infer(fold=fold)
        return call

    def eval_call(self, batch, size):
        """The (cached) inference call of this batch and image size."""
        key = (batch, size)
        if key not in self._eval_calls:
            self._eval_calls[key] = self.net.new_eval_call(batch, size)
        return self._eval_calls[key]

    def infer_tiled(self, src_u8, *, tile, overlap, col0=0, width=None, batch=None, fold=True):
        """Inference mode over a whole uint8 device image [H, W, C] of any size >= tile: overlapping tile x tile pieces through
        the eval call as a batch, blended back on the device -> fp32 device tensor [H, width, C] (gan_amd/tiling.py).  This method
        keeps to decoded image files: anything but uint8 is refused; a float image that is normalised already (the output of
        another generator) goes through tiling.infer_tiled itself."""
        if not isinstance(src_u8, torch.Tensor) or src_u8.dtype != torch.uint8:
            raise ValueError("infer_tiled: expected a contiguous uint8 [H, W, C] tensor on the model's device")
        return tiling.infer_tiled(self, src_u8, tile=tile, overlap=overlap, col0=col0, width=width, batch=batch, fold=fold)


class DiscriminatorModel(_Model):
    layers = DISC_LAYERS

    def __init__(self, net: DiscriminatorNet, obj_name='discriminator'):
        self.net, self.obj_name, self._calls, self._eval_calls = net, obj_name, {}, {}

    def __call__(self, inputs, training=True):
        ctx = self.net.ctx
        xs = inputs if isinstance(inputs, (list, tuple)) else [inputs]
        xs = [_to_dev(x, ctx) for x in xs]
        B, S, Cc = xs[0].shape[0], xs[0].shape[1], self.net.channels
        key = (B, S)
        calls = self._calls if training else self._eval_calls
        if key not in calls:
            calls[key] = self.net.new_call(B, S, calls=1) if training else self.net.new_eval_call(B, S)
        call = calls[key]
        for i, x in enumerate(xs):      # concatenate([inp, tar]) realised as channel slices (base_gan.py:139)
            v = call.xin.view(i * Cc, Cc)
            L.check(ctx.lib.gan_pack(ctx.dt, x.data_ptr(), C.byref(v), ctx.stream()), "pack")
        if training:
            call.forward()
        else:                           # inference mode: moving statistics (folded into the convolutions on every call)
            call.infer(fold=True)
        return call.logits.t.clone()


class AdamConfig:
    """`GAN.optimizer(...)` result: hyper-parameters; the state (m, v, step) lives beside the weights."""

    def __init__(self, learning_rate, beta_1, beta_2):
        self.learning_rate, self.beta_1, self.beta_2 = learning_rate, beta_1, beta_2
        self.params = None

    def bind(self, paramset):
        self.params = paramset
        return self

    def state_dict(self):
        if self.params is None:
            return {}
        ps = self.params
        out = {'iter/.ATTRIBUTES/VARIABLE_VALUE': ps.step.cpu().numpy().astype(np.int64).reshape(()),       # scalars, as Keras stores them
               'learning_rate/.ATTRIBUTES/VARIABLE_VALUE': np.float32(self.learning_rate),
               'beta_1/.ATTRIBUTES/VARIABLE_VALUE': np.float32(self.beta_1),
               'beta_2/.ATTRIBUTES/VARIABLE_VALUE': np.float32(self.beta_2),
               'decay/.ATTRIBUTES/VARIABLE_VALUE': np.float32(0.0)}
        for slot in ('m', 'v'):
            for k, a in ps.to_numpy(slot).items():
                out[f'slot/{slot}/{k}'] = a
        return out

    def load_state_dict(self, sd):
        if self.params is None:
            return
        ps = self.params
        if 'iter/.ATTRIBUTES/VARIABLE_VALUE' in sd:
            ps.step.copy_(torch.from_numpy(np.asarray(sd['iter/.ATTRIBUTES/VARIABLE_VALUE'], np.int32).reshape(1)))
        for slot in ('m', 'v'):
            for name in ps.entries:
                k = f'slot/{slot}/{name}'
                if k in sd:
                    ps.tensor(name, slot).copy_(torch.from_numpy(sd[k].astype(np.float32)).view(ps.entries[name][1]))


def pool_state(pool):
    """name -> tensor of one image pool (pool_y serves D_y, pool_x D_x)."""
    name = {STREAM_Y: 'pool_y', STREAM_X: 'pool_x'}.get(pool.stream_id, f'pool_{pool.stream_id}')
    return {f'{name}/{part}': t for part, t in zip(('state', 'storage'), pool.tensors())}


def diffaug_state(aug):
    return {f'diffaug/{part}': t for part, t in zip(('counter', 'table'), aug.tensors())}


def named_step_state(ctx, st, prefix='', net_names=None):
    """Device state a warm-up pass of capture() advances besides weights and Adam moments, name -> tensor in a fixed order: the
    fp16 loss-scale state and the per-call dropout draw counters (every new batch size captures a new step: without this each
    capture would move them), and the image pools of a CycleGAN step, state and contents, and the draw counter of a differentiable
    augmentation.  What belongs to the step object alone (the dropout counters of its calls) is named `<prefix><attribute>.mask_draws`;
    what the step shares with the model's other steps - `ls`, `lr_now/<network>`, `pool_y/...`, `diffaug/...` - carries no prefix.
    net_names: {id(network): name}; by default the position in st.nets().  This is also the device part of a checkpoint's
    train_state (gan_amd/train_state.py)."""
    out = {}
    if ctx.ls is not None:
        out['ls'] = ctx.ls
    for i, net in enumerate(st.nets()):
        if net.params.lr_now is not None:                 # (the rate a scheduled update reports)
            out[f"lr_now/{(net_names or {}).get(id(net), i)}"] = net.params.lr_now
    seen = set()
    for attr, call in vars(st).items():
        md = getattr(call, 'mask_draws', None)
        if isinstance(md, torch.Tensor) and md.data_ptr() not in seen:
            seen.add(md.data_ptr())
            out[f'{prefix}{attr}.mask_draws'] = md
    for pool in getattr(st, 'pools', None) or ():
        out.update(pool_state(pool))
    if getattr(st, 'diffaug', None) is not None:          # (the draw counter and the table of a Pix2Pix step with --diffaugment)
        out.update(diffaug_state(st.diffaug))
    return out


def _step_state(ctx, st):
    """named_step_state with a copy of every tensor, for _restore_step_state."""
    return [(t, t.clone()) for t in named_step_state(ctx, st).values()]


def _restore_step_state(saved):
    for t, v in saved:
        t.copy_(v)


class GAN(ABC):
    def __init__(self, config):
        self.config = config
        self.ctx = Ctx(config.get('device', 'cuda:0'), config.get('dtype', 'bf16'),
                       workspace_mb=workspace_mb_for(int(config.get('batch_size', 1)), int(config.get('img_size', 256)),
                                                     int(config.get('channels', 1)),
                                                     calls=3 if int(config.get('pool_size') or 0) > 0 else 2))
        self.loss_obj = self.loss_object()

    # ---- image helpers (base_gan.py:26-61) -------------------------------------------------------
    def load(self, image_file: str, resize: bool = False):
        image = D.load(image_file, int(self.config['channels']))
        if resize:
            image = self.resize(image, self.config['img_size'], self.config['img_size'])
        return image

    def resize(self, image, height: int, width: int):
        return D.resize_nearest(image, height, width)

    def normalize(self, image):
        return D.normalize(image)

    # ---- model builders (base_gan.py:124-225) ----------------------------------------------------
    def Discriminator(self, norm_type: str = 'batchnorm', target: bool = True, seed: int = 1, name='discriminator'):
        return DiscriminatorModel(DiscriminatorNet(self.ctx, int(self.config['channels']), target, norm_type.lower(), seed), name)

    def Generator(self, norm_type='batchnorm', shape: tuple = (None, None, None), seed: int = 0, name='generator'):
        channels = shape[2] if shape[2] is not None else int(self.config['channels'])
        return GeneratorModel(GeneratorNet(self.ctx, channels, norm_type.lower(), seed), name)

    # ---- losses / optimiser (base_gan.py:227-252) ------------------------------------------------
    def loss_object(self):
        """BinaryCrossentropy(from_logits=True), or with config['gan_loss'] == 'lsgan' the mean squared error on the raw logits
        (DESIGN.md section 16): callable(target_like, logits) -> scalar tensor."""
        ctx = self.ctx
        kind = self.config.get('gan_loss', 'bce')
        if kind not in ('bce', 'lsgan'):
            raise ValueError(f"gan_loss {kind!r}: 'bce' or 'lsgan'")
        what = "lsq_logits" if kind == 'lsgan' else "bce_logits"

        def bce(y_true, logits):
            t = float(y_true) if np.isscalar(y_true) else float(torch.as_tensor(y_true).flatten()[0])
            x = logits.to(device=ctx.device, dtype=torch.float32).contiguous()
            out = torch.zeros(1, dtype=torch.float32, device=ctx.device)
            ws = torch.empty(1024, dtype=torch.float32, device=ctx.device)
            fn = getattr(ctx.lib, "gan_" + what)          # gan_bce_logits / gan_lsq_logits: the same arguments
            L.check(fn(x.data_ptr(), x.numel(), t, 1.0, 0, out.data_ptr(), 0.0, ctx.dt, None, 8, ws.data_ptr(), None, ctx.stream()), what)
            return out[0]
        return bce

    def discriminator_loss(self, real, generated, factor: float = 1.0):
        real_loss = self.loss_obj(1.0, real)
        generated_loss = self.loss_obj(0.0, generated)
        return (real_loss + generated_loss) * factor

    def optimizer(self, learning_rate: float = 2e-4, beta_1: float = 0.5, beta_2: float = 0.999):
        return AdamConfig(learning_rate, beta_1, beta_2)

    # ---- trainer core: what Pix2Pix and CycleGAN share around their captured steps (no counterpart in the reference) ----------
    def _init_trainer(self, averaged):
        """Called by a model's __init__ once its networks exist.  averaged: the generators whose weights get a moving average
        (the first one is the generator that predicts) -> one WeightAverage per generator, or None each
        without --ema-decay / --predict-weights ema."""
        self._steps = {}          # (batch, training) -> (step object, graph replay)
        self.dist = ddp.DistInfo(0, 1, self.config.get('device'))      # enable_data_parallel() replaces it in a data-parallel run
        self._rng = np.random.default_rng(int(self.config.get('seed', 123)))
        self.sync = None          # gan_amd.ddp.GradSync for data-parallel training
        self.lr_schedule = None   # nets.LrSchedule of the training steps: fit() derives it from the config
        self.learning_rates = []  # ... and notes the rate of networks()[0] at the end of every epoch
        self.averages = ()        # every replayed training step moves them
        ema_decay = float(self.config.get('ema_decay', 0.0))
        if ema_decay > 0 or str(self.config.get('predict_weights', 'raw')) == 'ema':
            warmup = str(self.config.get('ema_warmup', 'true')) == 'true'
            self.averages = tuple(WeightAverage(g, ema_decay, warmup) for g in averaged)
        self.train_state = TrainState(self)      # the checkpoint object `train_state`: what --resume continues from
        return self.averages or (None,) * len(averaged)

    def _ema_active(self):
        return bool(self.averages) and self.averages[0].decay > 0

    def enable_data_parallel(self, info, wire='bf16', exchange='allreduce'):
        """One process per GPU (torchrun): gradients are averaged over the ranks with RCCL all-reduces overlapped with the
        backward pass (gan_amd/steps.py); normalisation statistics stay per replica; the augmentation stream and the dropout
        masks differ per rank.  The reference is single-device (base_gan.py:18-19 only prints the GPU count)."""
        self.dist = info
        if info.world > 1:
            self._rng = np.random.default_rng(int(self.config.get('seed', 123)) + 7919 * info.rank)
            self.sync = ddp.GradSync([m.net.params.grad for m in self.networks()], compress_bf16=(wire == 'bf16'), lib=self.ctx.lib,
                                     exchange=exchange)

    def _step_for(self, batch, training):
        key = (batch, bool(training))
        if key not in self._steps:
            st = self._build_step(batch, training)
            st.sync = self.sync
            if training:
                st.ema = self.averages
            saved = self._snapshot()       # capture() runs warm-up passes (they also move BatchNorm's moving statistics): undo them
            extra = _step_state(self.ctx, st)
            replay = st.capture(training=training)
            self._restore(saved)
            _restore_step_state(extra)
            self._steps[key] = (st, replay)
            self.train_state.apply_pending()       # restored state of this step object: behind the undo of the warm-up, not before
        return self._steps[key]

    def _snapshot(self):
        return [(ps, ps.master.clone(), ps.m.clone(), ps.v.clone(), ps.step.clone(), {k: v.clone() for k, v in ps.state.items()})
                for ps in (m.net.params for m in self.networks())]

    def _restore(self, saved):
        for ps, w, m, v, step, state in saved:
            ps.master.copy_(w); ps.m.copy_(m); ps.v.copy_(v); ps.step.copy_(step)
            for k, t in state.items():
                ps.state[k].copy_(t)
            ps.prepare()

    def _with_lr_line(self, after_epoch=None):
        """after_epoch of run_epochs with the learning-rate line in front (a run with a schedule only)."""
        if self.lr_schedule is None:
            return after_epoch

        def lr_line(epoch):         # the rate of networks()[0] at the epoch's last update, read back from the device: one 4-byte copy
            lr = next(st for (_, tr), (st, _) in self._steps.items() if tr).current_lr()
            self.learning_rates.append(lr)
            line = after_epoch(epoch) if after_epoch is not None else None
            return f"learning rate: {lr:.3e}" + (f"\n{line}" if line else "")
        return lr_line

    def _fit(self, output_path, checkpoint_manager, keys, train_batches, val_batches, steps_per_epoch, headline, sampler, after_epoch=None,
             datasets=()):
        """The tail of fit(): train_batches() / val_batches() yield the arguments of train_step, steps_per_epoch updates per epoch;
        sampler(path) draws the sample image of an epoch.  Rank 0 alone writes checkpoints and sample images.  datasets: fit()'s
        dataset arguments, whose pass counters belong to the train_state.  A model that restored a checkpoint with a train_state
        continues behind that checkpoint's epoch; any other starts at epoch 1."""
        samples = os.path.join(output_path, 'test_images')
        if self.dist.is_main:
            os.makedirs(samples, exist_ok=True)
        save = checkpoint_manager.save if checkpoint_manager is not None else (lambda: None)
        sample = lambda epoch: sampler(os.path.join(samples, f"epoch_{epoch}.png"))
        if not self.dist.is_main:
            save = sample = (lambda *a: None)
        self.lr_schedule = lr_schedule_for(self.config, steps_per_epoch)      # (before the first training step is built and captured)
        ts = self.train_state
        resumed = ts.begin_fit(list(keys), steps_per_epoch, datasets, (self.val_quality, self.val_quality_ema))
        lr_line = self._with_lr_line(after_epoch)

        def epoch_done(epoch):      # the histories hold this epoch by now: a checkpoint written next says so
            line = lr_line(epoch) if lr_line is not None else None
            ts.epoch = epoch
            return line
        return run_epochs(self.config['epochs'], list(keys), train_batches, val_batches, self.train_step, save, sample, headline,
                          epoch_mean=lambda acc, n: ddp.mean_over_ranks(acc, n, self.dist),
                          after_pass=(self.ctx.assert_no_stack_timeout if self.ctx.use_stacks else None),
                          after_epoch=epoch_done, checkpoint_every=int(self.config.get('checkpoint_every') or 5),
                          hist=ts.hist, resumed_after=resumed[0] if resumed else 0)

    @abstractmethod
    def networks(self):
        """The model objects, generators first, in the order their step object takes them: every loop over the ParamSets goes
        through it."""

    @abstractmethod
    def _build_step(self, batch, training):
        """-> the model's step object (gan_amd/steps.py) of this batch size on the model's networks, not yet captured."""

    # ---- abstract surface, as in the reference (base_gan.py:254-292) ----------------------------
    @abstractmethod
    def image_pipeline(self, *args, **kwargs): ...

    @abstractmethod
    def generator_loss(self, *args, **kwargs): ...

    @abstractmethod
    def generate_images(self, *args, **kwargs): ...

    @abstractmethod
    def train_step(self, *args, **kwargs): ...

    @abstractmethod
    def fit(self, *args, **kwargs): ...

    @abstractmethod
    def predict(self, *args, **kwargs): ...
