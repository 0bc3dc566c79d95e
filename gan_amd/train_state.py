"""What a training run needs beside weights, Adam moments and averaged weights to continue bit for bit (no
counterpart in the reference, which cannot continue a run): `TrainState` is the checkpoint object `train_state` of a model
(gan_amd/checkpoint.py: `state_dict()` / `load_state_dict()`), written into the same TensorBundle as everything else under
`train_state/...`, so it lives and dies with its `ckpt-N`.

Host part: the completed epoch, the updates per epoch, the loss / learning-rate / quality histories, the augmentation generator,
the pass counters of the datasets and the run-defining part of the config.  Device part (`device/...`): what
`base_gan._step_state` enumerates - the fp16 loss-scale word, every network's `lr_now`, the dropout draw counters of every captured
step object, the image pools and the DiffAugment counter and table - under stable names.  Step objects are built lazily: an entry
whose tensor does not exist yet is held and applied by `GAN._step_for` once the step exists, after the capture's warm-up has been
undone.

`check_resume` is the gate of `--resume` (runner.drive): it reads a bundle without a GPU and refuses what cannot be continued."""
from __future__ import annotations

import json
import os

import numpy as np

from . import tfbundle
from .checkpoint import latest_checkpoint

NAME = 'train_state'
DEVICE = 'device/'
# what shapes the trajectory of a run: a resumed run must agree with the stored one in all of it (epochs: see check_config)
CONFIG_KEYS = ('batch_size', 'img_size', 'channels', 'dtype', 'seed', 'learning_rate', 'beta_1', 'beta_2', 'lambda', 'gan_loss',
               'generator_loss', 'diffaugment', 'pool_size', 'ema_decay', 'ema_warmup', 'lr_decay_epochs', 'lr_end_factor', 'data_cache',
               'validation_size', 'test_img', 'input_img_orient')
PATH_KEYS = ('data', 'input_images', 'target_images')
# run-defining keys that joined after checkpoints were first written: a stored config without one holds its default
LATER_KEYS = ('edge_weight', 'msssim_alpha', 'preprocess_input', 'preprocess_target', 'clahe_clip', 'clahe_grid', 'blur_sigma')
_DEFAULTS = {'edge_weight': 0.0, 'msssim_alpha': 0.84, 'preprocess_input': '', 'preprocess_target': '', 'clahe_clip': 1.0, 'clahe_grid': 15,
             'blur_sigma': 0.5, 'diffaugment': '', 'pool_size': 0, 'ema_decay': 0.0, 'lr_decay_epochs': 0, 'lr_end_factor': 0.0, 'gan_loss': 'bce',
             'data_cache': 'host', 'ema_warmup': 'true', 'dtype': 'bf16', 'seed': 123}


class ResumeRefused(SystemExit):
    """--resume cannot continue this checkpoint with this command line; the message names the offending key."""


def _canonical(key, value):
    """A config value as it is compared and stored: a missing one is its default, numbers compare as numbers ('1' == 1), paths as
    absolute paths."""
    if value is None:
        value = _DEFAULTS.get(key)
    if value is None:
        return None
    if key in PATH_KEYS:
        return os.path.abspath(str(value))
    if isinstance(value, bool):
        return 'true' if value else 'false'
    try:
        return float(value)
    except (TypeError, ValueError):
        return str(value)


def run_config(config) -> dict:
    """The run-defining part of a model's config (JSON-ready)."""
    out = {k: _canonical(k, config.get(k)) for k in CONFIG_KEYS + PATH_KEYS + LATER_KEYS}
    out['epochs'] = None if config.get('epochs') is None else int(config['epochs'])
    return out


def check_config(stored: dict, config) -> None:
    """Refuse (ResumeRefused) a run whose config differs from the stored one in anything that shapes the trajectory.  epochs may
    grow when there is no learning-rate schedule (training longer at the constant rate); with a schedule it must match, since the
    schedule's end is part of every update's rate."""
    now = run_config(config)
    for k in CONFIG_KEYS + PATH_KEYS:
        if stored.get(k) != now[k]:
            raise ResumeRefused(f"--resume: {k} differs from the checkpoint's run: stored {stored.get(k)!r}, this run {now[k]!r}")
    for k in LATER_KEYS:
        was = _canonical(k, stored.get(k))
        if was != now[k]:
            raise ResumeRefused(f"--resume: {k} differs from the checkpoint's run: stored {was!r}, this run {now[k]!r}")
    was, is_ = stored.get('epochs'), now['epochs']
    if was is not None and is_ is not None and was != is_:
        if now['lr_decay_epochs']:
            raise ResumeRefused(f"--resume: epochs differs from the checkpoint's run (stored {was}, this run {is_}) and the run has a "
                                "learning-rate schedule (lr_decay_epochs), whose rates depend on it")
        if is_ < was:
            raise ResumeRefused(f"--resume: epochs {is_} is less than the checkpoint's run had ({was})")


def _json_array(obj) -> np.ndarray:
    return np.frombuffer(json.dumps(obj, sort_keys=True).encode(), dtype=np.uint8).copy()


def _from_json_array(a):
    return json.loads(np.asarray(a, dtype=np.uint8).tobytes().decode())


_MASK64 = (1 << 64) - 1


def rng_to_array(rng) -> np.ndarray:
    """numpy's PCG64 generator state as six uint64: state low / high, increment low / high, has_uint32, uinteger."""
    s = rng.bit_generator.state
    if s.get('bit_generator') != 'PCG64':
        raise TypeError(f"generator {s.get('bit_generator')!r}: only PCG64 (numpy.random.default_rng) is stored")
    st, inc = int(s['state']['state']), int(s['state']['inc'])
    return np.array([st & _MASK64, st >> 64, inc & _MASK64, inc >> 64, int(s['has_uint32']), int(s['uinteger'])], dtype=np.uint64)


def rng_from_array(rng, a) -> None:
    v = [int(x) for x in np.asarray(a, dtype=np.uint64).reshape(6)]
    rng.bit_generator.state = {'bit_generator': 'PCG64', 'state': {'state': v[0] | (v[1] << 64), 'inc': v[2] | (v[3] << 64)},
                               'has_uint32': v[4], 'uinteger': v[5]}


def _table(keys, per_key) -> np.ndarray:
    """{key: [per-epoch value, ...]} -> float64 [len(keys), epochs] (the shortest history decides: all of them grow together)."""
    n = min((len(per_key[k]) for k in keys), default=0)
    return np.array([[float(v) for v in per_key[k][:n]] for k in keys], dtype=np.float64).reshape(len(keys), n)


def _untable(keys, table) -> dict:
    t = np.asarray(table, dtype=np.float64)
    t = t.reshape(len(keys), t.size // max(len(keys), 1))
    return {k: [float(v) for v in row] for k, row in zip(keys, t)}


def device_to_numpy(t) -> np.ndarray:
    """A device tensor as the array the bundle stores: bf16 has no numpy dtype and travels as its uint16 bit pattern."""
    import torch
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def numpy_into_device(name, a, t) -> None:
    """t <- the stored array `a`, by its bytes; the size must be the tensor's (anything else is another run's state)."""
    import torch
    a = np.ascontiguousarray(a)
    if a.nbytes != t.numel() * t.element_size():
        raise ValueError(f"train_state {name}: stored {a.nbytes} bytes ({a.dtype} {a.shape}), the run's tensor holds "
                         f"{t.numel() * t.element_size()} ({t.dtype} {tuple(t.shape)})")
    raw = torch.from_numpy(a.reshape(-1).view(np.uint8).copy())
    t.copy_(raw.view(t.dtype).view(t.shape))


class TrainState:
    """The `train_state` checkpoint object of a GAN model (base_gan.GAN._init_trainer makes it)."""

    def __init__(self, model):
        self.model = model
        self.epoch = 0                  # epochs completed (the checkpoint is written after this one)
        self.steps_per_epoch = 0
        self.keys = []                  # loss keys, in the model's order
        self.hist = ({}, {})            # (train, val): {key: [epoch mean, ...]} - the very dicts fit() returns
        self.quality = ({}, {})         # (raw, averaged weights): the model's val_quality / val_quality_ema of this fit
        self.datasets = ()              # the counted datasets of this fit, in fit()'s argument order
        self.restored = False           # load_state_dict found a state: the next fit() continues it
        self.stored_config = None
        self.pending = {}               # device entries that wait for their tensors: name -> array
        self._data_epochs = None

    # ---- the names of the device state -----------------------------------------------------------------------------------------
    def device_tensors(self):
        """name -> tensor of every piece of device state that exists right now: the model-level ones once (they are shared by the
        step objects of every batch size), the per-step ones under `b<batch>.<train|val>/`, and the dropout counters of the
        generators' own calls (the sample image of an epoch is one)."""
        from .base_gan import diffaug_state, named_step_state, pool_state
        m, out = self.model, {}
        names = {id(net.net): net.obj_name for net in m.networks()}
        for (batch, training), (st, _) in m._steps.items():
            prefix = f"b{batch}.{'train' if training else 'val'}/"
            for name, t in named_step_state(m.ctx, st, prefix, names).items():
                out.setdefault(name, t)
        if m.ctx.ls is not None:                 # the model's own, whether or not a step exists yet
            out.setdefault('ls', m.ctx.ls)
        for pool in getattr(m, 'pools', None) or ():
            for name, t in pool_state(pool).items():
                out.setdefault(name, t)
        if getattr(m, 'diffaug', None) is not None:
            for name, t in diffaug_state(m.diffaug).items():
                out.setdefault(name, t)
        for net in m.networks():
            for (B, S), call in getattr(net, '_calls', {}).items():
                md = getattr(call, 'mask_draws', None)
                if md is not None:
                    out[f"calls/{net.obj_name}/b{B}.s{S}/mask_draws"] = md
        return out

    def apply_pending(self):
        """Write every held entry whose tensor exists by now (GAN._step_for calls this behind the warm-up's undo)."""
        if not self.pending:
            return
        live = self.device_tensors()
        for name in [n for n in self.pending if n in live]:
            numpy_into_device(name, self.pending.pop(name), live[name])
        for net in self.model.networks():       # a generator's own call is built by its first use: the model object applies these
            held = getattr(net, '_restored_draws', None)
            if held is None:
                continue
            lead = f"calls/{net.obj_name}/"
            for name in [n for n in self.pending if n.startswith(lead) and n.endswith('/mask_draws')]:
                b, s = name[len(lead):-len('/mask_draws')].split('.')
                held[(int(b[1:]), int(s[1:]))] = self.pending.pop(name)

    # ---- fit() ----------------------------------------------------------------------------------------------------------------
    def begin_fit(self, keys, steps_per_epoch, datasets, quality):
        """Called by GAN._fit.  -> None for a fresh run, or (completed epoch, (train, val) histories) to continue from: the
        histories, learning rates, quality histories and dataset counters are then the restored ones."""
        m = self.model
        self.keys, self.datasets, self.quality = list(keys), tuple(datasets), tuple(quality)
        if not self.restored:
            self.epoch, self.steps_per_epoch = 0, int(steps_per_epoch)
            self.hist = ({k: [] for k in self.keys}, {k: [] for k in self.keys})
            m.learning_rates = []
            return None
        self.restored = False
        if int(steps_per_epoch) != self.steps_per_epoch:
            raise ResumeRefused(f"--resume: steps_per_epoch differs from the checkpoint's run: stored {self.steps_per_epoch}, this run "
                                f"{steps_per_epoch} (another dataset?)")
        if list(self.hist[0]) != self.keys:
            raise ResumeRefused(f"--resume: the checkpoint's loss keys {list(self.hist[0])} are not this model's {self.keys}")
        if self._data_epochs is not None:
            if len(self._data_epochs) != len(self.datasets):
                raise ResumeRefused(f"--resume: the checkpoint counts {len(self._data_epochs)} datasets, this run {len(self.datasets)}")
            for d, e in zip(self.datasets, self._data_epochs):
                if hasattr(d, 'epoch'):
                    d.epoch = int(e)
        for mine, stored in zip(self.quality, self._quality):
            for k in mine:
                mine[k][:] = stored.get(k, [])
        m.learning_rates = list(self._learning_rates)
        return self.epoch, self.hist

    # ---- checkpoint object ------------------------------------------------------------------------------------------------------
    def state_dict(self):
        m = self.model
        qkeys = [list(q) for q in self.quality]
        out = {'epoch': np.array(self.epoch, np.int64),
               'steps_per_epoch': np.array(self.steps_per_epoch, np.int64),
               'history/keys': _json_array(self.keys),
               'history/train': _table(self.keys, self.hist[0]),
               'history/val': _table(self.keys, self.hist[1]),
               'learning_rates': np.array([float(v) for v in m.learning_rates], dtype=np.float64),
               'quality/keys': _json_array(qkeys),
               'quality/raw': _table(qkeys[0], self.quality[0]) if qkeys[0] else np.zeros((0, 0)),
               'quality/averaged': _table(qkeys[1], self.quality[1]) if qkeys[1] else np.zeros((0, 0)),
               'rng': rng_to_array(m._rng),
               'data/epochs': np.array([int(getattr(d, 'epoch', 0)) for d in self.datasets], dtype=np.int64),
               'config': _json_array(run_config(m.config))}
        for name, t in self.device_tensors().items():
            out[DEVICE + name] = device_to_numpy(t)
        for name, a in self.pending.items():        # restored, never needed since (a batch size that did not come up again): kept
            out.setdefault(DEVICE + name, np.asarray(a))
        return out

    def load_state_dict(self, sd):
        """Nothing among `sd` (a checkpoint written before there was a train_state): nothing happens and `restored` is False."""
        if 'epoch' not in sd:
            self.restored = False
            return
        m = self.model
        self.epoch = int(np.asarray(sd['epoch']).reshape(-1)[0])
        self.steps_per_epoch = int(np.asarray(sd['steps_per_epoch']).reshape(-1)[0])
        self.keys = list(_from_json_array(sd['history/keys']))
        self.hist = (_untable(self.keys, sd['history/train']), _untable(self.keys, sd['history/val']))
        self._learning_rates = [float(v) for v in np.asarray(sd['learning_rates']).reshape(-1)]
        qkeys = _from_json_array(sd['quality/keys'])
        self._quality = tuple(_untable(k, sd[n]) if k else {} for k, n in zip(qkeys, ('quality/raw', 'quality/averaged')))
        rng_from_array(m._rng, sd['rng'])
        self._data_epochs = [int(v) for v in np.asarray(sd['data/epochs']).reshape(-1)]
        self.stored_config = _from_json_array(sd['config'])
        self.pending = {k[len(DEVICE):]: np.array(v) for k, v in sd.items() if k.startswith(DEVICE)}
        self.apply_pending()
        self.restored = True


# ---- the gate of --resume ----------------------------------------------------------------------------------------------------------
def resume_prefix(path: str) -> str:
    """PATH of --resume -> checkpoint prefix: a training_checkpoints directory means its latest checkpoint, anything else is a
    prefix `.../ckpt-N`."""
    prefix = latest_checkpoint(path) if os.path.isdir(path) else path
    if prefix is None or not os.path.exists(prefix + '.index'):
        raise ResumeRefused(f"--resume: no checkpoint at {path!r} (a training_checkpoints directory or a prefix .../ckpt-N)")
    return prefix


def check_resume(path: str, config, world: int = 1) -> str:
    """-> the checkpoint prefix to restore, or ResumeRefused: data-parallel runs, a checkpoint without train_state, a config that
    differs in what shapes the trajectory (check_config), nothing left to do."""
    if world > 1:
        raise ResumeRefused("--resume: data-parallel runs (world > 1) cannot be resumed yet: only rank 0 writes checkpoints, and the "
                            "other ranks' augmentation generators, dropout counters and pool contents are not in them")
    prefix = resume_prefix(path)
    arrays = tfbundle.read_bundle(prefix)[0]
    lead = NAME + '/'
    if lead + 'epoch' not in arrays or lead + 'config' not in arrays:
        raise ResumeRefused(f"--resume: {prefix} holds no train_state (it was written before training state was saved); continuing from "
                            "the weights alone would not be a resume")
    check_config(_from_json_array(arrays[lead + 'config']), config)
    done, epochs = int(np.asarray(arrays[lead + 'epoch']).reshape(-1)[0]), int(config['epochs'])
    if done >= epochs:
        raise ResumeRefused(f"--resume: epochs {epochs}: the checkpoint was written after epoch {done}, there is nothing left to do")
    return prefix
