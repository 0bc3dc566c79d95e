"""--resume: a run that restores the checkpoint of an interrupted run ends with the bits of the uninterrupted one.

Protocol of every case: run A is one fit() of 4 epochs with a checkpoint every 2 (ckpt-1 behind epoch 2, ckpt-2 behind epoch 4); run B
is a fresh model object that restores A's ckpt-1 and calls fit().  B's final bundle and A's ckpt-2 must hold the same keys and, under
every key, the same bytes: weights, Adam moments, moving statistics, averaged weights and all of train_state.  The tolerance is zero:
both runs make the same launches on the same inputs.

Shapes: 256 x 256 x 1 (the U-Net's minimum), batch 2 over 5 training items - batches of 2, 2 and 1, so two training step objects with
their own dropout counters, the second built lazily in the middle of an epoch - and 2 validation items."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

EPOCHS, EVERY = 4, 2


# ---- data: 8 files per directory -> 1 test, ceil(7 * 0.25) = 2 validation, 5 training ------------------------------------------------
def _examples():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'example_pairs_256.npz'))


def _variant(a, i):
    a = a[:, ::-1] if (i // 2) % 2 else a
    return np.roll(a, 16 * (i // 4), axis=0)


@pytest.fixture(scope='module')
def pair_dir(tmp_path_factory):
    """8 pair images (input | target, 256 x 512) from the two committed example pairs, mirrored and shifted."""
    from PIL import Image
    ex, d = _examples(), str(tmp_path_factory.mktemp('pairs'))
    for i in range(8):
        a, b = (_variant(ex[k][i % 2, :, :, 0], i) for k in ('input_u8', 'target_u8'))
        Image.fromarray(np.concatenate([a, b], axis=1), 'L').save(os.path.join(d, f"p{i}.png"))
    return d


@pytest.fixture(scope='module')
def unpaired_dirs(tmp_path_factory):
    from PIL import Image
    ex, root = _examples(), tmp_path_factory.mktemp('unpaired')
    dx, dy = str(root / 'X'), str(root / 'Y')
    for d, key, n in ((dx, 'input_u8', 8), (dy, 'target_u8', 7)):      # Y: ceil(7 * 0.25) = 2 validation, 5 training
        os.makedirs(d)
        for i in range(n):
            Image.fromarray(_variant(ex[key][i % 2, :, :, 0], i), 'L').save(os.path.join(d, f"s{i}.png"))
    return dx, dy


# ---- the two runs ---------------------------------------------------------------------------------------------------------------------
P2P_NAMES = ('generator_optimizer', 'discriminator_optimizer', 'generator', 'discriminator')
CYCLE_NAMES = ('generator_g', 'generator_f', 'discriminator_x', 'discriminator_y')
CYCLE_NAMES = CYCLE_NAMES + tuple(n + '_optimizer' for n in CYCLE_NAMES)


def _pix2pix(data, extra):
    from gan_amd import pix2pix
    opt = pix2pix.parse_opt(['--data', data, '--output', data, '--train', '--epochs', str(EPOCHS), '--checkpoint-every', str(EVERY),
                             '--batch-size', '2', '--test-img', '1', '--validation-size', '0.25', *extra])
    from gan_amd.runner import config_of
    return pix2pix.Pix2Pix(config_of(opt)), P2P_NAMES


def _cyclegan(dirs, extra):
    from gan_amd import cycle_gan
    from gan_amd.runner import config_of
    opt = cycle_gan.parse_opt(['--input-images', dirs[0], '--target-images', dirs[1], '--output', dirs[0], '--train', '--epochs', str(EPOCHS),
                               '--checkpoint-every', str(EVERY), '--batch-size', '2', '--test-img', '1', '--validation-size', '0.25', *extra])
    return cycle_gan.CycleGAN(config_of(opt)), CYCLE_NAMES


def _objects(model, names, train_state=True):
    objects = {n: getattr(model, n) for n in names}
    objects.update({avg.model.obj_name + '_ema': avg for avg in model.averages})
    if train_state:
        objects['train_state'] = model.train_state
    return objects


def _fit(model, names, out, restore=None):
    """restore: None, or a callable(model, names) that restores a checkpoint into the model.  -> (histories, checkpoint directory)"""
    from gan_amd.checkpoint import Checkpoint, CheckpointManager
    checkpoint = Checkpoint(**_objects(model, names))
    if restore is not None:
        checkpoint.save_counter = restore(model, names)
    ck = os.path.join(str(out), 'training_checkpoints')
    manager = CheckpointManager(checkpoint, ck, max_to_keep=2)
    *train_val, test = model.image_pipeline(predict=False)
    assert len(train_val[0]) == 3 and len(train_val[0].files) == 5 and len(train_val[-1].files) == 2        # batches of 2, 2, 1; 2 validation items
    hist = model.fit(*train_val, test, str(out), checkpoint_manager=manager)
    return hist, ck


def _restore_all(prefix):
    def restore(model, names):
        from gan_amd.checkpoint import Checkpoint
        return Checkpoint(**_objects(model, names)).restore(prefix).save_counter
    return restore


def _restore_without_device_state(prefix):
    """The negative control's restore: everything but the `train_state/device/...` entries."""
    def restore(model, names):
        from gan_amd import tfbundle
        from gan_amd.checkpoint import Checkpoint
        counter = Checkpoint(**_objects(model, names, train_state=False)).restore(prefix).save_counter
        arrays = tfbundle.read_bundle(prefix)[0]
        lead = 'train_state/'
        host = {k[len(lead):]: v for k, v in arrays.items() if k.startswith(lead) and not k.startswith(lead + 'device/')}
        assert len(host) < sum(k.startswith(lead) for k in arrays)          # (there was device state to leave out)
        model.train_state.load_state_dict(host)
        return counter
    return restore


def _bundle(prefix):
    from gan_amd import tfbundle
    return tfbundle.read_bundle(prefix)[0]


def _unequal_keys(a, b):
    """Keys under which two bundles differ in dtype, shape or bytes."""
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    return sorted(k for k in a if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
                  or not np.array_equal(np.ascontiguousarray(a[k]).reshape(-1).view(np.uint8), np.ascontiguousarray(b[k]).reshape(-1).view(np.uint8)))


_runs_a = {}


def _run_a(case, make, tmp_path_factory):
    """Run A of a case, once per module: (histories, checkpoint directory)."""
    if case not in _runs_a:
        model, names = make()
        _runs_a[case] = _fit(model, names, tmp_path_factory.mktemp(f'a_{case}'))
        ck = _runs_a[case][1]
        assert sorted(os.listdir(ck)) == ['checkpoint', 'ckpt-1.data-00000-of-00001', 'ckpt-1.index', 'ckpt-2.data-00000-of-00001', 'ckpt-2.index']
    return _runs_a[case]


def _same_histories(a, b):
    for ha, hb in zip(a, b):
        assert list(ha) == list(hb)
        for k in ha:
            assert len(hb[k]) == EPOCHS and np.array_equal(np.array(ha[k]), np.array(hb[k]), equal_nan=True), (k, ha[k], hb[k])


def _check_resumed_equals_straight(case, make, tmp_path_factory, tmp_path, expect_keys):
    hist_a, ck_a = _run_a(case, make, tmp_path_factory)
    first = _bundle(os.path.join(ck_a, 'ckpt-1'))
    assert int(first['train_state/epoch']) == 2 and int(first['train_state/steps_per_epoch']) == 3
    for k in expect_keys:
        assert 'train_state/device/' + k in first, (k, sorted(x for x in first if x.startswith('train_state/device/')))
    model, names = make()
    hist_b, ck_b = _fit(model, names, tmp_path, restore=_restore_all(os.path.join(ck_a, 'ckpt-1')))
    assert sorted(os.listdir(ck_b)) == ['checkpoint', 'ckpt-2.data-00000-of-00001', 'ckpt-2.index']       # epochs 3 and 4 alone ran
    assert os.listdir(os.path.join(str(tmp_path), 'test_images')) == ['epoch_2.png']      # the sample that followed the checkpoint
    assert _unequal_keys(_bundle(os.path.join(ck_a, 'ckpt-2')), _bundle(os.path.join(ck_b, 'ckpt-2'))) == []
    _same_histories(hist_a, hist_b)
    return model


P2P_BF16 = ['--dtype', 'bf16', '--diffaugment', 'translation,cutout,brightness,saturation', '--ema-decay', '0.9', '--lr-decay-epochs', '2',
            '--data-cache', 'host']
# both training step objects and the validation step own dropout counters; the rest is the model's
P2P_BF16_KEYS = ('b2.train/g.mask_draws', 'b1.train/g.mask_draws', 'b2.val/g.mask_draws', 'diffaug/counter', 'diffaug/table',
                 'lr_now/generator', 'lr_now/discriminator')


def test_pix2pix_bf16_diffaugment_ema_lr_decay(pair_dir, tmp_path_factory, tmp_path):
    model = _check_resumed_equals_straight('p2p_bf16', lambda: _pix2pix(pair_dir, P2P_BF16), tmp_path_factory, tmp_path, P2P_BF16_KEYS)
    assert len(model.learning_rates) == EPOCHS and model.train_state.pending == {}


def test_pix2pix_f16_loss_scale_device_cache(pair_dir, tmp_path_factory, tmp_path):
    extra = ['--dtype', 'f16', '--data-cache', 'device']
    _check_resumed_equals_straight('p2p_f16', lambda: _pix2pix(pair_dir, extra), tmp_path_factory, tmp_path,
                                   ('ls', 'b2.train/g.mask_draws', 'b1.train/g.mask_draws'))


def test_cyclegan_bf16_pool_ema_lr_decay(unpaired_dirs, tmp_path_factory, tmp_path):
    """(--data-cache device: its jitter is drawn in the consuming thread, X before Y per batch; the host cache's two decode threads
    share the model's generator and race for it, so two host-cache runs of one command need not see the same crops.)"""
    extra = ['--dtype', 'bf16', '--pool-size', '4', '--lr-decay-epochs', '2', '--ema-decay', '0.9', '--data-cache', 'device']
    hist_a, ck_a = _run_a('cycle_bf16', lambda: _cyclegan(unpaired_dirs, extra), tmp_path_factory)
    first = _bundle(os.path.join(ck_a, 'ckpt-1'))
    state = first['train_state/device/pool_y/state']
    assert state[0] == 4 and first['train_state/device/pool_y/storage'].any()        # full (and swapping) well before the checkpoint
    _check_resumed_equals_straight('cycle_bf16', lambda: _cyclegan(unpaired_dirs, extra), tmp_path_factory, tmp_path,
                                   ('pool_x/state', 'pool_x/storage', 'pool_y/state', 'pool_y/storage', 'lr_now/generator_g'))


def test_without_the_device_state_the_runs_differ(pair_dir, tmp_path_factory, tmp_path):
    """Negative control: the same protocol with the device entries of train_state left out of the restore (dropout and DiffAugment
    counters restart at zero) must NOT reproduce run A - the comparison above can see that state."""
    make = lambda: _pix2pix(pair_dir, P2P_BF16)
    hist_a, ck_a = _run_a('p2p_bf16', make, tmp_path_factory)
    model, names = make()
    hist_b, ck_b = _fit(model, names, tmp_path, restore=_restore_without_device_state(os.path.join(ck_a, 'ckpt-1')))
    differ = _unequal_keys(_bundle(os.path.join(ck_a, 'ckpt-2')), _bundle(os.path.join(ck_b, 'ckpt-2')))
    assert any(k.startswith('generator/') for k in differ) and any(k.startswith('train_state/device/') for k in differ), differ
    key = 'Generator Total Loss'
    assert hist_b[0][key][:2] == hist_a[0][key][:2] and hist_b[0][key][2:] != hist_a[0][key][2:]


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def _cli(data, out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'pix2pix.py'), '--data', data, '--output', str(out), '--train', '--batch-size', '2',
           '--test-img', '1', '--validation-size', '0.25', '--logging', 'false', '--checkpoint-every', '1', *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    run = os.path.join(str(out), sorted(os.listdir(str(out)))[0])
    return run, os.path.join(run, 'training_checkpoints')


def test_cli_resume_in_a_child_process(pair_dir, tmp_path):
    """`pix2pix.py --train --epochs 2 --checkpoint-every 1` straight, against `--resume .../ckpt-1 --epochs 2` in a process of its own.
    The driver keeps one checkpoint (max_to_keep 1, the reference's), so the straight run's own ckpt-1 is gone when it ends: the
    interrupted run is the same command stopped behind epoch 1 (--epochs 1; without a learning-rate schedule the resumed run may ask
    for more epochs than the interrupted one), and its ckpt-1 is what the straight run had written there."""
    straight, ck_s = _cli(pair_dir, tmp_path / 'straight', '--epochs', '2')
    _, ck_i = _cli(pair_dir, tmp_path / 'interrupted', '--epochs', '1')
    resumed, ck_r = _cli(pair_dir, tmp_path / 'resumed', '--epochs', '2', '--resume', os.path.join(ck_i, 'ckpt-1'))
    metrics = [json.load(open(os.path.join(run, 'logs', name))) for run in (straight, resumed) for name in ('train_metrics.json', 'val_metrics.json')]
    assert all(len(v) == 2 for m in metrics for v in m.values())
    assert metrics[0] == metrics[2] and metrics[1] == metrics[3]
    assert sorted(os.listdir(ck_r)) == ['checkpoint', 'ckpt-2.data-00000-of-00001', 'ckpt-2.index']
    assert _unequal_keys(_bundle(os.path.join(ck_s, 'ckpt-2')), _bundle(os.path.join(ck_r, 'ckpt-2'))) == []
    assert sorted(os.listdir(os.path.join(resumed, 'test_images'))) == ['epoch_1.png']
