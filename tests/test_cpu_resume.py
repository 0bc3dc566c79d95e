"""--resume / --checkpoint-every without a GPU: the flags, every refusal of the resume gate against small
hand-made bundles, the cadence of the epoch driver, and train_state's round trip through the TensorBundle container."""
import os
import types

import numpy as np
import pytest
import torch

from gan_amd import cycle_gan, pix2pix, runner, tfbundle
from gan_amd import train_state as T
from gan_amd.checkpoint import Checkpoint, CheckpointManager


def _p2p_args(*extra):
    return ['--data', 'd', '--output', 'o', *extra]


def _cycle_args(*extra):
    return ['--input-images', 'x', '--target-images', 'y', '--output', 'o', *extra]


# ---- flags ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('parse, args', [(pix2pix.parse_opt, _p2p_args), (cycle_gan.parse_opt, _cycle_args)])
def test_flags_and_their_defaults(parse, args, capsys):
    opt = parse(args('--train', '--epochs', '3'))
    assert opt.resume is None and opt.checkpoint_every == 5                    # the reference's cadence
    opt = parse(args('--train', '--epochs', '3', '--resume', 'runs/training_checkpoints/ckpt-2', '--checkpoint-every', '2'))
    assert opt.resume == 'runs/training_checkpoints/ckpt-2' and opt.checkpoint_every == 2
    assert runner.config_of(opt)['checkpoint_every'] == 2
    for bad, word in ((args('--predict', '--weights', 'w', '--resume', 'c'), '--resume'),
                      (args('--train', '--epochs', '3', '--checkpoint-every', '0'), '--checkpoint-every')):
        with pytest.raises(SystemExit):
            parse(bad)
        assert word in capsys.readouterr().err


# ---- the epoch driver's cadence -----------------------------------------------------------------------------------------------------
def _drive(epochs, **kw):
    events = []
    step = lambda x, training: (torch.tensor(float(x)), torch.tensor(1.0))
    after = lambda epoch: events.append(('epoch', epoch))
    hist = runner.run_epochs(epochs, ['a', 'b'], lambda: [(1.0,), (3.0,)], lambda: [(5.0,)], step, lambda: events.append(('checkpoint', events[-1][1])),
                             lambda epoch: events.append(('sample', epoch)), ('a', 'b'), after_epoch=after, **kw)
    return hist, [e for e in events if e[0] != 'epoch']


def test_checkpoint_cadence(capsys):
    hist, events = _drive(11)
    assert events == [('checkpoint', 5), ('sample', 5), ('checkpoint', 10), ('sample', 10), ('checkpoint', 11)]       # every 5th and the last
    assert hist[0]['a'] == [2.0] * 11 and hist[1]['a'] == [5.0] * 11
    _, events = _drive(5, checkpoint_every=2)
    assert events == [('checkpoint', 2), ('sample', 2), ('checkpoint', 4), ('sample', 4), ('checkpoint', 5)]
    _, events = _drive(1)
    assert events == [('checkpoint', 1)]


def test_resumed_driver_continues_behind_the_checkpoint(capsys):
    before = ({'a': [9.0, 8.0], 'b': [1.0, 1.0]}, {'a': [7.0, 6.0], 'b': [1.0, 1.0]})
    hist, events = _drive(4, checkpoint_every=2, hist=before, resumed_after=2)
    assert events == [('sample', 2), ('checkpoint', 4)]        # the sample that followed ckpt behind epoch 2, then epochs 3 and 4
    assert hist is before and hist[0]['a'] == [9.0, 8.0, 2.0, 2.0] and hist[1]['a'] == [7.0, 6.0, 5.0, 5.0]
    _, events = _drive(4, checkpoint_every=2, hist=({'a': [0.0] * 3, 'b': [0.0] * 3},) * 2, resumed_after=3)
    assert events == [('checkpoint', 4)]                         # epoch 3 wrote no checkpoint under this cadence: no sample either


# ---- the gate -------------------------------------------------------------------------------------------------------------------------
CONFIG = {'data': 'some/data', 'batch_size': 2, 'img_size': 256, 'channels': '1', 'dtype': 'bf16', 'seed': 123, 'learning_rate': 2e-4,
          'beta_1': 0.5, 'beta_2': 0.999, 'lambda': 100, 'gan_loss': 'bce', 'generator_loss': 'l1', 'diffaugment': 'translation,cutout',
          'pool_size': 4, 'ema_decay': 0.9, 'ema_warmup': 'true', 'lr_decay_epochs': 0, 'lr_end_factor': 0.0, 'data_cache': 'host',
          'validation_size': 0.25, 'test_img': 1, 'input_img_orient': 'left', 'input_images': 'in/x', 'target_images': 'in/y', 'epochs': 4}


def _bundle(directory, config=CONFIG, epoch=2, n=1, with_state=True):
    os.makedirs(directory, exist_ok=True)
    arrays = {'generator/layer_with_weights-15/bias/.ATTRIBUTES/VARIABLE_VALUE': np.zeros(1, np.float32)}
    if with_state:
        arrays.update({'train_state/epoch': np.array(epoch, np.int64), 'train_state/config': T._json_array(T.run_config(config))})
    prefix = tfbundle.write_bundle(os.path.join(str(directory), f'ckpt-{n}'), arrays)
    with open(os.path.join(str(directory), 'checkpoint'), 'w') as f:
        f.write(f'model_checkpoint_path: "ckpt-{n}"\n')
    return prefix


def test_gate_accepts_the_same_run(tmp_path):
    prefix = _bundle(tmp_path)
    assert T.check_resume(prefix, CONFIG) == prefix
    assert T.check_resume(str(tmp_path), CONFIG) == prefix                        # a directory means its latest checkpoint
    assert T.check_resume(prefix, {**CONFIG, 'channels': 1, 'lambda': 100.0, 'data': os.path.abspath('some/data')}) == prefix
    assert T.check_resume(prefix, {**CONFIG, 'output': 'elsewhere', 'checkpoint_every': 1, 'logging': 'false'}) == prefix
    assert issubclass(T.ResumeRefused, SystemExit)


CHANGED = {'batch_size': 4, 'img_size': 512, 'channels': '3', 'dtype': 'f16', 'seed': 7, 'learning_rate': 1e-4, 'beta_1': 0.6, 'beta_2': 0.99,
           'lambda': 10, 'gan_loss': 'lsgan', 'generator_loss': 'dssim', 'diffaugment': 'cutout', 'pool_size': 50, 'ema_decay': 0.999,
           'ema_warmup': 'false', 'lr_decay_epochs': 2, 'lr_end_factor': 0.5, 'data_cache': 'device', 'validation_size': 0.1, 'test_img': 2,
           'input_img_orient': 'right', 'data': 'other/data', 'input_images': 'other/x', 'target_images': 'other/y'}


def test_every_trajectory_key_is_covered():
    assert set(CHANGED) == set(T.CONFIG_KEYS + T.PATH_KEYS)
    assert set(CHANGED) <= set(CONFIG)


@pytest.mark.parametrize('key', sorted(CHANGED))
def test_gate_refuses_a_changed_config(tmp_path, key):
    prefix = _bundle(tmp_path)
    with pytest.raises(T.ResumeRefused) as e:
        T.check_resume(prefix, {**CONFIG, key: CHANGED[key]})
    assert f' {key} ' in str(e.value)


def test_gate_epochs(tmp_path):
    prefix = _bundle(tmp_path)
    assert T.check_resume(prefix, {**CONFIG, 'epochs': 9}) == prefix              # longer at the constant rate
    for epochs in (2, 1):                                                         # written after epoch 2: nothing left
        with pytest.raises(T.ResumeRefused, match='epochs'):
            T.check_resume(prefix, {**CONFIG, 'epochs': epochs})
    with pytest.raises(T.ResumeRefused, match='epochs 3 is less'):
        T.check_resume(prefix, {**CONFIG, 'epochs': 3})
    scheduled = {**CONFIG, 'lr_decay_epochs': 2}
    prefix = _bundle(tmp_path / 's', scheduled)
    assert T.check_resume(prefix, scheduled) == prefix
    with pytest.raises(T.ResumeRefused, match='epochs differs .* learning-rate schedule'):
        T.check_resume(prefix, {**scheduled, 'epochs': 9})


def test_gate_refuses_old_checkpoints_missing_ones_and_data_parallel_runs(tmp_path):
    old = _bundle(tmp_path / 'old', with_state=False)
    with pytest.raises(T.ResumeRefused, match='no train_state'):
        T.check_resume(old, CONFIG)
    for missing in (str(tmp_path / 'nowhere'), str(tmp_path / 'old' / 'ckpt-7')):
        with pytest.raises(T.ResumeRefused, match='no checkpoint'):
            T.check_resume(missing, CONFIG)
    os.makedirs(tmp_path / 'empty')
    with pytest.raises(T.ResumeRefused, match='no checkpoint'):
        T.check_resume(str(tmp_path / 'empty'), CONFIG)
    with pytest.raises(T.ResumeRefused, match='data-parallel'):
        T.check_resume(_bundle(tmp_path / 'new'), CONFIG, world=2)


def test_driver_refuses_before_it_creates_a_run_directory(tmp_path):
    old = _bundle(tmp_path / 'old', with_state=False)
    opt = pix2pix.parse_opt(['--data', str(tmp_path), '--output', str(tmp_path / 'out'), '--train', '--epochs', '3', '--resume', old,
                             '--device', 'cpu'])
    with pytest.raises(SystemExit, match='no train_state'):
        pix2pix.main(opt)
    assert not os.path.exists(tmp_path / 'out')


# ---- train_state through the container ----------------------------------------------------------------------------------------------
class _Pool:
    def __init__(self, stream_id, fill):
        self.stream_id = stream_id
        self.state = torch.tensor([4, 9, 2], dtype=torch.int32)
        self.storage = torch.full((4, 2, 2, 1), fill, dtype=torch.bfloat16)

    def tensors(self):
        return [self.state, self.storage]


class _Data:
    def __init__(self, epoch):
        self.epoch = epoch


def _model(seed, draws=0, pools=True, ls=True):
    """What TrainState reads of a model, on the host: config, generator, learning rates, loss-scale word, pools, no steps yet."""
    from gan_amd.pool import STREAM_X, STREAM_Y
    m = types.SimpleNamespace(config=dict(CONFIG), _rng=np.random.default_rng(seed), learning_rates=[], _steps={}, networks=lambda: (),
                              ctx=types.SimpleNamespace(ls=torch.tensor([32768.0, 1 / 32768.0, 0.0, 17.0]) if ls else None),
                              pools=(_Pool(STREAM_Y, 0.5), _Pool(STREAM_X, -0.25)) if pools else None, diffaug=None)
    for _ in range(draws):
        m._rng.integers(0, 31), m._rng.random()
    m.train_state = T.TrainState(m)
    return m


def test_train_state_round_trip(tmp_path):
    a = _model(123, draws=11)
    a._rng.integers(0, 2 ** 32, dtype=np.uint32)                 # (PCG64 keeps the other half of a 64-bit draw: has_uint32 / uinteger)
    ts = a.train_state
    keys = ['Generator Total Loss', 'Discriminator Loss']
    quality = ({'SSIM': [], 'PSNR': []}, {'SSIM': [], 'PSNR': []})
    data = (_Data(0), _Data(0), _Data(0))
    assert ts.begin_fit(keys, 3, data, quality) is None
    for k, v in zip(keys, ([1.5, 0.1 + 0.2], [float('nan'), 2.0])):
        ts.hist[0][k] += v
        ts.hist[1][k] += v[::-1]
    quality[0]['SSIM'] += [0.25, 0.5]
    quality[0]['PSNR'] += [float('inf'), 30.0]
    a.learning_rates += [2e-4, float(np.float32(1e-4))]
    data[0].epoch, data[1].epoch, ts.epoch = 2, 3, 2
    ts.pending = {'b1.train/g.mask_draws': np.array([6, 0], np.int32)}        # restored earlier, its step never came up: carried on
    manager = CheckpointManager(Checkpoint(train_state=ts), str(tmp_path / 'ck'), max_to_keep=2)
    prefix = manager.save()
    stored = {k: v for k, v in tfbundle.read_bundle(prefix)[0].items() if k.startswith('train_state/')}
    assert {v.dtype for v in stored.values()} == {np.dtype(t) for t in ('int64', 'uint8', 'float64', 'uint64', 'float32', 'int32', 'uint16')}
    assert stored['train_state/device/pool_y/storage'].dtype == np.uint16 and stored['train_state/device/pool_y/storage'].shape == (4, 2, 2, 1)
    assert stored['train_state/history/train'].shape == (2, 2) and stored['train_state/quality/averaged'].shape == (2, 0)
    assert T.check_resume(prefix, CONFIG) == prefix

    b = _model(5)
    for p in b.pools:
        p.state.zero_(), p.storage.zero_()
    b.ctx.ls.zero_()
    Checkpoint(train_state=b.train_state).restore(prefix)
    tb = b.train_state
    assert tb.restored and tb.epoch == 2 and tb.steps_per_epoch == 3 and tb.stored_config == T.run_config(CONFIG)
    assert torch.equal(b.ctx.ls, a.ctx.ls)
    for pa, pb in zip(a.pools, b.pools):
        assert torch.equal(pa.state, pb.state) and torch.equal(pa.storage.view(torch.int16), pb.storage.view(torch.int16))
    assert list(tb.pending) == ['b1.train/g.mask_draws']          # no such step object yet: held
    assert b._rng.bit_generator.state == a._rng.bit_generator.state
    quality_b, data_b = ({'SSIM': [], 'PSNR': []}, {'SSIM': [], 'PSNR': []}), (_Data(0), _Data(0), _Data(0))
    done, hist = tb.begin_fit(keys, 3, data_b, quality_b)
    assert done == 2 and not tb.restored
    for ha, hb in zip(ts.hist, hist):
        assert list(ha) == list(hb) and all(np.array_equal(ha[k], hb[k], equal_nan=True) for k in ha)
    assert hist[0]['Generator Total Loss'][1] == 0.1 + 0.2                            # float64: not a bit lost
    assert quality_b[0] == quality[0] and quality_b[1] == quality[1]
    assert b.learning_rates == a.learning_rates and [d.epoch for d in data_b] == [2, 3, 0]
    # the second bundle holds what the first did
    again = CheckpointManager(Checkpoint(train_state=tb), str(tmp_path / 'ck2'), max_to_keep=2).save()
    second = {k: v for k, v in tfbundle.read_bundle(again)[0].items() if k.startswith('train_state/')}
    assert set(second) == set(stored) and all(second[k].dtype == stored[k].dtype and second[k].tobytes() == stored[k].tobytes() for k in stored)
    # ... and the generators draw the same from here on
    assert [int(a._rng.integers(0, 31)) for _ in range(8)] == [int(b._rng.integers(0, 31)) for _ in range(8)]
    assert a._rng.random(4).tolist() == b._rng.random(4).tolist()


def test_fit_refuses_another_dataset(tmp_path):
    a = _model(1, pools=False, ls=False)
    a.train_state.begin_fit(['k'], 3, (_Data(1),), ({}, {}))
    prefix = Checkpoint(train_state=a.train_state).write(str(tmp_path / 'ckpt-1'))
    b = _model(1, pools=False, ls=False)
    Checkpoint(train_state=b.train_state).restore(prefix)
    with pytest.raises(T.ResumeRefused, match='steps_per_epoch'):
        b.train_state.begin_fit(['k'], 4, (_Data(0),), ({}, {}))


def test_old_checkpoints_restore_nothing(tmp_path):
    old = _bundle(tmp_path, with_state=False)
    m = _model(1)
    before = m._rng.bit_generator.state
    Checkpoint(train_state=m.train_state).restore(old)
    assert not m.train_state.restored and m._rng.bit_generator.state == before
    assert m.train_state.begin_fit(['k'], 3, (), ({}, {})) is None                  # fit() starts at epoch 1, as ever


def test_stored_state_of_another_shape_is_refused():
    with pytest.raises(ValueError, match='pool_y/storage'):
        T.numpy_into_device('pool_y/storage', np.zeros((2, 2), np.uint16), torch.zeros((4, 2), dtype=torch.bfloat16))
