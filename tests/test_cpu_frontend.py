"""The command-line flags the Pix2Pix and CycleGAN drivers share (gan_amd.runner.add_common_flags / check_common_flags): both parsers
accept every one of them with the same default, and each parser keeps its own flags and refusals."""
import pytest

# flag -> default, written down from the two parsers as they stood before the flags were declared in one place
COMMON_DEFAULTS = {
    'img_size': 256, 'batch_size': 1, 'buffer_size': 99999, 'channels': '1', 'logging': 'true', 'seed': 123, 'save_weights': 'true',
    'epochs': 5, 'validation_size': 0.1, 'test_img': 5, 'learning_rate': 2e-4, 'beta_1': 0.5, 'beta_2': 0.999, 'weights': None,
    'dtype': 'bf16', 'gan_loss': 'bce', 'predict_training': 'true', 'data_cache': 'host', 'data_cache_gb': 64, 'ema_decay': 0.0,
    'ema_warmup': 'true', 'predict_weights': 'raw', 'lr_decay_epochs': 0, 'lr_end_factor': 0.0, 'device': 'cuda:0',
    'dist_backend': 'nccl', 'wire': 'bf16', 'exchange': 'allreduce',
}
# every common flag with a value other than its default, as a --predict command line accepts it (--epochs is not required there)
COMMON_GIVEN = {
    'img_size': 512, 'batch_size': 3, 'buffer_size': 7, 'channels': '3', 'logging': 'false', 'seed': 9, 'save_weights': 'false',
    'epochs': 2, 'validation_size': 0.2, 'test_img': 2, 'learning_rate': 1e-3, 'beta_1': 0.4, 'beta_2': 0.9, 'weights': 'w',
    'dtype': 'f16', 'gan_loss': 'lsgan', 'predict_training': 'false', 'data_cache': 'device', 'data_cache_gb': 1.5, 'ema_decay': 0.5,
    'ema_warmup': 'false', 'predict_weights': 'ema', 'device': 'cuda:1', 'dist_backend': 'gloo', 'wire': 'f32', 'exchange': 'rs_ag',
}
OWN = {'pix2pix': ['--data', 'd'], 'cyclegan': ['--input-images', 'x', '--target-images', 'y']}


def _parse(model, argv):
    from gan_amd import cycle_gan, pix2pix
    return {'pix2pix': pix2pix, 'cyclegan': cycle_gan}[model].parse_opt(OWN[model] + ['--output', 'o'] + argv)


@pytest.mark.parametrize("model", ['pix2pix', 'cyclegan'])
def test_common_flags_keep_their_defaults(model):
    """A --predict command line needs no --epochs, so the default of --epochs shows there; a --train one shows that of --weights."""
    o = vars(_parse(model, ['--predict', '--weights', 'w']))
    assert o['predict'] is True and o['train'] is False and o['weights'] == 'w' and o['output'] == 'o'
    for key, default in COMMON_DEFAULTS.items():
        if key != 'weights':
            assert key in o and o[key] == default and type(o[key]) is type(default), (key, o.get(key), default)
    t = vars(_parse(model, ['--train', '--epochs', '5']))
    assert t['weights'] is None and t['train'] is True and t['predict'] is False
    assert {k: t[k] for k in COMMON_DEFAULTS} == COMMON_DEFAULTS
    assert o['lambda'] == t['lambda'] == {'pix2pix': 100, 'cyclegan': 10}[model]          # (declared by both, with a default per model)


@pytest.mark.parametrize("model", ['pix2pix', 'cyclegan'])
def test_common_flags_are_accepted(model):
    argv = ['--predict']
    for key, v in COMMON_GIVEN.items():
        argv += ['--' + key.replace('_', '-'), str(v)]
    o = vars(_parse(model, argv))
    for key, v in COMMON_GIVEN.items():
        assert o[key] == v and type(o[key]) is type(v), (key, o[key], v)
    assert set(COMMON_GIVEN) | {'lr_decay_epochs', 'lr_end_factor'} == set(COMMON_DEFAULTS)
    t = vars(_parse(model, ['--train', '--epochs', '4', '--lr-decay-epochs', '3', '--lr-end-factor', '0.25']))
    assert (t['epochs'], t['lr_decay_epochs'], t['lr_end_factor']) == (4, 3, 0.25)


def test_both_parsers_declare_the_same_common_flags():
    p, c = (vars(_parse(m, ['--train', '--epochs', '1'])) for m in ('pix2pix', 'cyclegan'))
    shared = (set(p) & set(c)) - {'lambda'}
    assert shared == set(COMMON_DEFAULTS) | {'output', 'train', 'predict'}
    assert set(p) - set(c) == {'data', 'generator_loss', 'input_img_orient', 'predict_resolution', 'tile_overlap', 'quality_metrics'}
    assert set(c) - set(p) == {'input_images', 'target_images'}


@pytest.mark.parametrize("model", ['pix2pix', 'cyclegan'])
def test_common_refusals(model, capsys):
    train = ['--train', '--epochs', '1']
    for bad in ('1.0', '-0.1'):
        with pytest.raises(SystemExit):
            _parse(model, train + [f'--ema-decay={bad}'])
        assert f"--ema-decay {float(bad)} is outside [0, 1)" in capsys.readouterr().err
    for argv, message in ((['--img-size', '128'], "img-size currently only supported for 256 x 256 or 512 x 512 pixels!"),
                          (['--validation-size', '0.31'], "validation size is a proportion and bounded between 0-0.3!"),
                          (['--validation-size', '0'], "validation size is a proportion and bounded between 0-0.3!"),
                          (['--test-img', '0'], "test-img is an integer and must be >=1!")):
        with pytest.raises(AssertionError) as e:
            _parse(model, train + argv)
        assert str(e.value) == message
    for argv in (['--train'], ['--predict'], [], train + ['--predict', '--weights', 'w'], train + ['--dtype', 'f64'],
                 train + ['--gan-loss', 'hinge'], train + ['--lr-decay-epochs', '2'], ['--predict', '--weights', 'w', '--lr-end-factor', '0.5']):
        with pytest.raises(SystemExit):
            _parse(model, argv)
    with pytest.raises(SystemExit):       # --output is required
        from gan_amd import cycle_gan, pix2pix
        {'pix2pix': pix2pix, 'cyclegan': cycle_gan}[model].parse_opt(OWN[model] + train)


def test_each_parser_keeps_its_own_flags_and_refusals(capsys):
    from gan_amd import cycle_gan, pix2pix
    train = ['--train', '--epochs', '1']
    o = _parse('pix2pix', train)
    assert (o.generator_loss, o.input_img_orient, o.predict_resolution, o.tile_overlap, o.quality_metrics) == ('l1', 'left', 'resized', 64, 'false')
    assert _parse('pix2pix', train + ['--img-size', '512']).tile_overlap == 128
    with pytest.raises(SystemExit):
        _parse('pix2pix', train + ['--generator-loss', 'ssim'])
    assert "--generator-loss ssim is not supported by gan_amd" in capsys.readouterr().err
    assert _parse('pix2pix', train + ['--generator-loss', 'dssim']).generator_loss == 'dssim'
    predict = ['--predict', '--weights', 'w']
    for argv in (predict + ['--predict-resolution', 'native'], train + ['--predict-resolution', 'native', '--predict-training', 'false']):
        with pytest.raises(SystemExit):
            _parse('pix2pix', argv)
        assert "--predict-resolution native requires --predict and --predict-training false" in capsys.readouterr().err
    assert _parse('pix2pix', predict + ['--predict-resolution', 'native', '--predict-training', 'false']).predict_resolution == 'native'
    with pytest.raises(SystemExit):
        _parse('pix2pix', train + ['--tile-overlap', '129'])
    assert "--tile-overlap 129 is outside [0, img-size / 2 = 128]" in capsys.readouterr().err
    with pytest.raises(SystemExit):       # --data is required
        pix2pix.parse_opt(['--output', 'o'] + train)
    with pytest.raises(SystemExit):       # --target-images is required with --train ...
        cycle_gan.parse_opt(['--input-images', 'x', '--output', 'o'] + train)
    assert "--target-images" in capsys.readouterr().err
    assert cycle_gan.parse_opt(['--input-images', 'x', '--output', 'o'] + predict).target_images is None      # ... and only then
    with pytest.raises(SystemExit):       # --input-images always
        cycle_gan.parse_opt(['--target-images', 'y', '--output', 'o'] + train)
    for flag in ('--generator-loss', '--quality-metrics', '--predict-resolution'):                           # Pix2Pix's own
        with pytest.raises(SystemExit):
            _parse('cyclegan', train + [flag, 'l1'])
