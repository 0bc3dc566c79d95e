"""CPU side of inference mode (`model(x, training=False)`): the CLI flag, the C ABI of the fold, and the fp64 inference reference
of tests/test_gpu_inference.py checked against torch.nn.functional.batch_norm(training=False)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gan_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predict_training_flag():
    from gan_amd import cycle_gan, pix2pix
    p = ['--data', 'd', '--output', 'o', '--predict', '--weights', 'w']
    c = ['--input-images', 'x', '--output', 'o', '--predict', '--weights', 'w']
    for mod, base in ((pix2pix, p), (cycle_gan, c)):
        assert mod.parse_opt(base).predict_training == 'true'
        assert mod.parse_opt(base + ['--predict-training', 'false']).predict_training == 'false'
        assert mod.parse_opt(base + ['--predict-training', 'true']).predict_training == 'true'
        for bad in ('False', '0', 'no'):
            with pytest.raises(SystemExit):
                mod.parse_opt(base + ['--predict-training', bad])


def test_fold_abi_is_declared_and_bound():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_binding
    from gan_amd import _lib as L
    fields = gen_binding.parse_structs()['GanFoldEntry']
    assert [f for f, _ in fields] == ['master', 'gamma', 'beta', 'moving_mean', 'moving_var', 'bias', 'nk', 'A', 'B', 'transposed',
                                      'tile_start', 'tiles_k']
    assert [f for f, _ in L.GanFoldEntry._fields_] == [f for f, _ in fields]
    assert C.sizeof(L.GanFoldEntry) == 7 * 8 + 5 * 4 + 4          # (padded to 8 bytes: an array of entries on the device)
    lib = L.load()
    assert lib.gan_bn_fold_multi.argtypes[4] is C.c_float
    assert lib.gan_bn_fold_multi(None, 1, 1, L.BF16, 1e-3, None) == L.E_ARG       # argument checks happen before any launch
    assert lib.gan_bn_fold_multi(16, 1, 1, L.BF16, 0.0, None) == L.E_ARG


def test_chunked():
    from gan_amd.data import chunked
    assert list(chunked(range(7), 3)) == [[0, 1, 2], [3, 4, 5], [6]]
    assert list(chunked(range(6), 3)) == [[0, 1, 2], [3, 4, 5]] and list(chunked([], 3)) == []


def _torch_block(x, w, P, name, act, transposed):
    """Conv2D(k4, s2, 'same') | Conv2DTranspose(k4, s2, 'same') -> BatchNormalization(training=False) -> act, in torch fp64."""
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    if transposed:      # (kh, kw, cout, cin) -> (cin, cout, kh, kw); 'same' for k4 s2 = padding 1
        y = F.conv_transpose2d(xt, torch.from_numpy(w).permute(3, 2, 0, 1), stride=2, padding=1)
    else:               # HWIO -> OIHW; TF "same" for k4 s2 on an even input pads 1 on each side
        y = F.conv2d(F.pad(xt, (1, 1, 1, 1)), torch.from_numpy(w).permute(3, 2, 0, 1), stride=2)
    t = lambda k: torch.from_numpy(P[name + k])
    y = F.batch_norm(y, t('.moving_mean'), t('.moving_variance'), t('.gamma'), t('.beta'), training=False, eps=O.BN_EPS)
    y = F.leaky_relu(y, O.LEAKY_ALPHA) if act == 'lrelu' else F.relu(y)
    return y.permute(0, 2, 3, 1).numpy()


def test_inference_reference_blocks_match_torch_batch_norm():
    from tests.test_gpu_inference import bn_eval
    rng = np.random.default_rng(0)
    for name, cin, cout, hw, transposed, act in (('down1', 8, 16, 16, False, 'lrelu'), ('up3', 16, 8, 4, True, 'relu'),
                                                 ('down7', 12, 24, 2, False, 'lrelu')):
        x = rng.standard_normal((2, hw, hw, cin))
        w = 0.2 * rng.standard_normal((4, 4, cout, cin) if transposed else (4, 4, cin, cout))
        P = {name + '.gamma': rng.uniform(-1.5, 1.5, cout), name + '.beta': rng.normal(0, 0.3, cout),
             name + '.moving_mean': rng.normal(0, 0.5, cout), name + '.moving_variance': rng.uniform(0.05, 3.0, cout)}
        y = O.convT2d_fwd(x, w) if transposed else O.conv2d_fwd(x, w, 2)
        ours = O.act_fwd(bn_eval(y, P, name), act)
        ref = _torch_block(x, w, P, name, act, transposed)
        assert ours.shape == ref.shape and np.abs(ours - ref).max() < 1e-12, name
        # the fold the kernel computes: scaled kernel + bias equals conv -> BN (fp64, algebraically)
        s = P[name + '.gamma'] / np.sqrt(P[name + '.moving_variance'] + O.BN_EPS)
        bias = P[name + '.beta'] - P[name + '.moving_mean'] * s
        wf = w * (s[None, None, :, None] if transposed else s[None, None, None, :])
        yf = (O.convT2d_fwd(x, wf) if transposed else O.conv2d_fwd(x, wf, 2)) + bias
        assert np.abs(O.act_fwd(yf, act) - ours).max() < 1e-12, name


@pytest.mark.slow
def test_inference_reference_generator_is_batch_independent():
    """The fp64 inference reference itself: no batch coupling (unlike training mode, whose batch statistics couple the images)."""
    from tests.test_gpu_inference import generator_eval_ref
    P = O.init_generator(1, seed=4)
    rng = np.random.default_rng(1)
    for k in [k for k in P if k.endswith('.gamma')]:
        c = P[k].shape
        P[k.replace('.gamma', '.moving_mean')] = np.zeros(c, np.float32)
        P[k.replace('.gamma', '.moving_variance')] = rng.uniform(0.001, 0.01, c).astype(np.float32)
    x = O.synthetic_pair(2, 256, 1, seed=5)[0]
    y, _ = generator_eval_ref(P, x)
    y1, _ = generator_eval_ref(P, x[1:])
    assert np.abs(y[1] - y1[0]).max() < 1e-12 and np.abs(y[0] - y[1]).max() > 1e-3
