"""CPU tests of the MS-SSIM loss: the fp64 reference tests/msssim_ref.py pinned against tests/dssim_ref.py,
tests/quality_ref.py, central differences and its exact corner cases; the shape rule; header, binding and the descriptor's refusals
(found before any launch, so they need no GPU); the eager restatement; the command line and the --resume gate."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import dssim_ref as D
from tests import msssim_ref as R
from tests import quality_ref as Q


def _pair(shape, seed, amp=0.2):
    n, h, w, c = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    ph = rng.uniform(0, 6.28, (n, 1, 1, c))
    b = 0.7 * np.sin(0.21 * yy[None, :, :, None] + ph) * np.cos(0.13 * xx[None, :, :, None] - ph) + 0.05 * rng.uniform(-1, 1, shape)
    return np.clip(b + amp * rng.uniform(-1, 1, shape), -1, 1), b


def _hand_pool(x):
    """NHWC numpy, pixel by pixel from the definition."""
    n, h, w, c = x.shape
    out = np.zeros((n, (h + 1) // 2, (w + 1) // 2, c))
    for i in range(out.shape[1]):
        for k in range(out.shape[2]):
            i1, k1 = min(2 * i + 1, h - 1), min(2 * k + 1, w - 1)
            out[:, i, k] = 0.25 * ((x[:, 2 * i, 2 * k] + x[:, 2 * i, k1]) + (x[:, i1, 2 * k] + x[:, i1, k1]))
    return out


def test_one_scale_with_weight_one_is_dssim():
    a, b = _pair((2, 33, 29, 3), 1)
    loss, grad, _ = R.loss_and_grad(a, b, 1, (1.0,))
    want, gwant = D.loss_and_grad(a, b)
    assert abs(loss - want) <= 1e-12
    assert float((grad - gwant).abs().max()) <= 1e-12 * float(gwant.abs().max())


def test_level_means_equal_quality_ref_on_hand_pooled_images():
    a, b = _pair((2, 45, 47, 1), 2)
    fs = R.factors(R._nchw(a, torch.float64), R._nchw(b, torch.float64), 3)
    assert [tuple(f.shape) for f in fs] == [(2, 1)] * 3
    a1, b1 = _hand_pool(a), _hand_pool(b)
    a2, b2 = _hand_pool(a1), _hand_pool(b1)
    assert a1.shape == (2, 23, 24, 1) and a2.shape == (2, 12, 12, 1)
    # S of the last level is quality_ref's SSIM of the twice pooled images; S of every level (level_terms) likewise
    assert np.abs(fs[2][:, 0].numpy() - Q.ssim(a2, b2)).max() <= 1e-12
    for x, y in ((a, b), (a1, b1), (a2, b2)):
        s = R.level_terms(R._nchw(x, torch.float64), R._nchw(y, torch.float64))[1][:, 0].numpy()
        assert np.abs(s - Q.ssim(x, y)).max() <= 1e-12
    # and the score is the product the definition names
    cs0 = R.level_terms(R._nchw(a, torch.float64), R._nchw(b, torch.float64))[0][:, 0].numpy()
    cs1 = R.level_terms(R._nchw(a1, torch.float64), R._nchw(b1, torch.float64))[0][:, 0].numpy()
    want = cs0 ** R.POWER[0] * cs1 ** R.POWER[1] * Q.ssim(a2, b2) ** R.POWER[2]
    got = R.scores(R._nchw(a, torch.float64), R._nchw(b, torch.float64), 3).numpy()
    assert np.abs(got - want).max() <= 1e-12
    assert abs(R.loss(a, b, 3) - (1.0 - want.mean())) <= 1e-12


def test_gradient_against_central_differences():
    shape = (1, 23, 25, 3)
    a, b = _pair(shape, 3)
    _, grad, _ = R.loss_and_grad(a, b, 2)
    grad = grad.numpy()
    rng = np.random.default_rng(0)
    eps, worst = 1e-6, 0.0
    spots = [(0, 0, 0), (22, 24, 2), (22, 0, 1), (0, 24, 0), (11, 12, 1), (21, 23, 2)] + \
            [(int(rng.integers(23)), int(rng.integers(25)), int(rng.integers(3))) for _ in range(10)]
    for y, x, ch in spots:
        hi, lo = a.copy(), a.copy()
        hi[0, y, x, ch] += eps
        lo[0, y, x, ch] -= eps
        fd = (R.loss(hi, b, 2) - R.loss(lo, b, 2)) / (2 * eps)
        worst = max(worst, abs(fd - grad[0, y, x, ch]))
    assert worst <= 1e-5 * float(np.abs(grad).max()), (worst, float(np.abs(grad).max()))


def test_equal_images_have_zero_loss_and_opposite_images_score_zero():
    a, _ = _pair((2, 45, 47, 3), 4)
    loss, grad, sc = R.loss_and_grad(a, a.copy(), 3)
    assert abs(loss) < 1e-15 and np.abs(sc - 1.0).max() < 1e-15
    other = R.loss_and_grad(*_pair((2, 45, 47, 3), 4), 3)[1]
    assert float(grad.abs().max()) <= 1e-12 * float(other.abs().max())
    # a = -b on a smooth pattern: the covariance is minus the variance, every CS_j is negative and clamped
    _, b = _pair((2, 45, 47, 3), 5, amp=0.0)
    loss, grad, sc = R.loss_and_grad(-b, b, 3)
    assert R.min_factor(-b, b, 3) < 0.0
    assert loss == 1.0 and np.all(sc == 0.0) and float(grad.abs().max()) == 0.0


def test_shape_rule():
    assert R.shape_ok(176, 176, 5) and R.shape_ok(176, 4096, 5) and not R.shape_ok(175, 176, 5) and not R.shape_ok(176, 175, 5)
    assert R.shape_ok(11, 11, 1) and not R.shape_ok(10, 11, 1) and R.shape_ok(22, 23, 2) and not R.shape_ok(21, 23, 2)
    assert not R.shape_ok(256, 256, 0) and not R.shape_ok(256, 256, 6) and not R.shape_ok(4097, 256, 1)
    from gan_amd import _lib as L
    wsb = L.load().gan_msssim_workspace_bytes
    for h, w, m in [(176, 176, 5), (175, 176, 5), (176, 175, 5), (11, 11, 1), (10, 11, 1), (22, 23, 2), (21, 23, 2), (87, 91, 4), (88, 91, 4),
                    (256, 256, 0), (256, 256, 6), (4097, 256, 1), (4096, 4096, 5)]:
        assert (wsb(2, h, w, 3, m) > 0) == R.shape_ok(h, w, m), (h, w, m)
    assert wsb(0, 64, 64, 1, 1) == wsb(1, 64, 64, 2, 1) == 0
    # M = 1: two floats per (image, channel, tile) and one coefficient per (image, channel)
    assert wsb(3, 42, 43, 3, 1) == (3 * 3 * 4 * 2 + 3 * 3) * 4
    # M = 2 at 22 x 23: three pooled planes of 11 x 12, partials of both levels, two coefficients
    assert wsb(1, 22, 23, 1, 2) == (3 * 11 * 12 + 2 * 2 + 2) * 4


def test_eager_restatement_matches_the_reference():
    """Pix2Pix.generator_loss's torch form (fp32) against the fp64 reference, value and gradient, odd sides on two levels."""
    from gan_amd.pix2pix import _msssim_eager
    a, b = _pair((2, 45, 47, 3), 6)
    at = torch.from_numpy(a).float().requires_grad_(True)
    got = _msssim_eager(at, torch.from_numpy(b).float(), R.POWER[:3])
    got.backward()
    want, grad, _ = R.loss_and_grad(at.detach().double().numpy(), torch.from_numpy(b).float().double().numpy(), 3)
    assert abs(float(got.detach()) - want) <= 1e-5
    assert float((at.grad.double() - grad).abs().max()) <= 1e-3 * float(grad.abs().max())


# ---- header, binding, refusals ----------------------------------------------------------------------------------------------------
def _good(L, grad=True, scales=3):
    n, h, w, c = 3, 45, 47, 3
    ws = L.load().gan_msssim_workspace_bytes(n, h, w, c, scales)
    da = L.GanTensor(1 << 24, n, h, w, c, 8) if grad else L.GanTensor()
    return L.GanMsssimDesc(L.BF16, L.F32, L.GanTensor(4096, n, h, w, c, 8), L.GanTensor(1 << 20, n, h, w, c, c), 1.0, 0, 1 << 22, 100.0,
                           L.BF16, da, 1 << 23, ws, None, scales, L.msssim_power(scales), None, 0)


def test_binding_matches_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    import gen_binding
    from gan_amd import _lib as L
    fields = gen_binding.parse_structs()['GanMsssimDesc']
    want = [(f, getattr(C, t[2:]) if t.startswith('C.') else getattr(L, t)) for f, t in fields]
    assert list(L.GanMsssimDesc._fields_) == want and fields[0] == ('struct_size', 'C.c_uint32')
    assert ('power', 'Float5') in fields and L.Float5 is C.c_float * 5
    assert {'gan_msssim', 'gan_msssim_workspace_bytes'} <= set(L.SYMBOLS)
    # the size the library was compiled with: a descriptor of this size gets past the struct_size check (to the last check of all)
    d = _good(L)
    d.workspace_bytes = 0
    assert d.struct_size == C.sizeof(L.GanMsssimDesc) and L.load().gan_msssim(C.byref(d), None) == L.E_WORKSPACE
    # layout by hand from the header: 3 x 4, GanTensor (8 + 5 x 4 -> 32) x 2, 4 + 4, 8, 4 + 4, 32, 8, 8, 8, 4 + 20, 8, 4 (+ 4 pad)
    assert C.sizeof(L.GanTensor) == 32 and C.sizeof(L.GanMsssimDesc) == 16 + 64 + 8 + 8 + 8 + 32 + 24 + 24 + 8 + 8
    assert tuple(L.msssim_power(5)) == tuple(np.float32(R.POWER)) and tuple(L.msssim_power(2, (0.5, 0.25)))[:2] == (0.5, 0.25)
    with pytest.raises(ValueError):
        L.msssim_power(3, (1.0,))


def test_msssim_abi_refuses_bad_descriptors_before_any_launch():
    from gan_amd import _lib as L
    lib = L.load()
    call = lambda d: lib.gan_msssim(C.byref(d), None)
    assert lib.gan_msssim(None, None) == L.E_ARG

    def bad(code, sub=None, grad=True, **fields):
        d = _good(L, grad)
        for k, v in fields.items():
            setattr(getattr(d, sub) if sub else d, k, v)
        assert call(d) == code, (sub, fields)

    bad(L.E_ARG, struct_size=C.sizeof(L.GanMsssimDesc) - 8)
    bad(L.E_ARG, struct_size=C.sizeof(L.GanDssimDesc))
    for ptr in ('loss_out', 'workspace'):
        bad(L.E_ARG, **{ptr: None})
    for t in ('a', 'b', 'da'):
        if t != 'da':
            bad(L.E_ARG, t, ptr=None)
        for c in (0, 2, 4, 8):
            bad(L.E_ARG, t, c=c)
        for f in ('n', 'h', 'w'):
            bad(L.E_ARG, t, **{f: 50})
        bad(L.E_ARG, t, pitch=2)
    for dt in (-1, 3):
        bad(L.E_ARG, dtype_a=dt)
        bad(L.E_ARG, dtype_b=dt)
        bad(L.E_ARG, dtype_da=dt)
    for acc in (-1, 2):
        bad(L.E_ARG, loss_accumulate=acc)
        bad(L.E_ARG, grad_accumulate=acc)
    for m in (0, -1, 6):
        bad(L.E_ARG, scales=m)
    for p in (-0.1, float('nan'), float('inf')):
        d = _good(L)
        d.power[1] = p
        assert call(d) == L.E_ARG, p
    d = _good(L)
    d.power[4] = float('nan')                           # beyond `scales`: not looked at
    d.workspace_bytes = 0
    assert call(d) == L.E_WORKSPACE
    for grad in (True, False):
        for f in ('h', 'w'):
            for v in (43, 10, 4097):                    # 43 < 11 * 4
                d = _good(L, grad)
                for t in (d.a, d.b, d.da):
                    setattr(t, f, v)
                d.workspace_bytes = 1 << 30
                assert call(d) == L.E_SHAPE, (grad, f, v)
        bad(L.E_WORKSPACE, grad=grad, workspace_bytes=_good(L).workspace_bytes - 4)
        bad(L.E_WORKSPACE, grad=grad, workspace_bytes=0)
    d = _good(L, scales=5)                              # 45 x 47 holds three scales, not five
    d.workspace_bytes = 1 << 30
    assert call(d) == L.E_SHAPE


def test_step_refuses_unknown_losses_and_weights():
    from gan_amd.steps import Pix2PixStep
    for kw in (dict(generator_loss='ms-ssim'), dict(generator_loss='msssim-l1'), dict(generator_loss='msssim_l1', msssim_alpha=0.0),
               dict(generator_loss='msssim_l1', msssim_alpha=1.5), dict(generator_loss='msssim_l1', msssim_alpha=float('nan'))):
        with pytest.raises(ValueError):
            Pix2PixStep(None, 2, 256, 1, **kw)


# ---- CLI and the resume gate --------------------------------------------------------------------------------------------------------
BASE = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']


def test_flags(capsys):
    from gan_amd import cycle_gan, pix2pix
    from gan_amd.runner import config_of
    o = pix2pix.parse_opt(BASE)
    assert o.generator_loss == 'l1' and o.msssim_alpha == 0.84 and 'msssim_alpha' not in vars(o) and config_of(o)['msssim_alpha'] == 0.84
    o = pix2pix.parse_opt(BASE + ['--generator-loss', 'msssim'])
    assert o.generator_loss == 'msssim' and config_of(o)['generator_loss'] == 'msssim' and o.msssim_alpha == 0.84
    o = pix2pix.parse_opt(BASE + ['--generator-loss', 'msssim-l1'])
    assert o.generator_loss == 'msssim-l1' and o.msssim_alpha == 0.84
    o = pix2pix.parse_opt(BASE + ['--generator-loss', 'msssim-l1', '--msssim-alpha', '0.5', '--edge-weight', '0.25'])
    assert config_of(o)['msssim_alpha'] == 0.5 and config_of(o)['edge_weight'] == 0.25
    assert pix2pix.parse_opt(BASE + ['--generator-loss', 'msssim-l1', '--msssim-alpha', '1']).msssim_alpha == 1.0
    for bad in ('0', '-0.5', '1.01', 'nan', 'inf'):
        with pytest.raises(SystemExit):
            pix2pix.parse_opt(BASE + ['--generator-loss', 'msssim-l1', '--msssim-alpha', bad])
        assert '--msssim-alpha' in capsys.readouterr().err
    for other in ('l1', 'dssim', 'msssim'):             # the weight belongs to the mix alone
        with pytest.raises(SystemExit):
            pix2pix.parse_opt(BASE + ['--generator-loss', other, '--msssim-alpha', '0.84'])
        assert '--msssim-alpha belongs to --generator-loss msssim-l1' in capsys.readouterr().err
    for bad in ('ssim', 'MSSSIM', 'msssim_l1', 'ms-ssim'):
        with pytest.raises(SystemExit):
            pix2pix.parse_opt(BASE + ['--generator-loss', bad])
        capsys.readouterr()
    with pytest.raises(SystemExit):
        pix2pix.parse_opt(BASE + ['--help'])
    assert re.search(r'--msssim-alpha.*msssim-l1', capsys.readouterr().out, flags=re.S)
    with pytest.raises(SystemExit):
        cycle_gan.parse_opt(['--input-images', 'x', '--target-images', 'y', '--output', 'o', '--train', '--epochs', '1', '--msssim-alpha', '0.5'])
    assert 'unrecognized arguments: --msssim-alpha' in capsys.readouterr().err


def test_resume_gate_knows_the_loss_and_its_weight(tmp_path):
    from gan_amd import tfbundle
    from gan_amd import train_state as T
    from tests.test_cpu_resume import CONFIG, _bundle
    assert T.run_config(CONFIG)['msssim_alpha'] == 0.84 and 'generator_loss' in T.run_config(CONFIG)
    mix = {**CONFIG, 'generator_loss': 'msssim-l1', 'msssim_alpha': 0.5}
    prefix = _bundle(tmp_path / 'm', mix)
    assert T.check_resume(prefix, mix) == prefix and T.check_resume(prefix, {**mix, 'msssim_alpha': '0.5'}) == prefix
    with pytest.raises(T.ResumeRefused) as e:
        T.check_resume(prefix, {**mix, 'msssim_alpha': 0.84})
    assert ' msssim_alpha ' in str(e.value)
    with pytest.raises(T.ResumeRefused) as e:
        T.check_resume(prefix, {**mix, 'generator_loss': 'msssim'})
    assert ' generator_loss ' in str(e.value)
    # a checkpoint written before the key existed resumes as before
    stored = T.run_config(CONFIG)
    del stored['msssim_alpha']
    os.makedirs(tmp_path / 'old')
    old = tfbundle.write_bundle(os.path.join(str(tmp_path / 'old'), 'ckpt-1'),
                                {'generator/layer_with_weights-15/bias/.ATTRIBUTES/VARIABLE_VALUE': np.zeros(1, np.float32),
                                 'train_state/epoch': np.array(2, np.int64), 'train_state/config': T._json_array(stored)})
    assert T.check_resume(old, CONFIG) == old
