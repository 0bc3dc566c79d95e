"""CPU tests of the dSSIM loss: the fp64 reference tests/dssim_ref.py against the SSIM reference of
section 12, against finite differences and against the closed gradient formula of include/gan_amd.h restated in numpy; the CLI
choice; the descriptor's refusals (found before any launch, so they need no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dssim_ref as R
from tests import quality_ref as Q


def _pair(shape, seed, noise=1.0):
    rng = np.random.default_rng(seed)
    n, h, w, c = shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    base = 0.6 * np.sin(0.3 * yy + 0.2 * xx)[None, :, :, None]
    a = np.clip(base + noise * 0.3 * rng.uniform(-1, 1, shape), -1, 1)
    b = np.clip(0.9 * base + noise * 0.3 * rng.uniform(-1, 1, shape), -1, 1)
    return a, b


def closed_formula(a, b):
    """dloss/da as include/gan_amd.h states it: P, Q, R per map position, the transposed window, the per-pixel factors."""
    ua, ub = Q.display(a), Q.display(b)
    n, h, w, c = ua.shape
    mx, my, sxy, sq = Q._filter(ua), Q._filter(ub), Q._filter(ua * ub), Q._filter(ua * ua + ub * ub)
    A1, B1 = 2 * mx * my + Q.C1, mx ** 2 + my ** 2 + Q.C1
    A2, B2 = 2 * (sxy - mx * my) + Q.C2, sq - mx ** 2 - my ** 2 + Q.C2
    S = A1 * A2 / (B1 * B2)
    P = (2 * my * A2 - 2 * my * A1) / (B1 * B2) - S * (2 * mx / B1 - 2 * mx / B2)
    Qm = 2 * A1 / (B1 * B2)
    Rm = -S / B2
    g = Q.window()
    mh, mw = h - 10, w - 10

    def GT(Z):
        out = np.zeros_like(ua)
        for ky in range(11):
            for kx in range(11):
                out[:, ky:ky + mh, kx:kx + mw] += g[ky] * g[kx] * Z
        return out
    return -0.5 / (n * c * mh * mw) * (GT(P) + ub * GT(Qm) + 2 * ua * GT(Rm))


@pytest.mark.parametrize('shape', [(1, 11, 11, 1), (2, 12, 13, 3), (3, 23, 17, 1)], ids=lambda s: 'x'.join(map(str, s)))
def test_reference_loss_is_one_minus_mean_ssim(shape):
    a, b = _pair(shape, 1)
    got = R.loss(a, b)
    want = 1.0 - Q.ssim(a, b).mean()
    print(f"dssim ref {shape}: loss {got:.15f} 1 - mean ssim {want:.15f}")
    assert abs(got - want) <= 1e-12
    assert abs(R.loss_and_grad(a, b)[0] - want) <= 1e-12


def test_reference_gradient_matches_central_differences():
    shape = (1, 12, 13, 3)
    a, b = _pair(shape, 2)
    _, grad = R.loss_and_grad(a, b)
    grad = grad.numpy()
    eps = 1e-6
    worst = 0.0
    for idx in np.ndindex(*shape):
        ap, am = a.copy(), a.copy()
        ap[idx] += eps
        am[idx] -= eps
        fd = (R.loss(ap, b) - R.loss(am, b)) / (2 * eps)
        worst = max(worst, abs(fd - grad[idx]))
    scale = np.abs(grad).max()
    print(f"dssim ref central differences: worst {worst:.3e} of max|grad| {scale:.3e}")
    # central differences: truncation eps^2 * f''' (~1e-12) plus cancellation 1e-16 / eps (~1e-10) on a loss of order 1
    assert worst <= 1e-8 * max(scale, 1.0) and scale > 1e-4


@pytest.mark.parametrize('shape', [(1, 12, 13, 3), (2, 11, 11, 1), (2, 21, 22, 3), (1, 43, 42, 1)], ids=lambda s: 'x'.join(map(str, s)))
def test_reference_gradient_matches_the_closed_formula(shape):
    a, b = _pair(shape, 3)
    _, grad = R.loss_and_grad(a, b)
    want = closed_formula(a, b)
    err = np.abs(grad.numpy() - want).max() / np.abs(want).max()
    print(f"dssim closed formula {shape}: rel err {err:.3e}")
    assert err <= 1e-11


def test_equal_images_have_zero_loss_and_gradient():
    a, _ = _pair((2, 17, 15, 3), 4)
    loss, grad = R.loss_and_grad(a, a.copy())
    _, other = R.loss_and_grad(*_pair((2, 17, 15, 3), 4))
    print(f"dssim a == b: loss {loss:.3e} max|grad| {float(grad.abs().max()):.3e} (a != b: {float(other.abs().max()):.3e})")
    assert abs(loss) < 1e-15
    assert float(grad.abs().max()) <= 1e-12 * float(other.abs().max())


def test_eager_restatement_matches_the_reference():
    """Pix2Pix.generator_loss's torch form (fp32) against the fp64 reference, value and gradient."""
    from gan_amd.pix2pix import _dssim_eager
    shape = (2, 33, 29, 3)
    a, b = _pair(shape, 5)
    at = torch.from_numpy(a).float().requires_grad_(True)
    got = _dssim_eager(at, torch.from_numpy(b).float())
    got.backward()
    want, grad = R.loss_and_grad(at.detach().double().numpy(), torch.from_numpy(b).float().double().numpy())
    assert abs(float(got.detach()) - want) <= 1e-5
    assert float((at.grad.double() - grad).abs().max()) <= 1e-3 * float(grad.abs().max())


def test_cli_accepts_dssim_and_still_refuses_ssim():
    from gan_amd import pix2pix
    base = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']
    assert pix2pix.parse_opt(base).generator_loss == 'l1'
    assert pix2pix.parse_opt(base + ['--generator-loss', 'dssim']).generator_loss == 'dssim'
    assert pix2pix.parse_opt(base + ['--generator-loss', 'l1']).generator_loss == 'l1'
    for bad in ('ssim', 'DSSIM', 'l2'):
        with pytest.raises(SystemExit):
            pix2pix.parse_opt(base + ['--generator-loss', bad])


def _good(L, grad=True):
    n, h, w, c = 3, 43, 26, 3
    ws = L.load().gan_dssim_workspace_bytes(n, h, w, c)
    da = L.GanTensor(1 << 24, n, h, w, c, 8) if grad else L.GanTensor()
    return L.GanDssimDesc(L.BF16, L.F32, L.GanTensor(4096, n, h, w, c, 8), L.GanTensor(1 << 20, n, h, w, c, c), 1.0, 0, 1 << 22, 100.0,
                          L.BF16, da, 1 << 23, ws, None)


def test_dssim_abi_refuses_bad_descriptors_before_any_launch():
    from gan_amd import _lib as L
    lib = L.load()
    call = lambda d: lib.gan_dssim(C.byref(d), None)
    assert lib.gan_dssim(None, None) == L.E_ARG
    assert L.GanDssimDesc().struct_size == C.sizeof(L.GanDssimDesc)
    # workspace: one float per (image, 32 x 32 tile of pixels); 0 for a refused shape
    wsb = lib.gan_dssim_workspace_bytes
    assert wsb(1, 11, 11, 1) == 4 and wsb(3, 42, 43, 3) == 3 * 2 * 2 * 4 and wsb(16, 256, 256, 1) == 16 * 64 * 4
    assert wsb(1, 4096, 4096, 3) == 128 * 128 * 4
    assert wsb(0, 64, 64, 1) == wsb(1, 10, 64, 1) == wsb(1, 64, 10, 1) == wsb(1, 64, 64, 2) == wsb(1, 4097, 64, 1) == 0

    def bad(code, sub=None, grad=True, **fields):
        d = _good(L, grad)
        for k, v in fields.items():
            setattr(getattr(d, sub) if sub else d, k, v)
        assert call(d) == code, (sub, fields)

    bad(L.E_ARG, struct_size=C.sizeof(L.GanDssimDesc) - 8)
    bad(L.E_ARG, struct_size=0)
    for ptr in ('loss_out', 'workspace'):
        bad(L.E_ARG, **{ptr: None})
    for t in ('a', 'b', 'da'):
        if t != 'da':
            bad(L.E_ARG, t, ptr=None)
        for c in (0, 2, 4, 8):
            bad(L.E_ARG, t, c=c)
        for f in ('n', 'h', 'w'):
            bad(L.E_ARG, t, **{f: 34})                  # differs from the other tensors
        bad(L.E_ARG, t, pitch=2)                        # pitch < c
        bad(L.E_ARG, t, c=1)                            # c = 1 against c = 3
    for dt in (-1, 3, 7):
        bad(L.E_ARG, dtype_a=dt)
        bad(L.E_ARG, dtype_b=dt)
        bad(L.E_ARG, dtype_da=dt)
    for acc in (-1, 2):
        bad(L.E_ARG, loss_accumulate=acc)
    for c in (2, 4):                                    # c of all tensors alike, but not 1 or 3
        d = _good(L)
        d.a.c = d.b.c = d.da.c = c
        assert call(d) == L.E_ARG
    d = _good(L)
    d.a.n = d.b.n = d.da.n = 0
    assert call(d) == L.E_ARG
    for grad in (True, False):
        for f in ('h', 'w'):
            for v in (10, 1, 4097):
                d = _good(L, grad)
                for t in (d.a, d.b, d.da):
                    setattr(t, f, v)
                d.workspace_bytes = 1 << 30
                assert call(d) == L.E_SHAPE, (grad, f, v)
        bad(L.E_WORKSPACE, grad=grad, workspace_bytes=_good(L).workspace_bytes - 4)
        bad(L.E_WORKSPACE, grad=grad, workspace_bytes=0)


def test_binding_matches_the_header():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    import gen_binding
    from gan_amd import _lib as L
    fields = gen_binding.parse_structs()['GanDssimDesc']
    want = [(f, getattr(C, t[2:]) if t.startswith('C.') else getattr(L, t)) for f, t in fields]
    assert list(L.GanDssimDesc._fields_) == want and fields[0] == ('struct_size', 'C.c_uint32')
    assert {'gan_dssim', 'gan_dssim_workspace_bytes'} <= set(L.SYMBOLS)


def test_step_refuses_an_unknown_generator_loss():
    from gan_amd.steps import Pix2PixStep
    with pytest.raises(ValueError):
        Pix2PixStep(None, 2, 256, 1, generator_loss='ssim')
