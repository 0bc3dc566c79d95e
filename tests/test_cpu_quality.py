"""CPU side of the image-quality metrics: the fp64 reference tests/quality_ref.py pinned analytically and by
a second, independent implementation; the argument checks of gan_image_quality (nothing is launched without a GPU); the header,
the ctypes binding and the INTEGRATION.md snippet of GanQualityDesc; the CLI flag."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import quality_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _images(seed, n=2, h=23, w=31, c=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (n, h, w, c)), rng.uniform(-1, 1, (n, h, w, c))


def test_ssim_of_an_image_with_itself_is_exactly_one():
    a, _ = _images(0)
    assert np.array_equal(Q.ssim(a, a), np.ones(2))
    assert np.array_equal(Q.mae(a, a), np.zeros(2)) and np.all(np.isposinf(Q.psnr(a, a)))


def test_ssim_of_two_constant_images_is_the_luminance_term():
    for ra, rb in ((-0.7, 0.8), (1.0, -1.0), (0.25, 0.25), (-1.0, -1.0)):
        A, B = 0.5 * ra + 0.5, 0.5 * rb + 0.5
        got = Q.ssim(np.full((1, 14, 19, 1), ra), np.full((1, 14, 19, 1), rb))
        assert np.allclose(got, (2 * A * B + Q.C1) / (A * A + B * B + Q.C1), rtol=1e-12, atol=0), (ra, rb)
    assert abs(Q.ssim(np.full((1, 11, 11, 3), -0.7), np.full((1, 11, 11, 3), 0.8))[0] - 0.324405476) < 1e-9


def test_ssim_is_symmetric():
    a, b = _images(1)
    assert np.array_equal(Q.ssim(a, b), Q.ssim(b, a)) and np.array_equal(Q.quality(a, b)[:, 1:], Q.quality(b, a)[:, 1:])


def test_window_is_the_normalised_gaussian():
    g = Q.window()
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert np.allclose(g[4] / g[5], np.exp(-1 / 4.5), rtol=1e-14)


def test_reference_agrees_with_an_independent_depthwise_conv2d():
    """The same definition through torch.nn.functional.conv2d with the outer-product 11 x 11 window, one group per channel."""
    import torch.nn.functional as F
    k = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()
    for seed, (h, w, c) in enumerate([(23, 31, 3), (11, 11, 1), (40, 12, 1)]):
        a, b = _images(10 + seed, 2, h, w, c)
        ua, ub = (torch.from_numpy(0.5 * v + 0.5).permute(0, 3, 1, 2) for v in (a, b))
        win = (g[:, None] * g[None, :]).expand(c, 1, 11, 11).contiguous()
        filt = lambda t: F.conv2d(t, win, groups=c)
        mx, my = filt(ua), filt(ub)
        lum = (2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4)
        cs = (2 * filt(ua * ub) - 2 * mx * my + 9e-4) / (filt(ua * ua + ub * ub) - mx * mx - my * my + 9e-4)
        want = (lum * cs).mean(dim=(2, 3)).mean(dim=1).numpy()
        assert np.abs(Q.ssim(a, b) - want).max() < 1e-12, (h, w, c)


def test_psnr_and_mae_of_a_single_pixel_difference():
    h, w, c, d = 13, 17, 3, 0.375
    a = np.random.default_rng(3).uniform(-0.5, 0.5, (1, h, w, c))
    b = a.copy()
    b[0, 4, 9, 1] += d
    d = b[0, 4, 9, 1] - a[0, 4, 9, 1]
    q = Q.quality(a, b)[0]
    assert np.isclose(q[2], abs(d) / 2 / (h * w * c), rtol=1e-12) and np.isclose(q[3], (d / 2) ** 2 / (h * w * c), rtol=1e-12)
    assert np.isclose(q[1], -10 * np.log10((d / 2) ** 2 / (h * w * c)), rtol=1e-12) and q[0] < 1


def _good(L, n=2, h=40, w=33, c=3):
    """A descriptor that passes every check (device pointers are never read on the host)."""
    lib = L.load()
    ws = lib.gan_image_quality_workspace_bytes(n, h, w, c)
    return L.GanQualityDesc(L.BF16, L.F32, L.GanTensor(4096, n, h, w, c, 8), L.GanTensor(1 << 20, n, h, w, c, c), 1 << 22, 1 << 23, ws)


def test_quality_abi_refuses_bad_descriptors_before_any_launch():
    from gan_amd import _lib as L
    lib = L.load()
    call = lambda d: lib.gan_image_quality(C.byref(d), None)
    assert lib.gan_image_quality(None, None) == L.E_ARG
    assert L.GanQualityDesc().struct_size == C.sizeof(L.GanQualityDesc)
    # workspace: 16 bytes per (image, 32 x 32 tile of the (h-10) x (w-10) map); 0 for a refused shape
    wsb = lib.gan_image_quality_workspace_bytes
    assert wsb(1, 11, 11, 1) == 16 and wsb(3, 42, 43, 3) == 3 * 1 * 2 * 16 and wsb(16, 256, 256, 1) == 16 * 64 * 16
    assert wsb(1, 4096, 4096, 3) == 128 * 128 * 16
    assert wsb(0, 64, 64, 1) == wsb(1, 10, 64, 1) == wsb(1, 64, 10, 1) == wsb(1, 64, 64, 2) == wsb(1, 4097, 64, 1) == 0

    def bad(code, sub=None, **fields):
        d = _good(L)
        for k, v in fields.items():
            setattr(getattr(d, sub) if sub else d, k, v)
        assert call(d) == code, (sub, fields)

    bad(L.E_ARG, struct_size=C.sizeof(L.GanQualityDesc) - 8)
    bad(L.E_ARG, struct_size=0)
    for ptr in ('out', 'workspace'):
        bad(L.E_ARG, **{ptr: None})
    for t in ('a', 'b'):
        bad(L.E_ARG, t, ptr=None)
        for c in (0, 2, 4, 8):
            bad(L.E_ARG, t, c=c)                       # (also a mismatch with the other tensor)
        for f in ('n', 'h', 'w'):
            bad(L.E_ARG, t, **{f: 34})                  # differs from the other tensor
        bad(L.E_ARG, t, pitch=2)                        # pitch < c
        bad(L.E_ARG, t, c=1)                            # c = 1 against c = 3
    for dt in (-1, 3, 7):
        bad(L.E_ARG, dtype_a=dt)
        bad(L.E_ARG, dtype_b=dt)
    for c in (2, 4):                                    # c of both tensors alike, but not 1 or 3
        d = _good(L)
        d.a.c = d.b.c = c
        assert call(d) == L.E_ARG
    d = _good(L)
    d.a.n = d.b.n = 0
    assert call(d) == L.E_ARG
    for f in ('h', 'w'):
        for v in (10, 1, 4097):
            d = _good(L)
            setattr(d.a, f, v)
            setattr(d.b, f, v)
            d.workspace_bytes = 1 << 30
            assert call(d) == L.E_SHAPE, (f, v)
    d = _good(L)
    d.workspace_bytes -= 1
    assert call(d) == L.E_WORKSPACE
    bad(L.E_WORKSPACE, workspace_bytes=0)


def test_header_binding_and_integration_snippet_of_the_quality_descriptor_agree():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_binding
    from gan_amd import _lib as L
    fields = gen_binding.parse_structs()['GanQualityDesc']
    want = [(f, getattr(C, t[2:]) if t.startswith('C.') else getattr(L, t)) for f, t in fields]
    assert list(L.GanQualityDesc._fields_) == want and fields[0] == ('struct_size', 'C.c_uint32')
    assert {'gan_image_quality', 'gan_image_quality_workspace_bytes'} <= set(L.SYMBOLS)
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    first = re.search(r"```python\nimport ctypes as C\n(.*?)```", text, flags=re.S).group(1)
    code = re.search(r"```python\n(# --- generated from include/gan_amd.h by tools/gen_binding.py GanQualityDesc ---\n.*?)```", text, flags=re.S).group(1)
    gen = code[:code.index('# --- end of generated part')]
    assert gen.split('\n', 1)[1].strip() == gen_binding.ctypes_source(['GanQualityDesc']).strip()
    ns = {}
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        exec("import ctypes as C\n" + first + code, ns)          # loads the library, binds both symbols
    finally:
        os.chdir(cwd)
    assert C.sizeof(ns['GanQualityDesc']) == C.sizeof(L.GanQualityDesc) and callable(ns['image_quality'])
    d = ns['GanQualityDesc'](struct_size=C.sizeof(ns['GanQualityDesc']) - 4)
    assert ns['lib'].gan_image_quality(C.byref(d), None) == -1


def test_cli_flag_and_defaults():
    from gan_amd import pix2pix
    base = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']
    assert pix2pix.parse_opt(base).quality_metrics == 'false'
    assert pix2pix.parse_opt(base + ['--quality-metrics', 'true']).quality_metrics == 'true'
    assert pix2pix.parse_opt(['--data', 'd', '--output', 'o', '--predict', '--weights', 'w', '--quality-metrics', 'true']).quality_metrics == 'true'
    with pytest.raises(SystemExit):
        pix2pix.parse_opt(base + ['--quality-metrics', 'yes'])
    with pytest.raises(SystemExit):           # the degenerate SSIM loss stays refused
        pix2pix.parse_opt(base + ['--generator-loss', 'ssim'])


def test_summary_is_strict_json_and_meter_keeps_order():
    import json
    from gan_amd.quality import KEYS, QualityMeter, summary
    m = QualityMeter()
    m.add(torch.tensor([[1.0, float('inf'), 0.0, 0.0], [0.5, 20.0, 0.1, 0.01]]))
    m.add(torch.tensor([[0.25, 10.0, 0.2, 0.1]]))
    acc, n = m.sums()
    assert n == len(m) == 3 and acc.tolist()[0] == 1.75
    per = m.drain()
    assert tuple(per) == KEYS and per['SSIM'] == [1.0, 0.5, 0.25] and len(m) == 0
    text = json.dumps(summary(per), allow_nan=False)
    back = json.loads(text)
    assert back['per_image']['PSNR'] == [None, 20.0, 10.0] and back['mean']['PSNR'] is None
    assert abs(back['mean']['MAE'] - 0.1) < 1e-7
