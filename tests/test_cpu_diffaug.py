"""Differentiable augmentation, the parts that need no GPU: the float64 reference is pinned (autograd
against the closed transpose, the adjoint identity, the identity of neutral parameters, the laws of the draws), the header, the
binding and the INTEGRATION.md snippet agree, bad descriptors are refused before any launch, and the --diffaugment flag."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from tests import diffaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(h, w, rng, n):
    """n records with every policy on, drawn by the reference itself."""
    return R.draw(int(rng.integers(1 << 40)), int(rng.integers(100)), 48, n, h, w, R.POLICIES)


@pytest.mark.parametrize('h,w,group_c,c', [(16, 24, 3, 6), (17, 33, 1, 2), (8, 8, 3, 3), (9, 7, 1, 1)])
def test_autograd_backward_is_the_closed_transpose(h, w, group_c, c):
    rng = np.random.default_rng(h * w + c)
    params = _params(h, w, rng, 5)
    dy = rng.standard_normal((3, h, w, c))
    for sample0 in (0, 2):
        a, b = R.autograd_transpose(dy, params, group_c, sample0), R.transpose(dy, params, group_c, sample0)
        assert np.abs(a - b).max() <= 1e-12


@pytest.mark.parametrize('h,w,group_c,c', [(16, 24, 3, 6), (17, 33, 1, 2), (8, 8, 3, 3)])
def test_adjoint_identity(h, w, group_c, c):
    """<T x, y> = <x, T' y> for the linear part of T (brightness is an offset: T x - T 0 is linear)."""
    rng = np.random.default_rng(7 * h + w)
    params = _params(h, w, rng, 3)
    x, y = rng.standard_normal((3, h, w, c)), rng.standard_normal((3, h, w, c))
    lin = (R.forward(torch.from_numpy(x), params, group_c) - R.forward(torch.zeros(3, h, w, c, dtype=torch.float64), params, group_c)).numpy()
    lhs, rhs = (lin * y).sum(), (x * R.transpose(y, params, group_c)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_neutral_parameters_are_the_identity():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 9, 11, 6))
    params = [dict(R.NEUTRAL)] * 2
    for g in (1, 3):
        assert np.abs(R.forward(torch.from_numpy(x), params, g).numpy() - x).max() <= 1e-15      # (group 3: (x - m) + m in float64)
        assert np.abs(R.transpose(x, params, g) - x).max() <= 1e-15
    assert R.draw(1, 0, 48, 4, 16, 16, ()) == [R.NEUTRAL] * 4


def test_forward_order_is_colour_translation_cutout():
    """One hand-made record: brightness reaches only pixels that hold image content, the cut is in OUTPUT coordinates."""
    p = dict(R.NEUTRAL, tx=1, ty=-2, cut_x0=0, cut_y0=0, cut_w=2, cut_h=1, brightness=0.25)
    x = np.arange(4 * 5, dtype=np.float64).reshape(1, 4, 5, 1)
    y = R.forward(torch.from_numpy(x), [p], 1).numpy()[0, :, :, 0]
    want = np.zeros((4, 5))
    want[0:2, 1:5] = x[0, 2:4, 0:4, 0] + 0.25           # y(p) = x(p - t): rows move up by 2, columns right by 1
    want[0, 0:2] = 0                                    # the cut
    assert (y == want).all()


def _many(policy, size, launches=79):
    """>= 10,000 records of one policy: 79 launches of 128."""
    return [p for k in range(launches) for p in R.draw(123, k, 48, 128, size, size, (policy,))]


def _near(mean, want, sd, n):
    assert abs(mean - want) <= 4 * sd / np.sqrt(n), (mean, want)


def test_draws_lie_in_their_ranges_and_follow_the_uniform_law():
    size = 16
    T = (size + 4) // 8
    ps = _many('translation', size)
    n = len(ps)
    assert n >= 10000
    tx, ty = np.array([p['tx'] for p in ps]), np.array([p['ty'] for p in ps])
    assert set(tx) == set(ty) == set(range(-T, T + 1))                 # every value occurs
    sd = np.sqrt(((2 * T + 1) ** 2 - 1) / 12)
    _near(tx.mean(), 0, sd, n), _near(ty.mean(), 0, sd, n)
    assert all(p['cut_w'] == 0 and p['brightness'] == 0 and p['saturation'] == 1 for p in ps)
    ps = _many('brightness', size)
    b = np.array([p['brightness'] for p in ps])
    assert (b >= -0.5).all() and (b < 0.5).all() and (b == b.astype(np.float32)).all()
    _near(b.mean(), 0, np.sqrt(1 / 12), n)
    ps = _many('saturation', size)
    s = np.array([p['saturation'] for p in ps])
    assert (s >= 0).all() and (s < 2).all() and (s == s.astype(np.float32)).all()
    _near(s.mean(), 1, np.sqrt(4 / 12), n)
    assert all(p['tx'] == 0 and p['ty'] == 0 and p['cut_w'] == 0 for p in ps)


@pytest.mark.parametrize('size', [16, 18, 9])
def test_cutout_rectangles(size):
    """cs = size / 2; the centre offset is uniform on 0 .. size - cs % 2; the rectangle is clipped, never empty, never outside."""
    ps = _many('cutout', size)
    cs = size // 2
    N = size + (1 - cs % 2)
    starts = set()
    for p in ps:
        assert 0 < p['cut_w'] <= cs and 0 < p['cut_h'] <= cs
        assert 0 <= p['cut_x0'] and p['cut_x0'] + p['cut_w'] <= size and 0 <= p['cut_y0'] and p['cut_y0'] + p['cut_h'] <= size
        assert p['cut_w'] == cs or p['cut_x0'] == 0 or p['cut_x0'] + p['cut_w'] == size       # smaller only where an edge clips it
        starts.add(p['cut_x0'] if p['cut_w'] == cs else (-1 if p['cut_x0'] == 0 else size))
    assert set(range(0, size - cs + 1)) <= starts                                          # every unclipped position occurs
    # the offset itself: recompute it from the hash and compare its mean with the uniform law on 0 .. N-1
    offs = []
    for k in range(79):
        key = R.mix64((123 ^ (k << 32) ^ 48) & R.M64)
        offs += [((R.mix64(key ^ (4 * i + 1)) & 0xffffffff) * N) >> 32 for i in range(128)]
    offs = np.array(offs)
    assert offs.min() == 0 and offs.max() == N - 1
    _near(offs.mean(), (N - 1) / 2, np.sqrt((N * N - 1) / 12), len(offs))


def test_draws_depend_on_launch_stream_and_seed():
    a = R.draw(123, 0, 48, 8, 256, 256, R.POLICIES)
    assert a != R.draw(123, 1, 48, 8, 256, 256, R.POLICIES) and a != R.draw(123, 0, 49, 8, 256, 256, R.POLICIES)
    assert a != R.draw(124, 0, 48, 8, 256, 256, R.POLICIES) and a == R.draw(123, 0, 48, 8, 256, 256, R.POLICIES)
    assert (R.table(a)[:, :6] == [[p[k] for k in ('tx', 'ty', 'cut_x0', 'cut_y0', 'cut_w', 'cut_h')] for p in a]).all()
    assert R.records(R.table(a)) == a                                   # (the floats are exact in fp32)


def test_ulp_helper():
    assert R.ulp(1.0, 'bf16') == 2.0 ** -7 and R.ulp(1.9, 'f16') == 2.0 ** -10 and R.ulp(2.0, 'f32') == 2.0 ** -22
    assert R.ulp(0.0, 'f16') == 2.0 ** -24 and R.ulp(0.0, 'bf16') == 2.0 ** -133


# ---- header, binding, snippet -----------------------------------------------------------------------------------------------------
def test_header_binding_and_integration_snippet_agree():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_binding
    structs = gen_binding.parse_structs()
    for name in ('GanDiffAugParams', 'GanDiffAugDesc'):
        want = [(f, getattr(C, t[2:]) if t.startswith('C.') else getattr(L, t)) for f, t in structs[name]]
        assert list(getattr(L, name)._fields_) == want
    assert C.sizeof(L.GanDiffAugParams) == 32 and structs['GanDiffAugDesc'][0] == ('struct_size', 'C.c_uint32')
    hdr = open(os.path.join(ROOT, 'include', 'gan_amd.h')).read()
    for proto in (r'int gan_diffaug_policy\(const char\* names, uint32_t\* policy\);',
                  r'int gan_diffaug_draw\(GanDiffAugParams\* params, int32_t n, int32_t h, int32_t w, uint32_t policy, uint64_t seed,\s+'
                  r'uint32_t stream_id, int32_t\* launches, gan_stream_t stream\);',
                  r'int gan_diffaug_apply\(const GanDiffAugDesc\* d, gan_stream_t stream\);'):
        assert re.search(proto, hdr), proto
    assert {'gan_diffaug_policy', 'gan_diffaug_draw', 'gan_diffaug_apply'} <= set(L.SYMBOLS)
    lib = L.load()
    assert all(hasattr(lib, s) for s in ('gan_diffaug_policy', 'gan_diffaug_draw', 'gan_diffaug_apply'))
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    first = re.search(r"```python\nimport ctypes as C\n(.*?)```", text, flags=re.S).group(1)
    code = re.search(r"```python\n(# --- generated from include/gan_amd.h by tools/gen_binding.py GanDiffAugParams GanDiffAugDesc ---\n.*?)```",
                     text, flags=re.S).group(1)
    gen = code[:code.index('# --- end of generated part')]
    assert gen.split('\n', 1)[1].strip() == gen_binding.ctypes_source(['GanDiffAugParams', 'GanDiffAugDesc']).strip()
    ns = {}
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        exec("import ctypes as C\n" + first + code, ns)
    finally:
        os.chdir(cwd)
    assert C.sizeof(ns['GanDiffAugDesc']) == C.sizeof(L.GanDiffAugDesc) and callable(ns['diffaug_forward'])
    d = ns['GanDiffAugDesc'](struct_size=C.sizeof(ns['GanDiffAugDesc']) - 8)
    assert ns['lib'].gan_diffaug_apply(C.byref(d), None) == -1


def test_policy_names():
    lib = L.load()
    m = C.c_uint32(99)
    assert lib.gan_diffaug_policy(b"", C.byref(m)) == 0 and m.value == 0
    assert lib.gan_diffaug_policy(b"translation,cutout", C.byref(m)) == 0 and m.value == 3
    assert lib.gan_diffaug_policy(b"saturation,brightness,cutout,translation", C.byref(m)) == 0 and m.value == 15
    for bad in (b"contrast", b"cutout,", b",cutout", b"Cutout", b"cut"):
        m.value = 99
        assert lib.gan_diffaug_policy(bad, C.byref(m)) == L.E_ARG and m.value == 99, bad
    assert lib.gan_diffaug_policy(None, C.byref(m)) == L.E_ARG and lib.gan_diffaug_policy(b"cutout", None) == L.E_ARG
    from gan_amd import diffaug
    assert diffaug.policy_mask('cutout,translation') == 3 and diffaug.policy_mask('') == 0
    assert diffaug.parse_policies('saturation, cutout') == ('cutout', 'saturation')
    with pytest.raises(ValueError):
        diffaug.parse_policies('contrast')


def test_every_bad_argument_is_refused_before_any_launch():
    """No device memory is behind these pointers and no GPU need be present: the error code comes back before anything is enqueued."""
    lib = L.load()
    A = 4096

    def call(src=None, dst=None, **fields):
        view = lambda **kw: L.GanTensor(**{**dict(ptr=A, n=2, h=8, w=8, c=3, pitch=8), **kw})
        d = L.GanDiffAugDesc(L.BF16, view(**(src or {})), view(**(dst or {})), 3, 0, A, 0)
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.gan_diffaug_apply(C.byref(d), None)

    assert lib.gan_diffaug_apply(None, None) == L.E_ARG
    for size in (0, C.sizeof(L.GanDiffAugDesc) - 8, C.sizeof(L.GanDiffAugDesc) + 8):
        assert call(struct_size=size) == L.E_ARG
    assert call(dtype=3) == L.E_ARG and call(dtype=-1) == L.E_ARG
    assert call(params=None) == L.E_ARG and call(params=A + 2) == L.E_ARG
    assert call(src=dict(ptr=None)) == L.E_ARG and call(dst=dict(ptr=None)) == L.E_ARG
    for field, bad in (('n', 3), ('h', 9), ('w', 4), ('c', 6)):
        assert call(dst={field: bad}) == L.E_ARG, field
        assert call(src={field: bad}) == L.E_ARG, field
    assert call(src=dict(n=0), dst=dict(n=0)) == L.E_ARG
    assert call(src=dict(pitch=2)) == L.E_ARG and call(dst=dict(pitch=2)) == L.E_ARG
    assert call(group_c=2) == L.E_ARG and call(group_c=0) == L.E_ARG
    assert call(src=dict(c=4), dst=dict(c=4)) == L.E_ARG                     # c no multiple of group_c
    assert call(sample0=-1) == L.E_ARG and call(direction=2) == L.E_ARG and call(direction=-1) == L.E_ARG
    assert call(src=dict(ptr=A + 1)) == L.E_ARG and call(dtype=L.F32, dst=dict(ptr=A + 2)) == L.E_ARG
    big = dict(h=1 << 15, w=1 << 15, pitch=8)
    assert call(src=big, dst=big) == L.E_SHAPE
    assert call(src=dict(n=65536), dst=dict(n=65536)) == L.E_SHAPE
    draw = lambda params=A, n=4, h=16, w=16, policy=15, launches=A: lib.gan_diffaug_draw(params, n, h, w, policy, 123, 48, launches, None)
    assert draw(params=None) == L.E_ARG and draw(launches=None) == L.E_ARG
    assert draw(n=0) == L.E_ARG and draw(n=129) == L.E_ARG and draw(h=0) == L.E_ARG and draw(w=0) == L.E_ARG
    assert draw(policy=16) == L.E_ARG and draw(params=A + 2) == L.E_ARG and draw(launches=A + 1) == L.E_ARG


# ---- command line ---------------------------------------------------------------------------------------------------------------------
BASE = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']


def test_diffaugment_flag(capsys):
    from gan_amd import pix2pix
    from gan_amd.runner import config_of
    o = pix2pix.parse_opt(BASE)
    assert o.diffaugment == '' and config_of(o)['diffaugment'] == ''                    # the default: none (the reference)
    assert 'diffaugment' not in vars(o) and config_of(o)['data'] == 'd'                 # ... beside the flags both drivers are compared on
    for text, want in (('translation', 'translation'), ('cutout,translation', 'translation,cutout'),
                       ('saturation,brightness,cutout,translation', 'translation,cutout,brightness,saturation'), ('', '')):
        o = pix2pix.parse_opt(BASE + ['--diffaugment', text])
        assert o.diffaugment == want and config_of(o)['diffaugment'] == want            # (what config.json records)
    for bad in ('contrast', 'translation,contrast', 'cutout,,translation'):
        with pytest.raises(SystemExit):
            pix2pix.parse_opt(BASE + ['--diffaugment', bad])
        assert '--diffaugment' in capsys.readouterr().err


def test_cycle_gan_does_not_take_the_flag(capsys):
    from gan_amd import cycle_gan
    with pytest.raises(SystemExit):
        cycle_gan.parse_opt(['--input-images', 'x', '--target-images', 'y', '--output', 'o', '--train', '--epochs', '1', '--diffaugment', 'cutout'])
    assert 'unrecognized arguments: --diffaugment' in capsys.readouterr().err
