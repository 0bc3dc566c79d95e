"""CPU tests of the Sobel edge term: the fp64 reference tests/edge_ref.py against central differences and its
corner cases; header, binding and INTEGRATION.md snippet; the descriptor's refusals (found before any launch, so they need no GPU);
the --edge-weight flag and the --resume gate."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import edge_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clear_pair(shape, floor):
    """A uniform pair none of whose |ex|, |ey| is below `floor` (the first seed that gives one)."""
    for seed in range(200):
        rng = np.random.default_rng(seed)
        a, b = rng.uniform(-1, 1, shape), rng.uniform(-1, 1, shape)
        ex, ey = R.responses(a, b)
        if min(np.abs(ex).min(), np.abs(ey).min()) >= floor:
            return a, b
    raise AssertionError("no seed gives a pair clear of the kinks")


def test_reference_gradient_matches_central_differences():
    shape = (1, 6, 7, 3)
    a, b = _clear_pair(shape, 1e-3)
    ex, ey = R.responses(a, b)
    assert min(np.abs(ex).min(), np.abs(ey).min()) >= 1e-3          # the premise: no kink of |.| within reach of eps
    want_loss, grad = R.loss_and_grad(a, b)
    assert want_loss == R.loss(a, b) and grad.shape == shape
    eps, worst = 1e-6, 0.0
    for idx in np.ndindex(*shape):
        ap, am = a.copy(), a.copy()
        ap[idx] += eps
        am[idx] -= eps
        fd = (R.loss(ap, b) - R.loss(am, b)) / (2 * eps)
        worst = max(worst, abs(fd - grad[idx]))
    print(f"edge ref central differences: worst {worst:.3e} of max|grad| {np.abs(grad).max():.3e}")
    # piecewise linear away from the kinks: no truncation error, only the cancellation 1e-16 / eps of a loss of order 1
    assert worst <= 1e-9 and np.abs(grad).max() > 1e-3
    k = R.k_map(a, b)
    assert k.dtype == np.int64 and np.abs(k).max() <= 16 and np.array_equal(k / (16.0 * 3 * 4 * 5), grad)


def test_equal_images_have_zero_loss_and_gradient():
    a, _ = _clear_pair((2, 9, 8, 3), 0.0)
    loss, grad = R.loss_and_grad(a, a.copy())
    assert loss == 0.0 and not grad.any() and not R.k_map(a, a).any()


def test_three_by_three_image_has_one_map_position():
    rng = np.random.default_rng(3)
    a, b = rng.uniform(-1, 1, (1, 3, 3, 1)), rng.uniform(-1, 1, (1, 3, 3, 1))
    ex, ey = R.responses(a, b)
    assert ex.shape == ey.shape == (1, 1, 1, 1)
    d = (a - b)[0, :, :, 0]
    assert abs(ex[0, 0, 0, 0] - (R.SX * d).sum() / 8) < 1e-15 and abs(ey[0, 0, 0, 0] - (R.SY * d).sum() / 8) < 1e-15
    assert abs(R.loss(a, b) - (abs(ex).sum() + abs(ey).sum()) / 2) < 1e-15
    k = R.k_map(a, b)[0, :, :, 0]
    assert np.array_equal(k, (R.SX * np.sign(ex.item()) + R.SY * np.sign(ey.item())).astype(np.int64))
    assert np.isinf(R.min_response(a, b)).sum() == 0


def test_a_corner_pixel_receives_only_the_positions_that_exist():
    """d = a ramp in x: ex = 1 everywhere, ey = 0.  Interior pixels gather +-(1 + 2 + 1) from both sides (0); the first two and last
    two columns keep what their missing neighbours would have cancelled."""
    h, w = 6, 7
    a = np.tile(np.arange(w, dtype=np.float64)[None, :], (h, 1))[None, :, :, None] * 0.5
    b = np.zeros_like(a)
    ex, ey = R.responses(a, b)
    assert np.all(ex == 0.125 * 8 * 0.5) and not ey.any()
    k = R.k_map(a, b)[0, :, :, 0]
    col = np.array([1, 3, 4, 4, 3, 1])          # rows 0 .. 5: the Sx column weights (1, 2, 1) of the rows 1 .. 4 that exist
    assert np.array_equal(k[:, 0], -col) and np.array_equal(k[:, 1], -col) and np.array_equal(k[:, w - 1], col) and np.array_equal(k[:, w - 2], col)
    assert not k[:, 2:w - 2].any()


def test_eager_restatement_matches_the_reference():
    from gan_amd.pix2pix import _edge_eager
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-1, 1, (2, 13, 9, 3)), rng.uniform(-1, 1, (2, 13, 9, 3))
    at = torch.from_numpy(a).float().requires_grad_(True)
    bt = torch.from_numpy(b).float()
    got = _edge_eager(at, bt)
    got.backward()
    want, grad = R.loss_and_grad(at.detach().double().numpy(), bt.double().numpy())
    assert abs(float(got.detach()) - want) <= 1e-6
    assert float(np.abs(at.grad.double().numpy() - grad).max()) <= 1e-6 * float(np.abs(grad).max())


# ---- header, binding, snippet -----------------------------------------------------------------------------------------------------
def test_header_binding_and_integration_snippet_agree():
    from gan_amd import _lib as L
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_binding
    fields = gen_binding.parse_structs()['GanEdgeDesc']
    want = [(f, getattr(C, t[2:]) if t.startswith('C.') else getattr(L, t)) for f, t in fields]
    assert list(L.GanEdgeDesc._fields_) == want and fields[0] == ('struct_size', 'C.c_uint32')
    assert [f for f, _ in fields] == [f for f, _ in L.GanDssimDesc._fields_] + ['grad_accumulate']
    assert C.sizeof(L.GanEdgeDesc) == C.sizeof(L.GanDssimDesc) + 8          # one int32 and the padding to the struct's 8-byte alignment
    hdr = open(os.path.join(ROOT, 'include', 'gan_amd.h')).read()
    for proto in (r'size_t gan_edge_workspace_bytes\(int32_t n, int32_t h, int32_t w, int32_t c\);',
                  r'int gan_edge_l1\(const GanEdgeDesc\* d, gan_stream_t stream\);'):
        assert re.search(proto, hdr), proto
    assert L.SYMBOLS['gan_edge_l1'] == (C.c_int, [C.POINTER(L.GanEdgeDesc), C.c_void_p])
    assert L.SYMBOLS['gan_edge_workspace_bytes'] == (C.c_size_t, [C.c_int32] * 4)
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    first = re.search(r"```python\nimport ctypes as C\n(.*?)```", text, flags=re.S).group(1)
    code = re.search(r"```python\n(# --- generated from include/gan_amd.h by tools/gen_binding.py GanEdgeDesc ---\n.*?)```", text, flags=re.S).group(1)
    gen = code[:code.index('# --- end of generated part')]
    assert gen.split('\n', 1)[1].strip() == gen_binding.ctypes_source(['GanEdgeDesc']).strip()
    ns = {}
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        exec("import ctypes as C\n" + first + code, ns)
    finally:
        os.chdir(cwd)
    assert C.sizeof(ns['GanEdgeDesc']) == C.sizeof(L.GanEdgeDesc) and callable(ns['add_edge_term'])
    d = ns['GanEdgeDesc'](struct_size=C.sizeof(ns['GanEdgeDesc']) - 8)
    assert ns['lib'].gan_edge_l1(C.byref(d), None) == -1
    assert 'edge.hip' in open(os.path.join(ROOT, 'gan_amd', 'csrc', 'Makefile')).read()


# ---- refusals (pointers that are never dereferenced) ------------------------------------------------------------------------------
def _good(L, grad=True):
    n, h, w, c = 3, 43, 26, 3
    ws = L.load().gan_edge_workspace_bytes(n, h, w, c)
    da = L.GanTensor(1 << 24, n, h, w, c, 8) if grad else L.GanTensor()
    return L.GanEdgeDesc(L.BF16, L.F32, L.GanTensor(4096, n, h, w, c, 8), L.GanTensor(1 << 20, n, h, w, c, c), 1.0, 0, 1 << 22, 100.0,
                         L.BF16, da, 1 << 23, ws, None, 1)


def test_edge_abi_refuses_bad_descriptors_before_any_launch():
    from gan_amd import _lib as L
    lib = L.load()
    call = lambda d: lib.gan_edge_l1(C.byref(d), None)
    assert lib.gan_edge_l1(None, None) == L.E_ARG
    assert L.GanEdgeDesc().struct_size == C.sizeof(L.GanEdgeDesc)
    # workspace: one float per (image, 32 x 32 tile of pixels); 0 for a refused shape
    wsb = lib.gan_edge_workspace_bytes
    assert wsb(1, 3, 3, 1) == 4 and wsb(3, 33, 65, 3) == 3 * 2 * 3 * 4 and wsb(16, 256, 256, 1) == 16 * 64 * 4
    assert wsb(1, 4096, 4096, 3) == 128 * 128 * 4
    assert wsb(0, 64, 64, 1) == wsb(1, 2, 64, 1) == wsb(1, 64, 2, 1) == wsb(1, 64, 64, 2) == wsb(1, 4097, 64, 1) == wsb(1, 64, 4097, 3) == 0
    assert wsb(-1, 64, 64, 1) == wsb(1, 64, 64, 0) == wsb(1, 64, 64, 4) == 0

    def bad(code, sub=None, grad=True, **fields):
        d = _good(L, grad)
        for k, v in fields.items():
            setattr(getattr(d, sub) if sub else d, k, v)
        assert call(d) == code, (sub, fields)

    bad(L.E_ARG, struct_size=C.sizeof(L.GanEdgeDesc) - 8)                 # (a GanDssimDesc is not taken for one)
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
    for flag in (-1, 2):
        bad(L.E_ARG, loss_accumulate=flag)
        bad(L.E_ARG, grad_accumulate=flag)
        bad(L.E_ARG, grad=False, grad_accumulate=flag)
    for c in (2, 4):                                    # c of all tensors alike, but not 1 or 3
        d = _good(L)
        d.a.c = d.b.c = d.da.c = c
        assert call(d) == L.E_ARG
    for n in (0, -1):
        d = _good(L)
        d.a.n = d.b.n = d.da.n = n
        assert call(d) == L.E_ARG
    for grad in (True, False):
        for f in ('h', 'w'):
            for v in (2, 1, 0, 4097):
                d = _good(L, grad)
                for t in (d.a, d.b, d.da):
                    setattr(t, f, v)
                d.workspace_bytes = 1 << 30
                assert call(d) == L.E_SHAPE, (grad, f, v)
        bad(L.E_WORKSPACE, grad=grad, workspace_bytes=_good(L).workspace_bytes - 4)
        bad(L.E_WORKSPACE, grad=grad, workspace_bytes=0)


def test_step_refuses_a_negative_weight():
    from gan_amd.steps import Pix2PixStep
    for bad in (-0.5, float('nan')):
        with pytest.raises(ValueError):
            Pix2PixStep(None, 2, 256, 1, edge_weight=bad)


# ---- CLI and the resume gate ------------------------------------------------------------------------------------------------------
BASE = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']


def test_edge_weight_flag(capsys):
    from gan_amd import cycle_gan, pix2pix
    from gan_amd.runner import config_of
    o = pix2pix.parse_opt(BASE)
    assert o.edge_weight == 0.0 and type(o.edge_weight) is float and config_of(o)['edge_weight'] == 0.0      # the default: no edge term
    assert 'edge_weight' not in vars(o)                                   # ... beside the flags both drivers are compared on
    o = pix2pix.parse_opt(BASE + ['--edge-weight', '0.25'])
    assert o.edge_weight == 0.25 and config_of(o)['edge_weight'] == 0.25  # (what config.json records)
    assert pix2pix.parse_opt(BASE + ['--edge-weight', '0', '--generator-loss', 'dssim']).edge_weight == 0.0
    for bad in ('-1', '-0.001', 'nan', 'inf'):
        with pytest.raises(SystemExit):
            pix2pix.parse_opt(BASE + ['--edge-weight', bad])
        assert '--edge-weight' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        pix2pix.parse_opt(BASE + ['--help'])
    assert re.search(r'--edge-weight.*relative\s+to\s+--lambda', capsys.readouterr().out, flags=re.S)
    with pytest.raises(SystemExit):
        cycle_gan.parse_opt(['--input-images', 'x', '--target-images', 'y', '--output', 'o', '--train', '--epochs', '1', '--edge-weight', '0.25'])
    assert 'unrecognized arguments: --edge-weight' in capsys.readouterr().err


def test_resume_under_another_weight_is_refused_by_name(tmp_path):
    from gan_amd import tfbundle
    from gan_amd import train_state as T
    from tests.test_cpu_resume import CONFIG, _bundle
    assert 'edge_weight' in T.run_config(CONFIG) and T.run_config(CONFIG)['edge_weight'] == 0.0
    with_edge = {**CONFIG, 'edge_weight': 0.25}
    prefix = _bundle(tmp_path / 'e', with_edge)
    assert T.check_resume(prefix, with_edge) == prefix
    assert T.check_resume(prefix, {**with_edge, 'edge_weight': '0.25'}) == prefix
    for other in ({**CONFIG, 'edge_weight': 0.5}, {**CONFIG, 'edge_weight': 0.0}, CONFIG):
        with pytest.raises(T.ResumeRefused) as e:
            T.check_resume(prefix, other)
        assert ' edge_weight ' in str(e.value)
    plain = _bundle(tmp_path / 'p', CONFIG)
    with pytest.raises(T.ResumeRefused) as e:
        T.check_resume(plain, with_edge)
    assert ' edge_weight ' in str(e.value)
    # a checkpoint written before the key existed: its stored config has no such entry and resumes as weight 0
    stored = T.run_config(CONFIG)
    del stored['edge_weight']
    os.makedirs(tmp_path / 'old')
    old = tfbundle.write_bundle(os.path.join(str(tmp_path / 'old'), 'ckpt-1'),
                                {'generator/layer_with_weights-15/bias/.ATTRIBUTES/VARIABLE_VALUE': np.zeros(1, np.float32),
                                 'train_state/epoch': np.array(2, np.int64), 'train_state/config': T._json_array(stored)})
    assert T.check_resume(old, CONFIG) == old and T.check_resume(old, {**CONFIG, 'edge_weight': 0.0}) == old
    with pytest.raises(T.ResumeRefused) as e:
        T.check_resume(old, with_edge)
    assert ' edge_weight ' in str(e.value)
