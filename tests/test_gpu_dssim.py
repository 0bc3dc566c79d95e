"""gan_dssim through the C ABI on the GPU against the fp64 autograd reference tests/dssim_ref.py.

The reference is evaluated on the STORED values (after the rounding to bf16 / fp16).  Loss: within the SSIM gate of
tests/test_gpu_quality.py for the image kind, equal to 1 - mean of gan_image_quality's ssim column on the same buffers to 2e-6,
exactly 0 for a == b.  Gradient: e = max|got - want| / max|want| <= 8 * yardstick + ulp(dtype_da), where the yardstick is the same
reference run in float32 on the CPU against the fp64 one, computed per case at run time (the factor 8: the different summation
order of a tiled, separable transposed filter), and ulp is 2^-8 (bf16), 2^-11 (fp16), 0 (fp32).

Every call of run_dssim goes through guarded buffers: NaN in the pad channels of a and b and around them, a sentinel in da's pad
channels and guard regions (the images beyond n), which must keep their bits, and every real channel of da must have been written."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dssim_ref as R
from tests.test_gpu_quality import SSIM_GATE, make_pair

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
ULP = {'f32': 0.0, 'bf16': 2.0 ** -8, 'f16': 2.0 ** -11}
DTYPE_TRIPLES = [('f32', 'f32', 'f32'), ('bf16', 'f32', 'bf16'), ('f16', 'f16', 'f16'), ('bf16', 'bf16', 'bf16')]
# (11, 11): map 1 x 1; (21, 22): no pixel sees a full window set; (42, 43) / (43, 42): the 32 boundary in pixels and in the map at
# 32 / 33; (53, 75): three tiles, ragged
HW = [(11, 11), (12, 17), (21, 22), (42, 43), (43, 42), (53, 75)]
NC = [(1, 1), (1, 3), (3, 1), (3, 3)]
KINDS = ('noise', 'smooth', 'flat', 'const', 'same')
SENTINEL = -3.0
# grad_scale of the reference comparison: the product's lambda.  With grad_scale 1 the gradients of these shapes (0.5 / (n c |M|) times
# a sum of order 1 to 10: at most 1e-4) would sit in fp16's subnormal range, where the spacing is absolute (2^-24) and the relative
# ulp(fp16) = 2^-11 of the gate has no meaning; the step never writes them unscaled (lambda, and the fp16 loss scale on top).
GRAD_SCALE = 100.0
GUARD = 2048


def _code(dt):
    from gan_amd import _lib as L
    return {'f32': L.F32, 'bf16': L.BF16, 'f16': L.F16}[dt]


class Padded:
    """An NHWC batch inside a wider buffer: `pitch` channels per pixel and GUARD elements on both sides (the second guard stands
    for the images beyond n), everything but the real channels prefilled with `fill`."""

    def __init__(self, shape, dt, pitch, fill, values=None):
        n, h, w, c = shape
        self.shape, self.pitch, self.dt = shape, pitch, dt
        self.flat = torch.full((2 * GUARD + n * h * w * pitch,), fill, dtype=TD[dt], device='cuda:0')
        self.body = self.flat[GUARD:GUARD + n * h * w * pitch].view(n, h, w, pitch)
        if values is not None:
            self.body[..., :c] = values
        self.before = self.flat.clone()

    def tensor(self):
        from gan_amd import _lib as L
        n, h, w, c = self.shape
        return L.GanTensor(self.body.data_ptr(), n, h, w, c, self.pitch)

    def real(self):
        return self.body[..., :self.shape[3]]

    def outside_unchanged(self):
        """pad channels and guard regions keep their bits"""
        it = torch.int16 if self.flat.element_size() == 2 else torch.int32
        now, was = self.flat.view(it).clone(), self.before.view(it).clone()
        n, h, w, c = self.shape
        now[GUARD:GUARD + n * h * w * self.pitch].view(n, h, w, self.pitch)[..., :c] = 0
        was[GUARD:GUARD + n * h * w * self.pitch].view(n, h, w, self.pitch)[..., :c] = 0
        return torch.equal(now, was)


def stored(x64, dt):
    return torch.from_numpy(np.ascontiguousarray(x64)).to(TD[dt]).cuda()


def run_dssim(a, b, dts, pitch=None, grad=True, grad_scale=1.0, loss_scale=1.0, loss0=None, ls=None, stream=None):
    """a, b: stored device tensors [n, h, w, c] of dtypes dts[0], dts[1] -> (loss tensor [1], da [n, h, w, c] of dts[2] or None)."""
    from gan_amd import _lib as L
    lib = L.load()
    dta, dtb, dtd = dts
    shape = tuple(a.shape)
    n, h, w, c = shape
    pitch = pitch or c
    pa = Padded(shape, dta, pitch, float('nan'), a)
    pb = Padded(shape, dtb, pitch, float('nan'), b)
    pd = Padded(shape, dtd, pitch, SENTINEL)
    ws = torch.full((lib.gan_dssim_workspace_bytes(n, h, w, c) // 4,), float('nan'), device='cuda:0')
    out = torch.full((3,), 0.25 if loss0 is None else loss0, device='cuda:0')          # [1]: the loss; [0], [2]: neighbours
    d = L.GanDssimDesc(_code(dta), _code(dtb), pa.tensor(), pb.tensor(), loss_scale, int(loss0 is not None), out.data_ptr() + 4, grad_scale,
                       _code(dtd), pd.tensor() if grad else L.GanTensor(), ws.data_ptr(), ws.numel() * 4,
                       ls.data_ptr() if ls is not None else None)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    L.check(lib.gan_dssim(C.byref(d), st), "dssim")
    torch.cuda.synchronize()
    assert out[0] == out[2] == (0.25 if loss0 is None else loss0), "loss_out's neighbours"
    assert pd.outside_unchanged(), ("da: pad channels / guards", shape, dts, pitch)
    assert torch.equal(pa.flat.view(torch.uint8), pa.before.view(torch.uint8)) and torch.equal(pb.flat.view(torch.uint8), pb.before.view(torch.uint8))
    if not grad:
        assert bool((pd.flat == SENTINEL).all())
        return out[1:2].clone(), None
    da = pd.real().clone()
    assert not bool((da == SENTINEL).any()) and bool(torch.isfinite(da.float()).all()), ("da: every real channel written", shape, dts, pitch)
    return out[1:2].clone(), da


def quality_ssim(a, b, dts):
    from gan_amd import _lib as L
    lib = L.load()
    n, h, w, c = a.shape
    ws = torch.empty(lib.gan_image_quality_workspace_bytes(n, h, w, c) // 4, device='cuda:0')
    out = torch.empty((n, 4), device='cuda:0')
    d = L.GanQualityDesc(_code(dts[0]), _code(dts[1]), L.GanTensor(a.data_ptr(), n, h, w, c, c), L.GanTensor(b.data_ptr(), n, h, w, c, c),
                         out.data_ptr(), ws.data_ptr(), ws.numel() * 4)
    L.check(lib.gan_image_quality(C.byref(d), torch.cuda.current_stream().cuda_stream), "image_quality")
    return out[:, 0].double().cpu().numpy()


_REF = {}


def reference(kind, shape, dta, dtb, seed=None):
    """-> (a, b stored on the device, fp64 loss, fp64 gradient [numpy], yardstick).  Computed once per case and shared."""
    key = (kind, shape, dta, dtb, seed)
    if key not in _REF:
        a64, b64 = make_pair(kind, shape, 100 + KINDS.index(kind) if seed is None else seed)
        a, b = stored(a64, dta), stored(b64, dtb)
        if kind == 'same':          # equal as STORED (exact: dtb is fp32 or a's own dtype)
            b = a.to(TD[dtb])
        as_, bs_ = a.double().cpu().numpy(), b.double().cpu().numpy()
        loss, g64 = R.loss_and_grad(as_, bs_)
        _, g32 = R.loss_and_grad(as_, bs_, torch.float32)
        g64 = g64.numpy()
        scale = np.abs(g64).max()
        yard = float(np.abs(g32.double().numpy() - g64).max() / scale) if scale > 0 else 0.0
        _REF[key] = (a, b, loss, g64, yard)
    return _REF[key]


def grad_error(da, want):
    return float(np.abs(da.double().cpu().numpy() - want).max() / np.abs(want).max())


@pytest.mark.parametrize('hw', HW, ids=lambda s: 'x'.join(map(str, s)))
def test_matches_fp64_reference(hw):
    worst = {k: (0.0, 0.0, 0.0) for k in KINDS}          # kind -> (e, its yardstick, e / bound)
    for n, c in NC:
        shape = (n, hw[0], hw[1], c)
        noise_scale = float(np.abs(reference('noise', shape, 'f32', 'f32')[3]).max())
        for kind in KINDS:
            for k, dts in enumerate(DTYPE_TRIPLES):
                a, b, loss, g64, yard = reference(kind, shape, dts[0], dts[1])
                for pitch in (c, 8):
                    got_loss, da = run_dssim(a, b, dts, pitch, grad_scale=GRAD_SCALE)
                    got_loss = float(got_loss[0])
                    what = f"dssim {shape} {'/'.join(dts)} pitch {pitch} {kind}"
                    ssim_q = quality_ssim(a, b, dts)
                    e_q = abs(got_loss - (1.0 - ssim_q.mean()))
                    if kind == 'same':
                        amax = float(da.double().abs().max())
                        print(f"{what}: loss {got_loss!r} max|da| {amax:.3e} (noise max|want| {noise_scale:.3e})")
                        assert got_loss == 0.0, what
                        assert amax <= SSIM_GATE['noise'] * GRAD_SCALE * noise_scale, (what, amax)
                        assert e_q <= 2e-6, (what, e_q)
                        continue
                    e_loss = abs(got_loss - loss)
                    e = grad_error(da, GRAD_SCALE * g64)
                    bound = 8 * yard + ULP[dts[2]]
                    print(f"{what}: loss err {e_loss:.3e} vs quality {e_q:.3e} grad e {e:.3e} yardstick {yard:.3e} bound {bound:.3e}")
                    if e / bound > worst[kind][2]:
                        worst[kind] = (e, yard, e / bound)
                    assert e_loss <= SSIM_GATE[kind], (what, e_loss)
                    assert e_q <= 2e-6, (what, e_q)
                    assert e <= bound, (what, e, yard, bound)
    for kind, (e, yard, ratio) in worst.items():
        if kind != 'same':
            print(f"dssim worst {hw} {kind}: e {e:.3e} yardstick {yard:.3e} e/bound {ratio:.3f}")


@pytest.mark.parametrize('shape', [(1, 53, 75, 1), (1, 43, 42, 3)], ids=lambda s: 'x'.join(map(str, s)))
def test_impulse_at_every_corner_edge_and_seam(shape):
    """a = b + 0.5 delta(p) on the smooth kind, p at the corners, the edge midpoints and on both sides of pixel rows / columns 10,
    31 / 32 and h - 11 (w - 11): the full gradient within the gate (halo and ownership errors)."""
    n, h, w, c = shape
    _, b64 = make_pair('smooth', shape, 7)
    b = stored(b64, 'f32')
    ys = sorted({0, h - 1, h // 2, *(y for y in (9, 10, 11, 31, 32, h - 12, h - 11, h - 10) if 0 <= y < h)})
    xs = sorted({0, w - 1, w // 2, *(x for x in (9, 10, 11, 31, 32, w - 12, w - 11, w - 10) if 0 <= x < w)})
    worst = 0.0
    for y in ys:
        for x in xs:
            a = b.clone()
            a[0, y, x, (y + x) % c] += 0.5
            _, g64 = R.loss_and_grad(a.double().cpu().numpy(), b.double().cpu().numpy())
            _, g32 = R.loss_and_grad(a.double().cpu().numpy(), b.double().cpu().numpy(), torch.float32)
            g64 = g64.numpy()
            yard = float(np.abs(g32.double().numpy() - g64).max() / np.abs(g64).max())
            _, da = run_dssim(a, b, ('f32', 'f32', 'f32'))
            e = grad_error(da, g64)
            worst = max(worst, e / (8 * yard))
            assert e <= 8 * yard, (y, x, e, yard)
    print(f"dssim impulse {shape}: {len(ys) * len(xs)} positions, worst e / (8 * yardstick) {worst:.3f}")


def test_loss_scale_state_scales_the_gradient_only_and_accumulate_adds():
    shape = (3, 43, 42, 3)
    a, b, loss, g64, yard = reference('smooth', shape, 'f32', 'f32')
    dts = ('f32', 'f32', 'f32')
    l0, d0 = run_dssim(a, b, dts, 8, grad_scale=100.0)
    ls = torch.tensor([64.0, 1.0 / 64.0, 0.0, 0.0], device='cuda:0')
    l1, d1 = run_dssim(a, b, dts, 8, grad_scale=100.0, ls=ls)
    assert torch.equal(d1, d0 * 64.0) and torch.equal(l1, l0)
    assert torch.equal(ls.cpu(), torch.tensor([64.0, 1.0 / 64.0, 0.0, 0.0]))
    assert grad_error(d0, 100.0 * g64) <= 8 * yard
    l2, _ = run_dssim(a, b, dts, 8, loss_scale=0.5, loss0=2.0)
    assert float(l2[0]) == float(torch.tensor(2.0) + (l0[0].cpu() * 0.5))
    l3, none = run_dssim(a, b, dts, 8, grad=False)                       # loss only: same bits
    assert none is None and torch.equal(l3, l0)


def test_deterministic_and_an_image_does_not_depend_on_the_rest_of_the_batch():
    shape = (3, 53, 75, 3)
    a, b, _, _, _ = reference('noise', shape, 'f32', 'f32')
    dts = ('f32', 'f32', 'f32')
    l0, d0 = run_dssim(a, b, dts, 8)
    l1, d1 = run_dssim(a, b, dts, 8)
    assert torch.equal(l0, l1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32))
    for i in range(3):
        _, di = run_dssim(a[i:i + 1].contiguous(), b[i:i + 1].contiguous(), dts, 8)
        want = di[0].double().cpu().numpy() / 3.0
        got = d0[i].double().cpu().numpy()
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got - want) <= ulp), (i, float((np.abs(got - want) / ulp).max()))
    a16, b16, _, _, _ = reference('noise', shape, 'bf16', 'f32')
    x = run_dssim(a16, b16, ('bf16', 'f32', 'bf16'), 8)
    y = run_dssim(a16, b16, ('bf16', 'f32', 'bf16'), 8)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int16), y[1].view(torch.int16))


def test_refused_arguments_write_nothing():
    from gan_amd import _lib as L
    lib = L.load()
    shape = (2, 21, 22, 3)
    n, h, w, c = shape
    a, b, _, _, _ = reference('smooth', shape, 'f32', 'f32')
    da = torch.full(shape, SENTINEL, device='cuda:0')
    ws = torch.full((64,), SENTINEL, device='cuda:0')
    out = torch.full((1,), SENTINEL, device='cuda:0')
    T = lambda t, **kw: L.GanTensor(**{**dict(ptr=t.data_ptr(), n=n, h=h, w=w, c=c, pitch=c), **kw})

    def desc(**kw):
        f = dict(dtype_a=L.F32, dtype_b=L.F32, a=T(a), b=T(b), loss_scale=1.0, loss_accumulate=0, loss_out=out.data_ptr(), grad_scale=1.0,
                 dtype_da=L.F32, da=T(da), workspace=ws.data_ptr(), workspace_bytes=ws.numel() * 4, scale_state=None)
        f.update(kw)
        return L.GanDssimDesc(**f)
    st = torch.cuda.current_stream().cuda_stream
    cases = [(L.E_ARG, dict(dtype_a=5)), (L.E_ARG, dict(dtype_da=-1)), (L.E_ARG, dict(a=T(a, c=2))), (L.E_ARG, dict(b=T(b, h=h + 1))),
             (L.E_ARG, dict(da=T(da, w=w - 1))), (L.E_ARG, dict(a=T(a, pitch=2))), (L.E_ARG, dict(loss_out=None)),
             (L.E_ARG, dict(workspace=None)), (L.E_ARG, dict(loss_accumulate=2)),
             (L.E_SHAPE, dict(a=T(a, h=10), b=T(b, h=10), da=T(da, h=10))), (L.E_SHAPE, dict(a=T(a, w=4097), b=T(b, w=4097), da=T(da, w=4097))),
             (L.E_WORKSPACE, dict(workspace_bytes=4 * n - 4)), (L.E_WORKSPACE, dict(workspace_bytes=0))]
    for code, kw in cases:
        assert lib.gan_dssim(C.byref(desc(**kw)), st) == code, kw
    d = desc()
    d.struct_size -= 4
    assert lib.gan_dssim(C.byref(d), st) == L.E_ARG
    torch.cuda.synchronize()
    for t in (da, ws, out):
        assert bool((t == SENTINEL).all())
    assert lib.gan_dssim(C.byref(desc()), st) == 0          # and the good descriptor runs
    torch.cuda.synchronize()
    assert not bool((da == SENTINEL).any()) and float(out[0]) != SENTINEL


def test_capturable():
    from gan_amd import _lib as L
    from gan_amd.nets import Ctx
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=16)
    lib = L.load()
    shape = (3, 43, 74, 3)
    n, h, w, c = shape
    a, b, _, _, _ = reference('smooth', shape, 'bf16', 'f32')
    eager_loss, eager_da = run_dssim(a, b, ('bf16', 'f32', 'bf16'))
    da = torch.zeros(shape, dtype=torch.bfloat16, device='cuda:0')
    out = torch.zeros(1, device='cuda:0')
    ws = torch.zeros(lib.gan_dssim_workspace_bytes(n, h, w, c) // 4, device='cuda:0')
    d = L.GanDssimDesc(L.BF16, L.F32, L.GanTensor(a.data_ptr(), n, h, w, c, c), L.GanTensor(b.data_ptr(), n, h, w, c, c), 1.0, 0, out.data_ptr(),
                       1.0, L.BF16, L.GanTensor(da.data_ptr(), n, h, w, c, c), ws.data_ptr(), ws.numel() * 4, None)
    torch.cuda.synchronize()
    gr = ctx.capture_graph(lambda: L.check(lib.gan_dssim(C.byref(d), ctx.stream()), "dssim"))
    for _ in range(2):
        da.fill_(float('nan'))
        out.fill_(float('nan'))
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager_loss) and torch.equal(da.view(torch.int16), eager_da.view(torch.int16))
