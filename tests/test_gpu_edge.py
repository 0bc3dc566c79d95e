"""gan_edge_l1 through the C ABI on the GPU against the fp64 reference tests/edge_ref.py.

The reference is evaluated on the STORED values (after the rounding to bf16 / fp16).  Exact cases: operands that are multiples of
2^-6 in [-1, 1], for which every stored value, every d, every Sobel sum and every 32 x 32 partial sum is exact in fp32 - the integer
map k comes back exactly, the loss within 4 fp32 ulps (the double -> float rounding, the scale, the accumulate), 16-bit gradients as
the rounding of the header's fp32 product.  General cases: uniform operands, loss within 2048 * 2^-24 relative (the bound of an
fp32 tile partial of non-negative terms), gradient compared where no contributing response is within 1e-5 of a kink of |.|.

Every call goes through guarded buffers: NaN in the pad channels of a and b and around them, a sentinel (or NaN) in da's pad
channels and guard regions, which must keep their bits, and every real channel of da must have been written."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import edge_ref as R

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
DTYPE_TRIPLES = [('f32', 'f32', 'f32'), ('bf16', 'f32', 'bf16'), ('f16', 'f16', 'f16'), ('bf16', 'bf16', 'bf16'), ('f16', 'bf16', 'f32')]
# (3, 3): one map position; (3, 40): one row of positions over two tiles; (8, 8): inside one tile; (33, 65) / (40, 35): both tile
# edges, a one-pixel-high second tile row, three tile columns
HW = [(3, 3), (3, 40), (8, 8), (33, 65), (40, 35)]
NC = [(1, 1), (1, 3), (3, 1), (3, 3)]
# (pitch or None for c, channel offsets of a, b, da inside the pitch).  Pitch 8 at offset 0 is one aligned 16-byte pixel for the
# 16-bit types (the vector load), pitch 4 for fp32; an offset view is read by elements
LAYOUTS = [(None, 0, 0, 0), (8, 0, 2, 0), (8, 3, 0, 5), (4, 0, 1, 0)]
SENTINEL = -16384.0            # exact in all three types and no gradient value: k is an integer in [-16, 16] and F stays below 7
GUARD = 2048
GRAD_SCALE = 100.0


def _code(dt):
    from gan_amd import _lib as L
    return {'f32': L.F32, 'bf16': L.BF16, 'f16': L.F16}[dt]


class View:
    """An NHWC batch inside a wider buffer: `pitch` channels per pixel, the c real ones from channel `off` on, GUARD elements on both
    sides (the second guard stands for the images beyond n); everything but the real channels prefilled with `fill`."""

    def __init__(self, shape, dt, pitch, off, fill, values=None):
        n, h, w, c = shape
        assert off + c <= pitch
        self.shape, self.pitch, self.off, self.dt = shape, pitch, off, dt
        self.flat = torch.full((2 * GUARD + n * h * w * pitch,), fill, dtype=TD[dt], device='cuda:0')
        self.body = self.flat[GUARD:GUARD + n * h * w * pitch].view(n, h, w, pitch)
        if values is not None:
            self.real()[...] = values
        self.before = self.flat.clone()

    def tensor(self):
        from gan_amd import _lib as L
        n, h, w, c = self.shape
        return L.GanTensor(self.body.data_ptr() + self.off * self.flat.element_size(), n, h, w, c, self.pitch)

    def real(self):
        return self.body[..., self.off:self.off + self.shape[3]]

    def _bits(self, t):
        return t.view(torch.int16 if self.flat.element_size() == 2 else torch.int32)

    def outside_unchanged(self):
        """pad channels and guard regions keep their bits"""
        now, was = self._bits(self.flat).clone(), self._bits(self.before).clone()
        n, h, w, c = self.shape
        for t in (now, was):
            t[GUARD:GUARD + n * h * w * self.pitch].view(n, h, w, self.pitch)[..., self.off:self.off + c] = 0
        return torch.equal(now, was)

    def untouched(self):
        return torch.equal(self._bits(self.flat), self._bits(self.before))


def stored(x64, dt):
    return torch.from_numpy(np.ascontiguousarray(x64)).to(TD[dt]).cuda()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def run_edge(a, b, dts, layout=LAYOUTS[0], grad=True, grad_scale=1.0, loss_scale=1.0, loss0=None, ls=None, da_view=None):
    """a, b: stored device tensors [n, h, w, c] of dtypes dts[0], dts[1] -> (loss tensor [1], da [n, h, w, c] of dts[2] or None).
    da_view: a View whose real channels another call filled - the gradient is accumulated into it (grad_accumulate = 1)."""
    from gan_amd import _lib as L
    lib = L.load()
    dta, dtb, dtd = dts
    shape = tuple(a.shape)
    n, h, w, c = shape
    pitch, oa, ob, od = layout
    pitch = pitch or c
    pa = View(shape, dta, pitch, oa, float('nan'), a)
    pb = View(shape, dtb, pitch, ob, float('nan'), b)
    pd = da_view if da_view is not None else View(shape, dtd, pitch, od, SENTINEL)
    ws = torch.full((lib.gan_edge_workspace_bytes(n, h, w, c) // 4,), float('nan'), device='cuda:0')
    out = torch.full((3,), 0.25 if loss0 is None else loss0, device='cuda:0')          # [1]: the loss; [0], [2]: neighbours
    d = L.GanEdgeDesc(_code(dta), _code(dtb), pa.tensor(), pb.tensor(), loss_scale, int(loss0 is not None), out.data_ptr() + 4, grad_scale,
                      _code(dtd), pd.tensor() if grad else L.GanTensor(), ws.data_ptr(), ws.numel() * 4,
                      ls.data_ptr() if ls is not None else None, int(da_view is not None))
    L.check(lib.gan_edge_l1(C.byref(d), torch.cuda.current_stream().cuda_stream), "edge_l1")
    torch.cuda.synchronize()
    assert out[0] == out[2] == (0.25 if loss0 is None else loss0), "loss_out's neighbours"
    assert pd.outside_unchanged(), ("da: pad channels / guards", shape, dts, layout)
    assert pa.untouched() and pb.untouched()
    assert bool(torch.isfinite(ws).all()), "every tile wrote its partial"
    if not grad:
        assert pd.untouched()
        return out[1:2].clone(), None
    da = pd.real().clone()
    if da_view is None:
        assert not bool((da == SENTINEL).any()), ("da: every real channel written", shape, dts, layout)
    assert bool(torch.isfinite(da.float()).all())
    return out[1:2].clone(), da


def layouts_for(c, dts):
    """The layouts a case runs: dense, the two pitch-8 ones, and pitch 4 for c = 1 or fp32 operands (c + offset must fit)."""
    return [l for l in LAYOUTS if l[0] is None or max(l[1:]) + c <= l[0]]


def factor(grad_scale, shape):
    """The header's F = (float)(grad_scale / (16 c M)), the quotient in double from the fp32 grad_scale."""
    n, h, w, c = shape
    return np.float32(float(np.float32(grad_scale)) / (16.0 * c * (h - 2) * (w - 2)))


def expected_grad(k, grad_scale, shape, dt, ls=None, old=None):
    """The header's rounding order on the reference's k: (float(k) * F) / n [* ls] in fp32, [float(old) +], one rounding to dt."""
    g = (torch.from_numpy(k.astype(np.float32)) * torch.tensor(factor(grad_scale, shape))) / torch.tensor(np.float32(shape[0]))
    if ls is not None:
        g = g * torch.tensor(np.float32(ls))
    if old is not None:
        g = old.float().cpu() + g
    return g.to(TD[dt])


_REF = {}


def exact_pair(shape):
    """Multiples of 2^-6 in [-1, 1] (exact in all three types), with a block where a == b and one that straddles the tile corner."""
    if ('exact', shape) not in _REF:
        n, h, w, c = shape
        rng = np.random.default_rng(1000 + 7 * h + w + 100 * n + c)
        a = rng.integers(-64, 65, shape).astype(np.float64) / 64.0
        b = rng.integers(-64, 65, shape).astype(np.float64) / 64.0
        a[:, 1:6, 1:7] = b[:, 1:6, 1:7]                       # responses exactly 0: sgn(0) = 0
        a[:, 29:36, 28:35] = b[:, 29:36, 28:35]               # ... across the corner of four tiles, where the image reaches it
        ex, ey = R.responses(a, b)
        if h >= 7 and w >= 8:                                 # the positions whose window lies inside the first block
            assert not ex[:, 1:4, 1:5].any() and not ey[:, 1:4, 1:5].any()
        _REF[('exact', shape)] = (a, b, R.loss(a, b), R.abs_sum(a, b), R.k_map(a, b))
    return _REF[('exact', shape)]


def general_pair(shape, dta, dtb):
    """Uniform in [-1, 1] as stored -> (a, b on the device, fp64 loss, k, mask of the comparable elements)."""
    key = ('general', shape, dta, dtb)
    if key not in _REF:
        n, h, w, c = shape
        rng = np.random.default_rng(2000 + 7 * h + w + 100 * n + c)
        a, b = stored(rng.uniform(-1, 1, shape), dta), stored(rng.uniform(-1, 1, shape), dtb)
        as_, bs_ = a.double().cpu().numpy(), b.double().cpu().numpy()
        _REF[key] = (a, b, R.loss(as_, bs_), R.k_map(as_, bs_), R.min_response(as_, bs_) >= 1e-5)
    return _REF[key]


def ulps32(got, want):
    return abs(float(got) - want) / float(np.spacing(np.float32(abs(want)))) if want else abs(float(got)) / 2.0 ** -149


@pytest.mark.parametrize('hw', HW, ids=lambda s: 'x'.join(map(str, s)))
def test_exact_cases(hw):
    worst = 0.0
    for n, c in NC:
        shape = (n, hw[0], hw[1], c)
        a64, b64, loss, _, k = exact_pair(shape)
        kscale = 16.0 * n * c * (hw[0] - 2) * (hw[1] - 2)
        assert kscale < 2 ** 24
        for dts in DTYPE_TRIPLES:
            a, b = stored(a64, dts[0]), stored(b64, dts[1])
            assert np.array_equal(a.double().cpu().numpy(), a64) and np.array_equal(b.double().cpu().numpy(), b64)      # stored exactly
            for layout in layouts_for(c, dts):
                what = f"edge exact {shape} {'/'.join(dts)} layout {layout}"
                if dts[2] == 'f32':
                    got_loss, da = run_edge(a, b, dts, layout, grad_scale=kscale)                  # F = 1: da is k itself
                    assert np.array_equal(da.double().cpu().numpy(), k.astype(np.float64)), what
                else:
                    got_loss, da = run_edge(a, b, dts, layout, grad_scale=GRAD_SCALE)
                    want = expected_grad(k, GRAD_SCALE, shape, dts[2])
                    assert torch.equal(bits(da.cpu()), bits(want)), what
                u = ulps32(got_loss[0], loss)
                worst = max(worst, u)
                assert u <= 4.0, (what, float(got_loss[0]), loss, u)
                l2, none = run_edge(a, b, dts, layout, grad=False)                                 # loss only: same bits
                assert none is None and torch.equal(l2, got_loss), what
    print(f"edge exact {hw}: worst loss error {worst:.3f} fp32 ulps (gate 4)")


def test_equal_images_give_exactly_zero():
    shape = (3, 40, 35, 3)
    a64 = exact_pair(shape)[0]
    for dts in DTYPE_TRIPLES:
        a = stored(a64, dts[0])
        loss, da = run_edge(a, a.to(TD[dts[1]]), dts, LAYOUTS[1], grad_scale=GRAD_SCALE)
        assert float(loss[0]) == 0.0 and not bool(da.float().any())


@pytest.mark.parametrize('hw', HW, ids=lambda s: 'x'.join(map(str, s)))
def test_general_cases(hw):
    worst, share = 0.0, 0.0
    for n, c in NC:
        shape = (n, hw[0], hw[1], c)
        for dts in DTYPE_TRIPLES:
            a, b, loss, k, mask = general_pair(shape, dts[0], dts[1])
            excluded = 1.0 - mask.mean()
            share = max(share, excluded)
            assert excluded <= 0.01, (shape, dts, excluded)                  # (on the reference alone)
            for layout in layouts_for(c, dts):
                what = f"edge general {shape} {'/'.join(dts)} layout {layout}"
                got_loss, da = run_edge(a, b, dts, layout, grad_scale=GRAD_SCALE)
                rel = abs(float(got_loss[0]) - loss) / loss                  # = |sum error| / sum of the absolute terms: all terms are >= 0
                worst = max(worst, rel)
                assert rel <= 2048 * 2.0 ** -24, (what, float(got_loss[0]), loss, rel)
                want = expected_grad(k, GRAD_SCALE, shape, dts[2])
                m = torch.from_numpy(mask)
                assert torch.equal(bits(da.cpu())[m], bits(want)[m]), what
    print(f"edge general {hw}: worst loss rel err {worst:.3e} = {worst / 2.0 ** -24:.2f} * 2^-24 (gate 2048 * 2^-24); excluded share at most {share:.4f}")


def _l1_into(view, a, b, dt, grad_scale):
    """gan_l1's gradient of the same operands written into the real channels of `view` (dense a, b of view's dtype)."""
    from gan_amd import _lib as L
    lib = L.load()
    n, h, w, c = a.shape
    ws = torch.zeros(4096, device='cuda:0')
    out = torch.zeros(1, device='cuda:0')
    ta, tb = (L.GanTensor(t.data_ptr(), n, h, w, c, c) for t in (a, b))
    td = view.tensor()
    L.check(lib.gan_l1(_code(dt), C.byref(ta), C.byref(tb), 1.0, 0, out.data_ptr(), grad_scale, C.byref(td), ws.data_ptr(), None,
                       torch.cuda.current_stream().cuda_stream), "l1")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('dt', ['f32', 'bf16', 'f16'])
def test_grad_accumulate_adds_to_what_gan_l1_wrote(dt):
    shape = (3, 33, 65, 3)
    a64, b64, _, _, k = exact_pair(shape)
    a, b = stored(a64, dt), stored(b64, dt)
    for layout in [(8, 0, 2, 1), (None, 0, 0, 0)]:
        view = View(shape, dt, layout[0] or shape[3], layout[3], float('nan'))
        _l1_into(view, a, b, dt, GRAD_SCALE)
        old = view.real().clone()
        assert bool(torch.isfinite(old.float()).all()) and bool(old.float().any())
        view.before = view.flat.clone()                          # pads and guards: NaN, and they stay NaN bit for bit
        _, da = run_edge(a, b, (dt, dt, dt), layout, grad_scale=0.25 * GRAD_SCALE, da_view=view)
        want = expected_grad(k, 0.25 * GRAD_SCALE, shape, dt, old=old)
        assert torch.equal(bits(da.cpu()), bits(want)), (dt, layout)
        assert not torch.equal(bits(da), bits(old))


def test_loss_accumulate_adds_and_scale_state_scales_the_gradient_only():
    shape = (3, 40, 35, 3)
    dts = ('f32', 'f32', 'f32')
    a, b, loss, k, mask = general_pair(shape, 'f32', 'f32')
    l0, d0 = run_edge(a, b, dts, LAYOUTS[1], grad_scale=GRAD_SCALE)
    ls = torch.tensor([64.0, 1.0 / 64.0, 0.0, 0.0], device='cuda:0')
    l1, d1 = run_edge(a, b, dts, LAYOUTS[1], grad_scale=GRAD_SCALE, ls=ls)
    assert torch.equal(d1, d0 * 64.0) and torch.equal(l1, l0) and bool(d0.any())
    assert torch.equal(ls.cpu(), torch.tensor([64.0, 1.0 / 64.0, 0.0, 0.0]))
    ls3 = torch.tensor([3.0, 1.0 / 3.0, 0.0, 0.0], device='cuda:0')              # not a power of two: the second product rounds
    _, d3 = run_edge(a, b, dts, LAYOUTS[1], grad_scale=GRAD_SCALE, ls=ls3)
    m = torch.from_numpy(mask)
    assert torch.equal(bits(d3.cpu())[m], bits(expected_grad(k, GRAD_SCALE, shape, 'f32', ls=3.0))[m])
    l2, _ = run_edge(a, b, dts, LAYOUTS[1], loss_scale=0.5, loss0=2.0)
    assert float(l2[0]) == float(torch.tensor(2.0) + (l0[0].cpu() * 0.5))
    l4, _ = run_edge(a, b, dts, LAYOUTS[1], loss_scale=0.5)
    assert float(l4[0]) == float(l0[0].cpu() * 0.5)


def test_deterministic_and_an_image_does_not_depend_on_the_rest_of_the_batch():
    shape = (3, 33, 65, 3)
    dts = ('f32', 'f32', 'f32')
    a, b, _, _, _ = general_pair(shape, 'f32', 'f32')
    l0, d0 = run_edge(a, b, dts, LAYOUTS[1], grad_scale=GRAD_SCALE)
    l1, d1 = run_edge(a, b, dts, LAYOUTS[1], grad_scale=GRAD_SCALE)
    assert torch.equal(bits(l0), bits(l1)) and torch.equal(bits(d0), bits(d1))
    for i in range(3):
        _, di = run_edge(a[i:i + 1].contiguous(), b[i:i + 1].contiguous(), dts, LAYOUTS[1], grad_scale=GRAD_SCALE)
        want = di[0].double().cpu().numpy() / 3.0
        got = d0[i].double().cpu().numpy()
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got - want) <= ulp), (i, float((np.abs(got - want) / ulp).max()))
    a16, b16, _, _, _ = general_pair(shape, 'bf16', 'f32')
    x = run_edge(a16, b16, ('bf16', 'f32', 'bf16'), LAYOUTS[1], grad_scale=GRAD_SCALE)
    y = run_edge(a16, b16, ('bf16', 'f32', 'bf16'), LAYOUTS[1], grad_scale=GRAD_SCALE)
    assert torch.equal(bits(x[0]), bits(y[0])) and torch.equal(bits(x[1]), bits(y[1]))


def test_refused_arguments_write_nothing():
    from gan_amd import _lib as L
    lib = L.load()
    shape = (2, 8, 8, 3)
    n, h, w, c = shape
    a, b, _, _, _ = general_pair(shape, 'f32', 'f32')
    da = torch.full(shape, SENTINEL, device='cuda:0')
    ws = torch.full((64,), SENTINEL, device='cuda:0')
    out = torch.full((1,), SENTINEL, device='cuda:0')
    T = lambda t, **kw: L.GanTensor(**{**dict(ptr=t.data_ptr(), n=n, h=h, w=w, c=c, pitch=c), **kw})

    def desc(**kw):
        f = dict(dtype_a=L.F32, dtype_b=L.F32, a=T(a), b=T(b), loss_scale=1.0, loss_accumulate=0, loss_out=out.data_ptr(), grad_scale=1.0,
                 dtype_da=L.F32, da=T(da), workspace=ws.data_ptr(), workspace_bytes=ws.numel() * 4, scale_state=None, grad_accumulate=0)
        f.update(kw)
        return L.GanEdgeDesc(**f)
    st = torch.cuda.current_stream().cuda_stream
    cases = [(L.E_ARG, dict(dtype_a=5)), (L.E_ARG, dict(dtype_da=-1)), (L.E_ARG, dict(a=T(a, c=2))), (L.E_ARG, dict(b=T(b, h=h + 1))),
             (L.E_ARG, dict(da=T(da, w=w - 1))), (L.E_ARG, dict(a=T(a, pitch=2))), (L.E_ARG, dict(loss_out=None)),
             (L.E_ARG, dict(workspace=None)), (L.E_ARG, dict(loss_accumulate=2)), (L.E_ARG, dict(grad_accumulate=2)),
             (L.E_ARG, dict(grad_accumulate=-1)),
             (L.E_SHAPE, dict(a=T(a, h=2), b=T(b, h=2), da=T(da, h=2))), (L.E_SHAPE, dict(a=T(a, w=4097), b=T(b, w=4097), da=T(da, w=4097))),
             (L.E_WORKSPACE, dict(workspace_bytes=4 * n - 4)), (L.E_WORKSPACE, dict(workspace_bytes=0))]
    for code, kw in cases:
        assert lib.gan_edge_l1(C.byref(desc(**kw)), st) == code, kw
    d = desc()
    d.struct_size -= 4
    assert lib.gan_edge_l1(C.byref(d), st) == L.E_ARG
    torch.cuda.synchronize()
    for t in (da, ws, out):
        assert bool((t == SENTINEL).all())
    assert lib.gan_edge_l1(C.byref(desc()), st) == 0          # and the good descriptor runs
    torch.cuda.synchronize()
    assert not bool((da == SENTINEL).any()) and float(out[0]) != SENTINEL


def test_capturable():
    from gan_amd import _lib as L
    from gan_amd.nets import Ctx
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=16)
    lib = L.load()
    shape = (3, 33, 65, 3)
    n, h, w, c = shape
    a, b, _, _, _ = general_pair(shape, 'bf16', 'f32')
    eager_loss, eager_da = run_edge(a, b, ('bf16', 'f32', 'bf16'), grad_scale=GRAD_SCALE)
    da = torch.zeros(shape, dtype=torch.bfloat16, device='cuda:0')
    out = torch.zeros(1, device='cuda:0')
    ws = torch.zeros(lib.gan_edge_workspace_bytes(n, h, w, c) // 4, device='cuda:0')
    d = L.GanEdgeDesc(L.BF16, L.F32, L.GanTensor(a.data_ptr(), n, h, w, c, c), L.GanTensor(b.data_ptr(), n, h, w, c, c), 1.0, 0, out.data_ptr(),
                      GRAD_SCALE, L.BF16, L.GanTensor(da.data_ptr(), n, h, w, c, c), ws.data_ptr(), ws.numel() * 4, None, 0)
    torch.cuda.synchronize()
    gr = ctx.capture_graph(lambda: L.check(lib.gan_edge_l1(C.byref(d), ctx.stream()), "edge_l1"))
    for _ in range(2):
        da.fill_(float('nan'))
        out.fill_(float('nan'))
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager_loss) and torch.equal(bits(da), bits(eager_da))
