"""gan_msssim through the C ABI on the GPU against the fp64 autograd reference tests/msssim_ref.py.

The reference is evaluated on the STORED values (after the rounding to bf16 / fp16).  Images: b a smooth pattern + 5 % noise, uniform
noise, or bright and nearly flat; a = clip(b + amp * U(-1, 1)), amp 0.1 and 0.3 (not independent noise: its CS_j sit at the clamp,
where pow is ill-conditioned).  Premise, asserted on the reference alone: every factor CS_j, S_{M-1} is at least 0.4 - except for the
flat kind at amp 0.3, where the fp64 reference itself gives CS_0 = 0.21 .. 0.24 on every shape (a flat target has cs close to
c2 / (c2 + noise variance)) and 0.2 is asserted; the loss gate is NOT widened there.
Loss gate: under the premise |dMS| <= max_j |dCS_j| / 0.4, so the gate is tests/test_gpu_quality.py's SSIM gate of the kind times 2.5.
Gradient gate: e = max|got - want| / max|want| <= 8 * yardstick + ulp(dtype_da), the yardstick being the same reference run in
float32 on the CPU against the fp64 one, per case (tests/test_gpu_dssim.py's form).

Every call of run_msssim goes through guarded buffers (test_gpu_dssim.Padded): NaN in the pad channels of a and b and around them and
in the whole workspace, NaN in da's real channels (all must be written), pad channels and guard regions (which must keep their bits)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import msssim_ref as R
from tests.test_gpu_dssim import DTYPE_TRIPLES, SENTINEL, TD, ULP, Padded, _code, grad_error, stored
from tests.test_gpu_quality import SSIM_GATE

pytestmark = pytest.mark.gpu

# odd sides on every level and the minimum size 11 * 2^(M - 1); (75, 53, 2): the 32-pixel tile edges on two levels
HWM = [(22, 23, 2), (44, 45, 3), (45, 47, 3), (88, 91, 4), (176, 177, 5), (75, 53, 2)]
KINDS = ('smooth', 'noise', 'flat')
AMPS = (0.1, 0.3)
GRAD_SCALE = 100.0          # the product's lambda (test_gpu_dssim.GRAD_SCALE: fp16 gradients out of the subnormal range)
LOSS_GATE = {k: 2.5 * SSIM_GATE[k] for k in KINDS}


def premise(kind, amp):
    return 0.2 if (kind, amp) == ('flat', 0.3) else 0.4


def make_images(kind, shape, amp, seed):
    """-> (a, b) float64 raw images in [-1, 1]"""
    n, h, w, c = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    ph = rng.uniform(0, 6.28, (n, 1, 1, c))
    wave = np.sin(0.21 * yy[None, :, :, None] + ph) * np.cos(0.13 * xx[None, :, :, None] - ph)
    if kind == 'smooth':
        b = 0.7 * wave + 0.05 * rng.uniform(-1, 1, shape)
    elif kind == 'noise':
        b = rng.uniform(-1, 1, shape)
    else:                        # display 0.98 + 0.01 sin: bright, nearly flat
        b = 2 * (0.98 + 0.01 * wave) - 1
    return np.clip(b + amp * rng.uniform(-1, 1, shape), -1, 1), b


def run_msssim(a, b, dts, scales, power=None, pitch=None, grad=True, grad_scale=1.0, loss_scale=1.0, loss0=None, ls=None, da0=None,
               stream=None, want_scores=True):
    """a, b: stored device tensors [n, h, w, c] of dtypes dts[0], dts[1] -> (loss tensor [1], da [n, h, w, c] of dts[2] or None,
    per_image [n] or None).  da0: values da holds before the call, which then runs with grad_accumulate = 1."""
    from gan_amd import _lib as L
    lib = L.load()
    dta, dtb, dtd = dts
    shape = tuple(a.shape)
    n, h, w, c = shape
    pitch = pitch or c
    pa = Padded(shape, dta, pitch, float('nan'), a)
    pb = Padded(shape, dtb, pitch, float('nan'), b)
    pd = Padded(shape, dtd, pitch, float('nan'), da0)          # (NaN, not a value: a bf16 gradient may be any number)
    need = lib.gan_msssim_workspace_bytes(n, h, w, c, scales)
    assert need > 0, (shape, scales)
    ws = torch.full((need // 4 + 2,), float('nan'), device='cuda:0')          # + 2: a guard behind the workspace
    ws[-2:] = SENTINEL
    out = torch.full((3,), 0.25 if loss0 is None else loss0, device='cuda:0')          # [1]: the loss; [0], [2]: neighbours
    per = torch.full((n + 2,), SENTINEL, device='cuda:0')
    d = L.GanMsssimDesc(_code(dta), _code(dtb), pa.tensor(), pb.tensor(), loss_scale, int(loss0 is not None), out.data_ptr() + 4, grad_scale,
                        _code(dtd), pd.tensor() if grad else L.GanTensor(), ws.data_ptr(), need,
                        ls.data_ptr() if ls is not None else None, scales, L.msssim_power(scales, power),
                        per.data_ptr() + 4 if want_scores else None, int(da0 is not None))
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    L.check(lib.gan_msssim(C.byref(d), st), "msssim")
    torch.cuda.synchronize()
    assert out[0] == out[2] == (0.25 if loss0 is None else loss0), "loss_out's neighbours"
    assert per[0] == per[-1] == SENTINEL and bool((ws[-2:] == SENTINEL).all()), "per_image's neighbours / behind the workspace"
    assert pd.outside_unchanged(), ("da: pad channels / guards", shape, dts, pitch)
    assert torch.equal(pa.flat.view(torch.uint8), pa.before.view(torch.uint8)) and torch.equal(pb.flat.view(torch.uint8), pb.before.view(torch.uint8))
    scores = per[1:-1].clone() if want_scores else None
    if not want_scores:
        assert bool((per == SENTINEL).all())
    if not grad:
        assert torch.equal(pd.flat.view(torch.uint8), pd.before.view(torch.uint8))
        return out[1:2].clone(), None, scores
    da = pd.real().clone()
    assert bool(torch.isfinite(da.float()).all()), ("da: every real channel written", shape, dts, pitch)
    return out[1:2].clone(), da, scores


_REF = {}


def reference(kind, shape, amp, scales, dta, dtb, seed=None):
    """-> (a, b stored on the device, fp64 loss, fp64 gradient [numpy], yardstick, fp64 scores [n], smallest factor).  Computed
    once per case with n = 3 and shared; the batch-1 case is its first image (loss 1 - score_0, gradient 3 x that of image 0)."""
    n, h, w, c = shape
    key = (kind, (3, h, w, c), amp, scales, dta, dtb, seed)
    if key not in _REF:
        a64, b64 = make_images(kind, (3, h, w, c), amp, 100 + KINDS.index(kind) if seed is None else seed)
        a, b = stored(a64, dta), stored(b64, dtb)
        as_, bs_ = a.double().cpu().numpy(), b.double().cpu().numpy()
        loss, g64, sc = R.loss_and_grad(as_, bs_, scales)
        _, g32, _ = R.loss_and_grad(as_, bs_, scales, dtype=torch.float32)
        _REF[key] = (a, b, loss, g64.numpy(), g32.double().numpy(), sc, R.min_factor(as_, bs_, scales))
    a, b, loss, g64, g32, sc, fmin = _REF[key]
    if n == 1:
        a, b, loss, g64, g32, sc = a[:1].contiguous(), b[:1].contiguous(), 1.0 - float(sc[0]), 3.0 * g64[:1], 3.0 * g32[:1], sc[:1]
    else:
        assert n == 3
    yard = float(np.abs(g32 - g64).max() / np.abs(g64).max())
    return a, b, loss, g64, yard, sc, fmin


@pytest.mark.parametrize('amp', AMPS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('hwm', HWM, ids=lambda s: 'x'.join(map(str, s)))
def test_matches_fp64_reference(hwm, kind, amp):
    h, w, scales = hwm
    worst = (0.0, 0.0, 0.0, 0.0)            # e / bound, e, its yardstick, loss error / gate
    for c in (1, 3):
        for n in (3, 1):
            shape = (n, h, w, c)
            for dts in DTYPE_TRIPLES:
                a, b, loss, g64, yard, sc, fmin = reference(kind, shape, amp, scales, dts[0], dts[1])
                assert fmin >= premise(kind, amp), (shape, kind, amp, dts, fmin)
                for pitch in (c, 8):
                    got_loss, da, per = run_msssim(a, b, dts, scales, pitch=pitch, grad_scale=GRAD_SCALE)
                    what = f"msssim {shape} M {scales} {'/'.join(dts)} pitch {pitch} {kind} amp {amp}"
                    e_loss = abs(float(got_loss[0]) - loss)
                    e_per = float(np.abs(per.double().cpu().numpy() - sc).max())
                    e = grad_error(da, GRAD_SCALE * g64)
                    bound = 8 * yard + ULP[dts[2]]
                    print(f"{what}: min factor {fmin:.3f} loss err {e_loss:.3e} per-image err {e_per:.3e} grad e {e:.3e} yardstick {yard:.3e} "
                          f"bound {bound:.3e}")
                    worst = max(worst, (e / bound, e, yard, max(e_loss, e_per) / LOSS_GATE[kind]))
                    assert e_loss <= LOSS_GATE[kind], (what, e_loss)
                    assert e_per <= LOSS_GATE[kind], (what, e_per)
                    assert e <= bound, (what, e, yard, bound)
    print(f"msssim worst {hwm} {kind} amp {amp}: e/bound {worst[0]:.3f} (e {worst[1]:.3e} yardstick {worst[2]:.3e})")


def _impulse_spots(h, w):
    ys = sorted({0, h - 1, *(y for y in (9, 10, 11, 20, 21, 31, 32, h - 12, h - 11, h - 10) if 0 <= y < h)})
    xs = sorted({0, w - 1, *(x for x in (9, 10, 11, 20, 21, 31, 32, w - 12, w - 11, w - 10) if 0 <= x < w)})
    spots = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}
    spots |= {(y, w // 2) for y in ys} | {(y, w - 1) for y in ys} | {(h // 2, x) for x in xs} | {(h - 1, x) for x in xs}
    spots |= {(ys[i % len(ys)], xs[i % len(xs)]) for i in range(max(len(ys), len(xs)))}
    return sorted(spots)


@pytest.mark.parametrize('case', [(1, 45, 47, 1, 3), (1, 75, 53, 3, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_impulse_at_corners_odd_edges_and_seams(case):
    """a = b + 0.5 delta(p) on the smooth kind: p at the corners, in the last (odd) row and column and on both sides of pixel rows /
    columns 10, 20 / 21, 31 / 32 and h - 11 (w - 11): the full gradient within the gate (a wrong pooling transpose, halo or owner)."""
    n, h, w, c, scales = case
    _, b64 = make_images('smooth', (n, h, w, c), 0.0, 7)
    b = stored(b64, 'f32')
    worst, spots = 0.0, _impulse_spots(h, w)
    for y, x in spots:
        a = b.clone()
        a[0, y, x, (y + x) % c] += 0.5
        _, g64, _ = R.loss_and_grad(a.double().cpu().numpy(), b.double().cpu().numpy(), scales)
        _, g32, _ = R.loss_and_grad(a.double().cpu().numpy(), b.double().cpu().numpy(), scales, dtype=torch.float32)
        g64 = g64.numpy()
        yard = float(np.abs(g32.double().numpy() - g64).max() / np.abs(g64).max())
        _, da, _ = run_msssim(a, b, ('f32', 'f32', 'f32'), scales)
        e = grad_error(da, g64)
        worst = max(worst, e / (8 * yard))
        assert e <= 8 * yard, (y, x, e, yard)
    print(f"msssim impulse {case}: {len(spots)} positions, worst e / (8 * yardstick) {worst:.3f}")


@pytest.mark.parametrize('hwm', [(45, 47, 3), (176, 177, 5)], ids=lambda s: 'x'.join(map(str, s)))
def test_equal_and_opposite_images_are_exact(hwm):
    h, w, scales = hwm
    shape = (3, h, w, 3)
    a64, b64 = make_images('noise', shape, 0.3, 11)
    _, s64 = make_images('smooth', shape, 0.0, 12)
    for dts in DTYPE_TRIPLES:
        a = stored(a64, dts[0])
        b = a.to(TD[dts[1]])                  # equal as STORED (exact: dtb is fp32 or a's own dtype)
        for pitch in (3, 8):
            loss, da, per = run_msssim(a, b, dts, scales, pitch=pitch, grad_scale=GRAD_SCALE)
            assert float(loss[0]) == 0.0 and bool((per == 1.0).all()) and bool((da == 0).all()), (dts, pitch)
        s = stored(s64, dts[0])
        loss, da, per = run_msssim(-s, s.to(TD[dts[1]]), dts, scales, pitch=8, grad_scale=GRAD_SCALE, loss_scale=0.375)
        assert float(loss[0]) == 0.375 and bool((per == 0.0).all()) and bool((da == 0).all()), dts


def test_one_scale_with_weight_one_is_gan_dssim():
    from tests import test_gpu_dssim as TDS
    for shape in [(3, 53, 75, 3), (1, 43, 42, 1)]:
        for dts in DTYPE_TRIPLES:
            a, b, _, g64, yard = TDS.reference('smooth', shape, dts[0], dts[1])
            l_d, da_d = TDS.run_dssim(a, b, dts, 8, grad_scale=GRAD_SCALE)
            l_m, da_m, _ = run_msssim(a, b, dts, 1, power=(1.0,), pitch=8, grad_scale=GRAD_SCALE)
            e = float((da_m.double() - da_d.double()).abs().max() / da_d.double().abs().max())
            print(f"msssim M = 1 against gan_dssim {shape} {'/'.join(dts)}: loss diff {abs(float(l_m[0]) - float(l_d[0])):.3e} grad e {e:.3e}")
            assert abs(float(l_m[0]) - float(l_d[0])) <= 2e-6
            assert e <= 8 * yard + ULP[dts[2]], (shape, dts, e, yard)


def test_per_image_is_quality_ms_ssim():
    from gan_amd import quality
    from gan_amd.nets import Ctx
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=16)
    for (h, w, scales), dts in (((176, 177, 5), ('bf16', 'f32', 'bf16')), ((45, 47, 3), ('f32', 'f32', 'f32'))):
        a, b, _, _, _, sc, _ = reference('smooth', (3, h, w, 3), 0.3, scales, dts[0], dts[1])
        _, _, per = run_msssim(a, b, dts, scales, grad=False)
        got = quality.ms_ssim(ctx, a, b, scales=scales)
        again = quality.ms_ssim(ctx, a, b.cpu().numpy(), scales=scales)       # the cached workspace, a host target
        torch.cuda.synchronize()
        assert got.shape == (3,) and torch.equal(got, per) and torch.equal(again, per)
        assert float(np.abs(got.double().cpu().numpy() - sc).max()) <= LOSS_GATE['smooth']
    with pytest.raises(ValueError):
        quality.ms_ssim(ctx, a, b, scales=5)                                  # 45 x 47 holds three scales


def test_scale_state_accumulation_and_loss_only():
    shape, scales = (3, 45, 47, 3), 3
    dts = ('f32', 'f32', 'f32')
    a, b, loss, g64, yard, _, _ = reference('smooth', shape, 0.3, scales, 'f32', 'f32')
    l0, d0, p0 = run_msssim(a, b, dts, scales, pitch=8, grad_scale=100.0)
    ls = torch.tensor([64.0, 1.0 / 64.0, 0.0, 0.0], device='cuda:0')
    l1, d1, _ = run_msssim(a, b, dts, scales, pitch=8, grad_scale=100.0, ls=ls)
    assert torch.equal(d1, d0 * 64.0) and torch.equal(l1, l0)
    assert torch.equal(ls.cpu(), torch.tensor([64.0, 1.0 / 64.0, 0.0, 0.0]))
    l2, _, _ = run_msssim(a, b, dts, scales, pitch=8, loss_scale=0.5, loss0=2.0)
    assert float(l2[0]) == float(torch.tensor(2.0) + (l0[0].cpu() * 0.5))
    l3, none, p3 = run_msssim(a, b, dts, scales, pitch=8, grad=False)             # loss only: same bits
    assert none is None and torch.equal(l3, l0) and torch.equal(p3, p0)
    l4, _, none = run_msssim(a, b, dts, scales, pitch=8, grad=False, want_scores=False)
    assert none is None and torch.equal(l4, l0)
    # grad_accumulate = 1 on a prefilled da: dtype_da(float(old) + g), g the fp32 gradient of the grad_accumulate = 0 call
    rng = np.random.default_rng(5)
    for dtd in ('f32', 'bf16', 'f16'):
        for dta, dtb in (('f32', 'f32'), ('bf16', 'f32')):
            a, b = reference('smooth', shape, 0.3, scales, dta, dtb)[:2]
            _, g, _ = run_msssim(a, b, (dta, dtb, 'f32'), scales, pitch=8, grad_scale=100.0)
            old = stored(0.01 * rng.uniform(-1, 1, shape), dtd)
            _, got, _ = run_msssim(a, b, (dta, dtb, dtd), scales, pitch=8, grad_scale=100.0, da0=old)
            want = (old.float() + g).to(TD[dtd])
            assert torch.equal(got, want), (dtd, dta, dtb)


def test_deterministic_and_an_image_does_not_depend_on_the_rest_of_the_batch():
    shape, scales = (3, 75, 53, 3), 2
    dts = ('f32', 'f32', 'f32')
    a, b = reference('noise', shape, 0.3, scales, 'f32', 'f32')[:2]
    l0, d0, p0 = run_msssim(a, b, dts, scales, pitch=8)
    l1, d1, p1 = run_msssim(a, b, dts, scales, pitch=8)
    assert torch.equal(l0, l1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and torch.equal(p0, p1)
    for i in range(3):
        _, di, pi = run_msssim(a[i:i + 1].contiguous(), b[i:i + 1].contiguous(), dts, scales, pitch=8)
        want = di[0].double().cpu().numpy() / 3.0
        got = d0[i].double().cpu().numpy()
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got - want) <= ulp), (i, float((np.abs(got - want) / ulp).max()))
        assert torch.equal(pi[0], p0[i])
    a16, b16 = reference('noise', shape, 0.3, scales, 'bf16', 'f32')[:2]
    x = run_msssim(a16, b16, ('bf16', 'f32', 'bf16'), scales, pitch=8)
    y = run_msssim(a16, b16, ('bf16', 'f32', 'bf16'), scales, pitch=8)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int16), y[1].view(torch.int16))


def test_refused_arguments_write_nothing():
    from gan_amd import _lib as L
    lib = L.load()
    shape, scales = (2, 45, 47, 3), 3
    n, h, w, c = shape
    a, b = (t[:2].contiguous() for t in reference('smooth', (3, h, w, c), 0.3, scales, 'f32', 'f32')[:2])
    da = torch.full(shape, SENTINEL, device='cuda:0')
    ws = torch.full((lib.gan_msssim_workspace_bytes(n, h, w, c, scales) // 4,), SENTINEL, device='cuda:0')
    out = torch.full((1,), SENTINEL, device='cuda:0')
    per = torch.full((n,), SENTINEL, device='cuda:0')
    T = lambda t, **kw: L.GanTensor(**{**dict(ptr=t.data_ptr(), n=n, h=h, w=w, c=c, pitch=c), **kw})

    def desc(**kw):
        f = dict(dtype_a=L.F32, dtype_b=L.F32, a=T(a), b=T(b), loss_scale=1.0, loss_accumulate=0, loss_out=out.data_ptr(), grad_scale=1.0,
                 dtype_da=L.F32, da=T(da), workspace=ws.data_ptr(), workspace_bytes=ws.numel() * 4, scale_state=None, scales=scales,
                 power=L.msssim_power(scales), per_image=per.data_ptr(), grad_accumulate=0)
        f.update(kw)
        return L.GanMsssimDesc(**f)
    st = torch.cuda.current_stream().cuda_stream
    cases = [(L.E_ARG, dict(dtype_a=5)), (L.E_ARG, dict(dtype_da=-1)), (L.E_ARG, dict(a=T(a, c=2))), (L.E_ARG, dict(b=T(b, h=h + 1))),
             (L.E_ARG, dict(da=T(da, w=w - 1))), (L.E_ARG, dict(a=T(a, pitch=2))), (L.E_ARG, dict(loss_out=None)),
             (L.E_ARG, dict(workspace=None)), (L.E_ARG, dict(loss_accumulate=2)), (L.E_ARG, dict(grad_accumulate=2)),
             (L.E_ARG, dict(grad_accumulate=-1)), (L.E_ARG, dict(scales=0)), (L.E_ARG, dict(scales=6)),
             (L.E_ARG, dict(power=L.Float5(0.1, -0.2, 0.3, 0, 0))), (L.E_ARG, dict(power=L.Float5(0.1, 0.2, float('nan'), 0, 0))),
             (L.E_ARG, dict(power=L.Float5(float('inf'), 0.2, 0.3, 0, 0))),
             (L.E_SHAPE, dict(scales=4, power=L.msssim_power(4), workspace_bytes=1 << 30)),
             (L.E_SHAPE, dict(a=T(a, h=43), b=T(b, h=43), da=T(da, h=43))), (L.E_SHAPE, dict(a=T(a, w=4097), b=T(b, w=4097), da=T(da, w=4097))),
             (L.E_WORKSPACE, dict(workspace_bytes=ws.numel() * 4 - 4)), (L.E_WORKSPACE, dict(workspace_bytes=0))]
    for code, kw in cases:
        assert lib.gan_msssim(C.byref(desc(**kw)), st) == code, kw
    d = desc()
    d.struct_size -= 4
    assert lib.gan_msssim(C.byref(d), st) == L.E_ARG
    torch.cuda.synchronize()
    for t in (da, ws, out, per):
        assert bool((t == SENTINEL).all())
    assert lib.gan_msssim(C.byref(desc()), st) == 0          # and the good descriptor runs
    torch.cuda.synchronize()
    assert not bool((da == SENTINEL).any()) and float(out[0]) != SENTINEL and not bool((per == SENTINEL).any())


def test_capturable():
    from gan_amd import _lib as L
    from gan_amd.nets import Ctx
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=16)
    lib = L.load()
    shape, scales = (3, 88, 91, 3), 4
    n, h, w, c = shape
    a, b = reference('smooth', shape, 0.3, scales, 'bf16', 'f32')[:2]
    eager_loss, eager_da, eager_per = run_msssim(a, b, ('bf16', 'f32', 'bf16'), scales)
    da = torch.zeros(shape, dtype=torch.bfloat16, device='cuda:0')
    out = torch.zeros(1, device='cuda:0')
    per = torch.zeros(n, device='cuda:0')
    ws = torch.zeros(lib.gan_msssim_workspace_bytes(n, h, w, c, scales) // 4, device='cuda:0')
    d = L.GanMsssimDesc(L.BF16, L.F32, L.GanTensor(a.data_ptr(), n, h, w, c, c), L.GanTensor(b.data_ptr(), n, h, w, c, c), 1.0, 0, out.data_ptr(),
                        1.0, L.BF16, L.GanTensor(da.data_ptr(), n, h, w, c, c), ws.data_ptr(), ws.numel() * 4, None, scales,
                        L.msssim_power(scales), per.data_ptr(), 0)
    torch.cuda.synchronize()
    gr = ctx.capture_graph(lambda: L.check(lib.gan_msssim(C.byref(d), ctx.stream()), "msssim"))
    for _ in range(2):
        da.fill_(float('nan'))
        out.fill_(float('nan'))
        per.fill_(float('nan'))
        ws.fill_(float('nan'))
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager_loss) and torch.equal(da.view(torch.int16), eager_da.view(torch.int16)) and torch.equal(per, eager_per)
