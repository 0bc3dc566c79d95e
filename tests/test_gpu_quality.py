"""gan_image_quality on the GPU against the fp64 reference tests/quality_ref.py.

The reference is evaluated on the STORED values (after the rounding to bf16 / fp16), so the gates do not depend on the dtype:
SSIM within 1e-5 on textured images and within 5e-4 on bright flat / constant ones (what the cancellation in F(u^2) - mx^2 costs a
naive fp32 restatement there: 2.6e-6 and 2.7e-4), exactly 1 for a == b; MAE and MSE to rtol 2e-5 (the project's fp32 op gate); PSNR
within 1e-4 dB, +inf for a == b."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import quality_ref as Q

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
DTYPE_PAIRS = [('f32', 'f32'), ('bf16', 'f32'), ('f16', 'f32'), ('bf16', 'bf16')]
# h, w from {11, 12, 26, 27, 42, 43, 74, 75}: one window, and T + 10 / T + 11 for tile edges T = 16, 32, 64
SHAPES = [(1, 11, 11, 1), (3, 12, 75, 3), (1, 43, 26, 3), (3, 26, 27, 1), (1, 27, 42, 3), (3, 42, 43, 1), (1, 43, 74, 1), (1, 74, 75, 3),
          (3, 75, 12, 1), (1, 11, 74, 3), (3, 75, 75, 1), (1, 12, 12, 3), (1, 26, 11, 1), (3, 43, 43, 3)]
KINDS = ('noise', 'smooth', 'flat', 'const', 'same')
SSIM_GATE = {'noise': 1e-5, 'smooth': 1e-5, 'flat': 5e-4, 'const': 5e-4}


@pytest.fixture(scope='module')
def ctx():
    from gan_amd.nets import Ctx
    return Ctx('cuda:0', 'bf16', workspace_mb=16)


def make_pair(kind, shape, seed):
    """-> (a, b) float64 raw images in [-1, 1]"""
    n, h, w, c = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    ph = rng.uniform(0, 6.28, (n, 1, 1, c))
    wave = lambda k: np.sin(0.21 * yy[None, :, :, None] + ph * k) * np.cos(0.13 * xx[None, :, :, None] - ph)
    if kind == 'noise':
        return rng.uniform(-1, 1, shape), rng.uniform(-1, 1, shape)
    if kind == 'smooth':      # a smooth pattern plus 5 % noise
        base = 0.7 * wave(1.0)
        return base + 0.05 * rng.uniform(-1, 1, shape), 0.9 * base + 0.05 * rng.uniform(-1, 1, shape)
    if kind == 'flat':        # display 0.98 + 0.01 sin: bright, nearly flat
        return 2 * (0.98 + 0.01 * wave(1.0)) - 1, 2 * (0.98 + 0.01 * wave(2.0)) - 1
    if kind == 'const':
        return np.full(shape, -0.7), np.full(shape, 0.8)
    a = rng.uniform(-1, 1, shape)
    return a, a.copy()


def run_quality(ta, dta, tb, dtb, shape, ws=None, out=None, stream=None):
    """Low-level call on GanTensor views -> device tensor [n, 4]."""
    from gan_amd import _lib as L
    lib = L.load()
    n, h, w, c = shape
    dev = torch.device('cuda:0')
    if ws is None:
        ws = torch.full((lib.gan_image_quality_workspace_bytes(n, h, w, c) // 4,), float('nan'), device=dev)
    if out is None:
        out = torch.full((n, 4), float('nan'), device=dev)
    d = L.GanQualityDesc({'f32': L.F32, 'bf16': L.BF16, 'f16': L.F16}[dta], {'f32': L.F32, 'bf16': L.BF16, 'f16': L.F16}[dtb], ta, tb,
                         out.data_ptr(), ws.data_ptr(), ws.numel() * 4)
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    L.check(lib.gan_image_quality(C.byref(d), st), "image_quality")
    return out


def dense(t):
    from gan_amd import _lib as L
    n, h, w, c = t.shape
    return L.GanTensor(t.data_ptr(), n, h, w, c, c)


def stored(a, dt):
    return torch.from_numpy(a).to(TD[dt]).cuda().contiguous()


def check_rows(got, want, kind, what):
    """got: [n, 4] float32 from the device, want: [n, 4] float64 reference.  Prints each figure before it asserts."""
    got = got.double().cpu().numpy()
    e_ssim = np.abs(got[:, 0] - want[:, 0]).max()
    print(f"quality {what} {kind}: ssim err {e_ssim:.3e}", end='')
    if kind == 'same':
        print(f" ssim {got[:, 0].tolist()} psnr {got[:, 1].tolist()}")
        assert np.array_equal(got[:, 0], np.ones(len(got))), (what, got[:, 0])
        assert np.all(np.isposinf(got[:, 1])) and np.array_equal(got[:, 2:], np.zeros((len(got), 2))), (what, got)
        return
    rel = lambda j: (np.abs(got[:, j] - want[:, j]) / np.abs(want[:, j])).max()
    e_psnr = np.abs(got[:, 1] - want[:, 1]).max()
    print(f" psnr err {e_psnr:.3e} dB, mae rel {rel(2):.3e}, mse rel {rel(3):.3e}")
    assert np.isfinite(got).all(), (what, kind)
    assert e_ssim <= SSIM_GATE[kind], (what, kind, e_ssim)
    assert rel(2) <= 2e-5 and rel(3) <= 2e-5, (what, kind, rel(2), rel(3))
    assert e_psnr <= 1e-4, (what, kind, e_psnr)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_matches_fp64_reference(shape):
    for k, kind in enumerate(KINDS):
        a64, b64 = make_pair(kind, shape, 100 + k)
        for dta, dtb in DTYPE_PAIRS:
            a, b = stored(a64, dta), stored(b64, dtb)
            if kind == 'same':      # equal as STORED: b takes a's rounded values (exact: dtb is fp32 or a's own dtype)
                b = a.to(TD[dtb])
            want = Q.quality(a.double().cpu().numpy(), b.double().cpu().numpy())
            got = run_quality(dense(a), dta, dense(b), dtb, shape)
            check_rows(got, want, kind, f"{shape} {dta}/{dtb}")


@pytest.mark.parametrize('shape', [(1, 75, 43, 3), (1, 43, 74, 1), (1, 11, 12, 1)], ids=lambda s: 'x'.join(map(str, s)))
def test_every_pixel_and_map_position_counts_exactly_once(shape):
    """One impulse, placed in turn at each corner, on each edge, inside, and on both sides of every tile seam."""
    n, h, w, c = shape
    a64, _ = make_pair('smooth', shape, 7)
    a = stored(a64, 'f32')
    ys = sorted({0, h - 1, h // 2, *(y for y in (15, 16, 31, 32, 41, 42, 63, 64, h - 11, h - 10) if 0 <= y < h)})
    xs = sorted({0, w - 1, w // 2, *(x for x in (15, 16, 31, 32, 41, 42, 63, 64, w - 11, w - 10) if 0 <= x < w)})
    worst = 0.0
    for y in ys:
        for x in xs:
            b = a.clone()
            ch = (y + x) % c
            b[0, y, x, ch] += 0.375
            d = float(b[0, y, x, ch].double() - a[0, y, x, ch].double())
            got = run_quality(dense(a), 'f32', dense(b), 'f32', shape).double().cpu().numpy()
            want = Q.quality(a.double().cpu().numpy(), b.double().cpu().numpy())
            mae = abs(d) / 2 / (h * w * c)
            worst = max(worst, abs(got[0, 0] - want[0, 0]))
            assert abs(got[0, 2] - mae) <= 1e-6 * mae, (y, x, got[0, 2], mae)
            assert abs(got[0, 3] - (d / 2) ** 2 / (h * w * c)) <= 2e-5 * want[0, 3], (y, x)
            assert abs(got[0, 0] - want[0, 0]) <= 1e-5, (y, x, got[0, 0], want[0, 0])
    print(f"impulse {shape}: {len(ys) * len(xs)} positions, worst ssim err {worst:.3e}")


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_pad_channels_and_guard_regions_may_hold_nan(dt):
    """pitch 8 with NaN in every pad channel and NaN guards around the buffer; and a channel-slice view at a non-zero channel
    offset of a 16-channel buffer: finite, and bit-equal to clean dense operands."""
    from gan_amd import _lib as L
    for shape in ((3, 43, 26, 3), (1, 27, 42, 1)):
        n, h, w, c = shape
        a64, b64 = make_pair('smooth', shape, 11)
        a, b = stored(a64, dt), stored(b64, 'f32')
        clean = run_quality(dense(a), dt, dense(b), 'f32', shape)
        for pitch, c0 in ((8, 0), (16, 5)):
            guard = 4096
            flat = torch.full((2 * guard + n * h * w * pitch,), float('nan'), dtype=TD[dt], device='cuda:0')
            body = flat[guard:guard + n * h * w * pitch].view(n, h, w, pitch)
            body[..., c0:c0 + c] = a
            view = L.GanTensor(body.data_ptr() + c0 * flat.element_size(), n, h, w, c, pitch)
            fb = torch.full((2 * guard + n * h * w * pitch,), float('nan'), dtype=torch.float32, device='cuda:0')
            bbody = fb[guard:guard + n * h * w * pitch].view(n, h, w, pitch)
            bbody[..., c0:c0 + c] = b
            bview = L.GanTensor(bbody.data_ptr() + c0 * 4, n, h, w, c, pitch)
            got = run_quality(view, dt, bview, 'f32', shape)
            assert torch.isfinite(got).all() and torch.equal(got, clean), (shape, pitch, c0)
            got = run_quality(view, dt, dense(b), 'f32', shape)          # padded prediction against the dense target: the product's case
            assert torch.equal(got, clean), (shape, pitch, c0)


def test_deterministic_and_independent_of_the_rest_of_the_batch():
    shape = (3, 75, 43, 3)
    a64, b64 = make_pair('noise', shape, 21)
    a, b = stored(a64, 'bf16'), stored(b64, 'f32')
    first = run_quality(dense(a), 'bf16', dense(b), 'f32', shape)
    again = run_quality(dense(a), 'bf16', dense(b), 'f32', shape)
    assert torch.equal(first, again)
    for i in range(3):
        ai, bi = a[i:i + 1].contiguous(), b[i:i + 1].contiguous()
        alone = run_quality(dense(ai), 'bf16', dense(bi), 'f32', (1, 75, 43, 3))
        assert torch.equal(alone[0], first[i]), i


def test_capturable(ctx):
    from gan_amd.quality import image_quality
    shape = (3, 43, 74, 3)
    a64, b64 = make_pair('smooth', shape, 31)
    a, b = stored(a64, 'bf16'), stored(b64, 'f32')
    eager = image_quality(ctx, a, b).clone()                # (also allocates the cached workspace before the capture)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    gr = ctx.capture_graph(lambda: image_quality(ctx, a, b, out=out))
    for _ in range(2):
        out.fill_(float('nan'))
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_product_shapes(ctx):
    """256^2 batch 16 c 1 with the bf16 prediction read through the generator's 8-channel-padded output layout (a nets.Buf) against
    the dense fp32 target; 512^2 batch 2 c 3 in fp32."""
    from gan_amd.nets import Buf
    from gan_amd.quality import image_quality
    shape = (16, 256, 256, 1)
    a64, b64 = make_pair('smooth', shape, 41)
    buf = Buf(ctx, 16, 256, 256, 8)
    buf.t.fill_(float('nan'))
    buf.t[..., :1] = torch.from_numpy(a64).to(torch.bfloat16).cuda()
    b = stored(b64, 'f32')
    got = image_quality(ctx, buf, b)
    want = Q.quality(buf.t[..., :1].double().cpu().numpy(), b.double().cpu().numpy())
    check_rows(got, want, 'smooth', 'product 256 b16 bf16/f32')
    assert torch.equal(got, image_quality(ctx, buf.view(0, 1), b))          # the GanTensor view form
    shape = (2, 512, 512, 3)
    a64, b64 = make_pair('noise', shape, 42)
    a, b = stored(a64, 'f32'), stored(b64, 'f32')
    check_rows(image_quality(ctx, a, b), Q.quality(a64.astype(np.float32).astype(np.float64), b64.astype(np.float32).astype(np.float64)),
               'noise', 'product 512 b2 f32/f32')


def _p2p(tmp, extra=()):
    from gan_amd import pix2pix
    return pix2pix.Pix2Pix(vars(pix2pix.parse_opt(['--data', str(tmp), '--output', str(tmp), '--train', '--epochs', '1', '--batch-size', '2',
                                                   '--dtype', 'f32', *extra])))


def test_pix2pix_evaluate_matches_reference_and_leaves_training_untouched(tmp_path):
    rng = np.random.default_rng(5)
    xs = torch.from_numpy(rng.uniform(-1, 1, (4, 256, 256, 1)).astype(np.float32)).cuda()
    ys = torch.from_numpy(rng.uniform(-1, 1, (4, 256, 256, 1)).astype(np.float32)).cuda()
    ds = [(xs[:2], ys[:2]), (xs[2:], ys[2:])]
    m = _p2p(tmp_path)
    l0 = torch.stack(m.train_step(xs[:2], ys[:2])).clone()
    got = m.evaluate(ds)
    l1 = torch.stack(m.train_step(xs[2:], ys[2:])).clone()
    assert list(got) == ['SSIM', 'PSNR', 'MAE', 'MSE'] and all(len(v) == 4 for v in got.values())
    # after the second step the weights differ: take the predictions from a twin that stops after the first
    twin = _p2p(tmp_path)
    t0 = torch.stack(twin.train_step(xs[:2], ys[:2])).clone()
    twin.generator.fold()
    pred = torch.cat([twin.generator.infer(x, fold=False) for x, _ in ds]).double().cpu().numpy()
    want = Q.quality(pred, ys.double().cpu().numpy())
    rows = torch.tensor([got[k] for k in ('SSIM', 'PSNR', 'MAE', 'MSE')], dtype=torch.float64).T
    check_rows(rows, want, 'noise', 'Pix2Pix.evaluate')
    t1 = torch.stack(twin.train_step(xs[2:], ys[2:])).clone()
    assert torch.equal(l0, t0) and torch.equal(l1, t1)          # two train steps with the evaluation between them = without it
    # training=True: the reference's batch-1 call; same layout, SSIM in range
    tr = m.evaluate(ds, training=True)
    assert all(len(v) == 4 for v in tr.values()) and all(-1 <= s <= 1 for s in tr['SSIM'])


def _run_dir(out):
    return os.path.join(out, sorted(os.listdir(out))[0])


def test_pix2pix_cli_quality_metrics(tmp_path):
    from PIL import Image
    from gan_amd import pix2pix
    rng = np.random.default_rng(0)
    data = str(tmp_path / 'data')
    os.makedirs(data)
    for i in range(10):
        Image.fromarray(rng.integers(0, 256, (256, 512), dtype=np.uint8), 'L').save(os.path.join(data, f"p{i}.png"))
    base = ['--data', data, '--train', '--epochs', '1', '--batch-size', '2', '--logging', 'false', '--seed', '7']
    strict = lambda p: json.loads(open(p).read(), parse_constant=lambda s: pytest.fail(f"not strict JSON: {s} in {p}"))
    logs = {}
    for flag in ('true', 'false'):
        out = str(tmp_path / f'out_{flag}')
        pix2pix.main(pix2pix.parse_opt(base + ['--output', out, '--quality-metrics', flag]))
        logs[flag] = os.path.join(_run_dir(out), 'logs')
    for name in ('train_metrics.json', 'val_metrics.json'):
        assert strict(os.path.join(logs['true'], name)) == strict(os.path.join(logs['false'], name)), name
    for name in ('val_quality.json', 'test_quality.json'):
        assert os.path.exists(os.path.join(logs['true'], name)) and not os.path.exists(os.path.join(logs['false'], name)), name
    val = strict(os.path.join(logs['true'], 'val_quality.json'))
    assert sorted(val) == ['MAE', 'PSNR', 'SSIM'] and all(len(v) == 1 for v in val.values()) and -1 <= val['SSIM'][0] <= 1
    test = strict(os.path.join(logs['true'], 'test_quality.json'))
    assert sorted(test) == ['mean', 'per_image'] and all(len(test['per_image'][k]) == 5 for k in ('SSIM', 'PSNR', 'MAE', 'MSE'))
    assert all(-1 <= s <= 1 for s in test['per_image']['SSIM']) and abs(test['mean']['SSIM'] - np.mean(test['per_image']['SSIM'])) < 1e-9
    ck = os.path.join(os.path.dirname(logs['true']), 'training_checkpoints')
    for mode in ('true', 'false'):
        out = str(tmp_path / f'pred_{mode}')
        pix2pix.main(pix2pix.parse_opt(['--data', data, '--predict', '--weights', ck, '--logging', 'false', '--batch-size', '4', '--output', out,
                                        '--quality-metrics', 'true', '--predict-training', mode]))
        pm = strict(os.path.join(_run_dir(out), 'logs', 'prediction_metrics.json'))
        assert all(len(pm['per_image'][k]) == 10 for k in ('SSIM', 'PSNR', 'MAE', 'MSE')) and all(-1 <= s <= 1 for s in pm['per_image']['SSIM'])
