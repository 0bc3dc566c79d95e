"""CycleGAN cycle-consistency metrics and native-size prediction on the GPU: gan_tile_gather bit-exact against
torch slices on the same device; float-source infer_tiled; the cycle at the source resolution against the fp64 restatement
(tests/tile_ref.py, tests/quality_ref.py); cycle_quality on img_size batches; no side effects on training; the CLI.

Gates, taken from the tests of the parts: a blended image max |err| <= 1e-5 + one ulp of the storage type at 1.0
(tests/test_gpu_tiles.py: the blend's fp32 arithmetic plus the typed read; the network sees the same bits on both sides); metric rows
SSIM 1e-5, PSNR 1e-4 dB, MAE 2e-5 relative (tests/test_gpu_quality.py, textured images), on the STORED images."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import quality_ref as QR
from tests import tile_ref as R

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
BITS = {'f32': torch.int32, 'bf16': torch.int16, 'f16': torch.int16}
SOURCES = [(16, 16), (17, 31), (29, 40)]          # one tile; 2 x 2 with pulled-back last tiles; 3 x 3 (V = 4)
S = 16
GATE = 1e-5
EPS = {'f32': 2.0 ** -23, 'bf16': 2.0 ** -7}          # one ulp of the storage type at 1.0
PAIRS = [('f32', 'bf16'), ('f32', 'f16'), ('f32', 'f32'), ('bf16', 'bf16')]


@pytest.fixture(scope='module')
def ctx():
    from gan_amd.nets import Ctx
    return Ctx('cuda:0', 'bf16', workspace_mb=16)


def code(dt):
    from gan_amd import _lib as L
    return {'f32': L.F32, 'bf16': L.BF16, 'f16': L.F16}[dt]


def view(t, c, n0=0, n=None):
    """GanTensor over the first c channels of tiles [n0, n0 + n) of a [nt, S, S, pitch] tensor."""
    from gan_amd import _lib as L
    nt, s, _, pitch = t.shape
    n = nt - n0 if n is None else n
    return L.GanTensor(t.data_ptr() + n0 * s * s * pitch * t.element_size(), n, s, s, c, pitch)


def nan_tiles(n, pitch, dt):
    return torch.full((n, S, S, pitch), float('nan'), dtype=TD[dt], device='cuda')


def source(h, w, c, sdt, seed, right_half=False):
    """-> (float device tensor [h, wfull, c] of values that need the rounding - plus an inf, a NaN and a -0.0 -, col0)."""
    rng = np.random.default_rng(seed)
    wfull, col0 = (2 * w + 3, w + 1) if right_half else (w, 0)
    a = rng.uniform(-1, 1, (h, wfull, c)).astype(np.float32)
    a[0, col0, 0], a[h - 1, col0 + w - 1, c - 1], a[h // 2, col0 + w // 2, 0] = np.inf, np.nan, -0.0
    return torch.from_numpy(a).to(TD[sdt]).cuda().contiguous(), col0


def gather(ctx, src, got, c, ddt, h, w, V, col0, t0=0, n=None, n0=None):
    from gan_amd.tiling import gather_tiles_f
    n = got.shape[0] - t0 if n is None else n
    gather_tiles_f(ctx, src, view(got, c, t0 if n0 is None else n0, n), h=h, w=w, tile=S, overlap=V, t0=t0, n=n, col0=col0, dtype=code(ddt))


def same_bits(a, b, dt):
    return torch.equal(a.contiguous().view(BITS[dt]), b.contiguous().view(BITS[dt]))


# ---------------------------------------------------------------------------------------------------------------------
# gan_tile_gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('sdt,ddt', PAIRS)
def test_gather_is_bit_exact_against_torch_slices(ctx, sdt, ddt, c):
    from gan_amd.tiling import cut_tiles, tile_grid
    for k, (h, w) in enumerate(SOURCES):
        for V in (0, 4, 8):
            for pitch in (8, c):
                for right in (False, True):
                    src, col0 = source(h, w, c, sdt, 100 * k + V + pitch, right)
                    nt = int(np.prod(tile_grid(h, w, S, V)))
                    want = nan_tiles(nt, pitch, ddt)
                    want[..., :c] = cut_tiles(src, S, V, col0, w).to(TD[ddt])        # src[oy:oy+S, ox:ox+S, :c].to(dtype) per tile
                    got = nan_tiles(nt, pitch, ddt)
                    gather(ctx, src, got, c, ddt, h, w, V, col0)
                    what = (h, w, V, pitch, right)
                    assert same_bits(got, want, ddt), what                          # the whole destination: pad slots stay NaN
                    if nt > 2:      # t0 > 0: a sub-range lands at the start of its own view and touches nothing else
                        sub = nan_tiles(nt, pitch, ddt)
                        gather(ctx, src, sub, c, ddt, h, w, V, col0, t0=1, n=nt - 2)
                        assert same_bits(sub[1:nt - 1], got[1:nt - 1], ddt), what
                        assert bool(torch.isnan(sub[0]).all()) and bool(torch.isnan(sub[nt - 1]).all()), what
                    for step in (1, 2):     # chunks of 1 and 2 tiles give the bits of one launch
                        parts = nan_tiles(nt, pitch, ddt)
                        for t0 in range(0, nt, step):
                            gather(ctx, src, parts, c, ddt, h, w, V, col0, t0=t0, n=min(step, nt - t0))
                        assert same_bits(parts, got, ddt), (what, step)


def test_gather_replays_from_a_captured_graph(ctx):
    from gan_amd.tiling import tile_grid
    h, w, V, c = 29, 40, 4, 3
    src, col0 = source(h, w, c, 'f32', 77, right_half=True)
    nt = int(np.prod(tile_grid(h, w, S, V)))
    t = nan_tiles(nt, 8, 'bf16')
    run = lambda: (gather(ctx, src, t, c, 'bf16', h, w, V, col0, t0=0, n=5), gather(ctx, src, t, c, 'bf16', h, w, V, col0, t0=5, n=nt - 5))
    run()
    torch.cuda.synchronize()
    eager = t.clone()
    gr = ctx.capture_graph(run)
    for _ in range(2):
        t.fill_(float('nan'))
        gr.replay()
        torch.cuda.synchronize()
        assert same_bits(t, eager, 'bf16')


def test_bad_geometry_is_an_error_and_launches_nothing(ctx):
    from gan_amd import _lib as L
    from gan_amd.tiling import gather_tiles_f
    src, _ = source(29, 40, 1, 'f32', 3)
    t = nan_tiles(9, 8, 'bf16')
    ok = dict(h=29, w=40, tile=S, overlap=4, t0=0, n=9, col0=0)
    for bad in (dict(overlap=9), dict(h=15), dict(w=4097), dict(t0=1), dict(n=4), dict(col0=1), dict(h=30), dict(tile=24)):
        with pytest.raises(L.GanAmdError):
            gather_tiles_f(ctx, src, view(t, 1), **{**ok, **bad})
    with pytest.raises(L.GanAmdError):          # bf16 -> f16: a 16-bit source is copied, never converted
        gather_tiles_f(ctx, src.bfloat16(), view(t, 1), **ok, dtype=L.F16)
    torch.cuda.synchronize()
    assert bool(torch.isnan(t).all())


# ---------------------------------------------------------------------------------------------------------------------
# the real networks: CycleGAN generators after one train step, C = 1, S = 256
# ---------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _new(dt, extra=()):
    from gan_amd import cycle_gan
    from gan_amd.runner import config_of
    return cycle_gan.CycleGAN(config_of(cycle_gan.parse_opt(['--input-images', 'x', '--target-images', 'y', '--output', 'o', '--train',
                                                             '--epochs', '1', '--dtype', dt, '--seed', '3', *extra])))


def _xy(n, seed):
    rng = np.random.default_rng(seed)
    return tuple(torch.from_numpy(rng.uniform(-1, 1, (n, 256, 256, 1)).astype(np.float32)).cuda() for _ in range(2))


def trained(dt):
    if dt not in _MODELS:
        m = _new(dt)
        m.train_step(*_xy(1, 9), True)
        _MODELS[dt] = m
    return _MODELS[dt]


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_float_source_of_one_tile_is_infer(dt):
    from gan_amd.tiling import infer_tiled
    g = trained(dt).generator_g
    x = _xy(1, 1)[0]
    want = g.infer(x)[0]
    assert torch.equal(infer_tiled(g, x[0].contiguous(), tile=256, overlap=64), want)          # a single tile: the weight is exactly 1
    wide = torch.cat([x[0].flip(1), x[0]], dim=1).contiguous()                                 # the same image as a column window
    assert torch.equal(infer_tiled(g, wide, tile=256, overlap=0, col0=256), want)
    if dt == 'bf16':        # a source in the storage type: the bits are copied
        assert torch.equal(infer_tiled(g, x[0].bfloat16().contiguous(), tile=256, overlap=64), g.infer(x.bfloat16().float())[0])
    for bad in (x[0].double(), x[0].half(), x[0].long()):
        with pytest.raises(ValueError):
            infer_tiled(g, bad.contiguous(), tile=256, overlap=64)
    with pytest.raises(ValueError):         # the method keeps to decoded files
        g.infer_tiled(x[0].contiguous(), tile=256, overlap=64)


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_uint8_source_keeps_its_bits(dt):
    """The uint8 path is untouched, and lut[src] through the float gather gives its bits: the table holds fp32 numbers, and both
    gathers round an fp32 value to the storage type with the same store.  bf16: so does the image of the rounded table values."""
    from gan_amd.tiling import infer_tiled, normalize_lut
    m = trained(dt)
    g = m.generator_g
    src = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (256, 320, 1), dtype=np.uint8)).cuda()
    via_u8 = infer_tiled(g, src, tile=256, overlap=64)
    assert torch.equal(via_u8, g.infer_tiled(src, tile=256, overlap=64))
    real = normalize_lut(m.ctx)[src.long()]
    assert torch.equal(infer_tiled(g, real, tile=256, overlap=64), via_u8)          # (fp32 -> bf16 rounds as the table path does)
    if dt == 'bf16':
        assert torch.equal(infer_tiled(g, real.bfloat16(), tile=256, overlap=64), via_u8)


def _blended(model, image64, h, w, V, chunk):
    """fp64 restatement of one tiled pass: numpy-cut tiles through `infer` in the same batch composition, tile_ref blend."""
    tiles = R.cut(image64.astype(np.float32), 256, V)
    out = np.concatenate([model.infer(tiles[t0:t0 + chunk], fold=False).double().cpu().numpy() for t0 in range(0, len(tiles), chunk)])
    return R.blend(out, h, w, 256, V)


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('h,w,batch', [(256, 256, None), (256, 320, None), (256, 320, 1), (300, 300, None), (300, 300, 3)])
def test_cycle_at_the_source_resolution_matches_the_fp64_restatement(dt, h, w, batch):
    from gan_amd import cycle_quality as Q
    from gan_amd import data as D
    from gan_amd.tiling import tile_grid
    m = trained(dt)
    V = 64
    src = np.random.default_rng(h + w).integers(0, 256, (h, w, 1), dtype=np.uint8)
    real = D.normalize(src.astype(np.float32)).astype(np.float64)
    nt = int(np.prod(tile_grid(h, w, 256, V)))
    chunk = nt if batch is None else batch
    m._fold()
    rows, fake, cycled = Q.cycle_quality_tiled(m, torch.from_numpy(src).cuda(), tile=256, overlap=V, batch=batch)
    assert fake.shape == cycled.shape == (h, w, 1) and rows.shape == (1, 3)
    fake64, cycled64 = fake.double().cpu().numpy(), cycled.double().cpu().numpy()
    gate = GATE + EPS[dt]
    # first pass
    fake_ref = _blended(m.generator_g, real, h, w, V, chunk)
    e1 = float(np.abs(fake64 - fake_ref).max())
    # second pass from the image the device holds: the network sees the same bits on both sides, only the blend differs
    e2 = float(np.abs(cycled64 - _blended(m.generator_f, fake64, h, w, V, chunk)).max())
    # ... and from the reference's own first pass: the whole chain
    chain = _blended(m.generator_f, fake_ref, h, w, V, chunk)
    e3 = float(np.abs(cycled64 - chain).max())
    print(f"cycle {dt} {h}x{w} batch={batch}: fake {e1:.3e}, cycled from the stored fake {e2:.3e}, whole chain {e3:.3e} (gate {gate:.3e})")
    want = QR.quality(cycled64[None], real[None])
    got = rows.double().cpu().numpy()
    e_ssim, e_psnr, e_mae = abs(got[0, 0] - want[0, 0]), abs(got[0, 1] - want[0, 1]), abs(got[0, 2] - want[0, 2]) / want[0, 2]
    print(f"    rows {got[0].tolist()}: ssim err {e_ssim:.3e}, psnr err {e_psnr:.3e} dB, mae rel {e_mae:.3e}")
    assert np.isfinite(fake64).all() and np.isfinite(cycled64).all() and np.isfinite(got).all()
    assert e1 <= gate and e2 <= gate and e3 <= gate, (e1, e2, e3)
    assert e_ssim <= 1e-5 and e_psnr <= 1e-4 and e_mae <= 2e-5, (e_ssim, e_psnr, e_mae)


def _ref_rows(m, x, y):
    """-> [B, 12] fp64: quality_ref on the stored predictions of the same batch composition; the second generator reads the first
    one's typed output (its stored values go through `infer` unchanged)."""
    G, F = m.generator_g, m.generator_f
    cols = []
    for a, b, z in ((G, F, x), (F, G, y)):
        z64 = z.double().cpu().numpy()
        mid = a.infer(z, fold=False)
        cols.append(QR.quality(b.infer(mid, fold=False).double().cpu().numpy(), z64)[:, :3])
        cols.append(QR.quality(b.infer(z, fold=False).double().cpu().numpy(), z64)[:, :3])
    return np.concatenate(cols, axis=1)


def _distance(a, b):
    """Rows [.., 12] -> (SSIM abs, PSNR abs in dB, MAE relative to b): the largest over the four groups and the images."""
    a, b = a.reshape(-1, 4, 3), b.reshape(-1, 4, 3)
    return (float(np.abs(a[..., 0] - b[..., 0]).max()), float(np.abs(a[..., 1] - b[..., 1]).max()),
            float((np.abs(a[..., 2] - b[..., 2]) / np.abs(b[..., 2])).max()))


def _check_rows(want, got, what):
    """got [B, 12] against the fp64 reference of its own batch composition, at the gates of gan_image_quality."""
    e = _distance(got.double().cpu().numpy(), want)
    print(f"cycle_quality {what}: ssim err {e[0]:.3e}, psnr err {e[1]:.3e} dB, mae rel {e[2]:.3e}")
    assert e[0] <= 1e-5 and e[1] <= 1e-4 and e[2] <= 2e-5, (what, e)


# An image alone and inside a batch of 3: the convolutions pick their plan by the batch, so a stored prediction moves in its last
# bits with the batch size, and with it the row.  How far is a property of the forwards, not of
# cycle_quality: the fp64 reference moves by REF_ACROSS between the predictions `infer` stores at batch 1 and at batch 3 (measured
# on these inputs, the largest over the three images and four groups; SSIM, PSNR in dB, MAE relative).  The rows are gated at twice
# that, as the issue has the bf16 image gate made, plus one ulp of the fp32 number a row holds: two roundings of half an ulp each
# (at PSNR 10.5 dB that ulp, 9.5e-7, is more than the whole fp32 move).
REF_ACROSS = {'bf16': (6.633e-5, 2.935e-4, 4.282e-5), 'f32': (1.355e-8, 4.068e-8, 5.152e-9)}


def _across_gate(dt, rows):
    r = np.abs(rows.double().cpu().numpy()).reshape(-1, 4, 3)
    ulp = (float(np.spacing(np.float32(r[..., 0].max()))), float(np.spacing(np.float32(r[..., 1].max()))), 2.0 ** -23)
    return tuple(2 * ref + u for ref, u in zip(REF_ACROSS[dt], ulp))


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_cycle_quality_rows_are_their_own_images(dt):
    """Batches 1 and 3 match per-image calls row for row.  Each batch size is held against the reference on the predictions its
    forwards store, at the gates of gan_image_quality; an image's row alone is held against its row in the batch at twice the
    reference's own move between the two batch sizes plus an ulp of the row (_across_gate); and with the batch size fixed - the same plans - a row is its image's bit for
    bit: wherever the image stands in the batch, whatever the other images are."""
    from gan_amd import cycle_quality as Q
    m = trained(dt)
    x, y = _xy(3, 21)
    m._fold()
    both = Q.cycle_quality(m, x, y).clone()
    assert both.shape == (3, 12) and bool(torch.isfinite(both).all())
    assert torch.equal(Q.cycle_quality(m, x), both[:, :6]) and torch.equal(Q.cycle_quality(m, x, y), both)
    ref3 = _ref_rows(m, x, y)
    _check_rows(ref3, both, f'{dt} batch 3')
    gate = _across_gate(dt, both)
    for i in range(3):
        one = Q.cycle_quality(m, x[i:i + 1], y[i:i + 1]).clone()
        ref1 = _ref_rows(m, x[i:i + 1], y[i:i + 1])
        _check_rows(ref1, one, f'{dt} image {i}')
        moved = _distance(one.double().cpu().numpy(), both[i:i + 1].double().cpu().numpy())
        ref_moved = _distance(ref1, ref3[i:i + 1])
        print(f"    {dt} image {i} alone against its row in the batch: ssim {moved[0]:.3e}, psnr {moved[1]:.3e} dB, mae rel {moved[2]:.3e}"
              f" (the reference moves {ref_moved[0]:.3e}, {ref_moved[1]:.3e}, {ref_moved[2]:.3e}; gate {gate})")
        assert all(d <= g for d, g in zip(moved, gate)), (i, moved, gate)
    order = [2, 0, 1]
    assert torch.equal(Q.cycle_quality(m, x[order].contiguous(), y[order].contiguous()), both[order])
    (x2, y2), xr, yr = _xy(3, 22), x.clone(), y.clone()
    xr[1:], yr[1:] = x2[1:], y2[1:]
    others = Q.cycle_quality(m, xr, yr)
    assert torch.equal(others[0], both[0]) and not torch.equal(others[1:], both[1:])


class _Wire:
    """An eval call whose output is its input: one buffer."""

    def __init__(self, ctx, B, size):
        from gan_amd.nets import Buf
        self.ctx, self.C = ctx, 1
        self.xin = Buf(ctx, B, size, size, 8)

    def set_input(self, x):
        import ctypes as C
        from gan_amd import _lib as L
        v = self.xin.view(0, 1)
        L.check(self.ctx.lib.gan_pack(self.ctx.dt, x.data_ptr(), C.byref(v), self.ctx.stream()), "pack")

    def infer(self, fold=True):
        pass

    def out_view(self, n0=0, n=None):
        return self.xin.view(0, 1, n0, n)


def test_identity_generators_give_exactly_one_and_infinity():
    """F = G^-1 cannot be built from trained weights; a pair of wires can: the cycle and the identity map then hand x itself to
    gan_image_quality as the prediction, through the same copies - SSIM exactly 1, PSNR +inf, MAE 0 (its a == b path)."""
    from gan_amd import cycle_quality as Q
    ctx = trained('f32').ctx
    def wire():
        calls = {}
        return SimpleNamespace(eval_call=lambda B, size: calls.setdefault((B, size), _Wire(ctx, B, size)))
    model = SimpleNamespace(ctx=ctx, generator_g=wire(), generator_f=wire())
    x, y = _xy(2, 5)
    rows = Q.cycle_quality(model, x, y).cpu().numpy()
    assert rows.shape == (2, 12)
    for g in range(4):
        assert np.array_equal(rows[:, 3 * g], np.ones(2)) and np.all(np.isposinf(rows[:, 3 * g + 1])), (g, rows)
        assert np.array_equal(rows[:, 3 * g + 2], np.zeros(2)), (g, rows)


def test_evaluate_leaves_training_untouched():
    from gan_amd import cycle_quality as Q
    (x0, y0), (x1, y1) = _xy(1, 31), _xy(1, 32)
    m, twin = _new('f32'), _new('f32')
    masters = lambda g: [n.net.params.master.clone() for n in g.networks()]
    l0 = torch.stack(m.train_step(x0, y0)).clone()
    got = m.evaluate((b for b in [(x0,), (x1,)]), (b for b in [(y0,), (y1,)]))          # (generators: the zip closes its iterators)
    only_x = m.evaluate([(x0,), (x1,)])
    l1 = torch.stack(m.train_step(x1, y1)).clone()
    t0 = torch.stack(twin.train_step(x0, y0)).clone()
    t1 = torch.stack(twin.train_step(x1, y1)).clone()
    assert torch.equal(l0, t0) and torch.equal(l1, t1)          # two train steps with the evaluations between them = without them
    assert all(torch.equal(a, b) for a, b in zip(masters(m), masters(twin)))
    assert tuple(got) == Q.keys() and all(len(v) == 2 for v in got.values())
    assert tuple(only_x) == Q.keys(Q.GROUPS_X) and all(only_x[k] == got[k] for k in only_x)          # X alone, the same batches: the same bits
    assert all(-1 <= s <= 1 for k in got if k.endswith('ssim') for s in got[k])


def _pngs(folder, n, shape, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(folder)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8), 'L').save(os.path.join(folder, f"p{i}.png"))
    return [os.path.join(folder, f"p{i}.png") for i in range(n)]


def test_predict_at_img_size_with_metrics_plots_the_plain_prediction(tmp_path, monkeypatch):
    """--predict --predict-training false --quality-metrics true at img_size: the plotted prediction is read back from generator_g's
    eval call after generator_f has run twice behind it.  It is generator_g.infer of the same batch, bit for bit, and the metrics
    are cycle_quality's rows of that batch: cycle_x_* and identity_x_*."""
    from gan_amd import cycle_gan
    from gan_amd import cycle_quality as Q
    from gan_amd import data as D
    m = trained('bf16')
    for k, v in (('predict_training', 'false'), ('quality_metrics', 'true'), ('predict_resolution', 'resized'), ('batch_size', 2)):
        monkeypatch.setitem(m.config, k, v)
    files = _pngs(str(tmp_path / 'p'), 3, (64, 64), 4)          # batches of 2 and 1
    plotted = []
    monkeypatch.setattr(cycle_gan, 'save_panels', lambda path, panels, gray: plotted.append([np.array(img) for _, img in panels]))
    got = m.predict(D.Batches(files, m.process_images_pred, 1, None), str(tmp_path / 'out'))
    assert tuple(got) == Q.keys(Q.GROUPS_X) and all(len(v) == 3 for v in got.values())
    xs = np.stack([m.process_images_pred(f)[0] for f in files])
    assert len(plotted) == 3
    for lo, hi in ((0, 2), (2, 3)):
        want = m.generator_g.infer(xs[lo:hi], fold=False).cpu().numpy()
        rows = Q.cycle_quality(m, xs[lo:hi]).cpu().numpy()
        for k in range(lo, hi):
            assert np.array_equal(plotted[k][0], xs[k]) and np.array_equal(plotted[k][1], want[k - lo]), k
            assert [got[name][k] for name in got] == rows[k - lo].tolist(), k


# ---------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------
def _run_dir(out):
    return os.path.join(out, sorted(os.listdir(out))[0])


def _strict(p):
    return json.loads(open(p).read(), parse_constant=lambda s: pytest.fail(f"not strict JSON: {s} in {p}"))


def test_evaluate_does_not_move_the_orders_of_later_epochs(tmp_path):
    """The validation sets are shuffled and count their passes; the extra pass of --quality-metrics is not to change the pairs the
    later epochs' validation passes see (val_metrics.json is that of a run without the flag)."""
    from gan_amd import data as D
    m = trained('bf16')
    fx, fy = _pngs(str(tmp_path / 'x'), 5, (64, 64), 0), _pngs(str(tmp_path / 'y'), 4, (64, 64), 1)
    new = lambda files, seed: D.Batches(files, m.process_images_pred, 2, m.ctx.device, shuffle_seed=seed)
    seq = lambda ds: torch.cat([b for (b,) in ds])
    twin_x, twin_y = new(fx, 5), new(fy, 6)
    want = [(seq(twin_x), seq(twin_y)) for _ in range(3)]
    assert not torch.equal(want[1][0], want[2][0]) and not torch.equal(want[1][1], want[2][1])
    ds_x, ds_y = new(fx, 5), new(fy, 6)
    for k in range(3):          # three epochs' validation passes with evaluations between them, as fit() makes them
        assert torch.equal(seq(ds_x), want[k][0]) and torch.equal(seq(ds_y), want[k][1]), k
        got = m.evaluate(ds_x, ds_y)
        assert all(len(v) == 4 for v in got.values())          # the zip of 5 and 4 images in batches of 2
        m.evaluate(ds_x)


def test_cli_ema_twins_and_prediction_on_both_averages(tmp_path, monkeypatch):
    """--ema-decay with --quality-metrics writes the _ema twins.  --predict-weights ema puts BOTH generators on their averages, the
    pair that was averaged together: identity_x_* is F(x) against x, made by generator_f alone, and differs from the raw weights'."""
    from gan_amd import cycle_gan
    from gan_amd import cycle_quality as Q
    from gan_amd import runner
    dx, dy, dp = str(tmp_path / 'x'), str(tmp_path / 'y'), str(tmp_path / 'p')
    _pngs(dx, 7, (64, 64), 0), _pngs(dy, 5, (64, 64), 1), _pngs(dp, 3, (64, 64), 2)
    monkeypatch.setattr(cycle_gan, 'save_panels', lambda *a, **k: None)          # (figures are not what this test is about)
    monkeypatch.setattr(runner, 'plot_loss_curves', lambda *a, **k: None)
    out = str(tmp_path / 'out')
    cycle_gan.main(cycle_gan.parse_opt(['--input-images', dx, '--target-images', dy, '--train', '--epochs', '1', '--batch-size', '1',
                                        '--logging', 'false', '--seed', '7', '--test-img', '2', '--validation-size', '0.2', '--data-cache',
                                        'device', '--ema-decay', '0.9', '--quality-metrics', 'true', '--output', out]))
    logs = os.path.join(_run_dir(out), 'logs')
    val, val_ema = (_strict(os.path.join(logs, n)) for n in ('val_quality.json', 'val_quality_ema.json'))
    assert sorted(val_ema) == sorted(val) == sorted(Q.keys()) and all(len(v) == 1 for v in val_ema.values()) and val_ema != val
    test, test_ema = (_strict(os.path.join(logs, n)) for n in ('test_quality.json', 'test_quality_ema.json'))
    assert sorted(test_ema['per_image']) == sorted(test['per_image']) == sorted(Q.keys(Q.GROUPS_X)) and test_ema != test
    ck = os.path.join(_run_dir(out), 'training_checkpoints')
    per_image = {}
    for weights in ('raw', 'ema'):
        pred = str(tmp_path / f'pred_{weights}')
        cycle_gan.main(cycle_gan.parse_opt(['--input-images', dp, '--predict', '--weights', ck, '--logging', 'false', '--output', pred,
                                            '--batch-size', '4', '--predict-training', 'false', '--quality-metrics', 'true',
                                            '--predict-weights', weights]))
        per_image[weights] = _strict(os.path.join(_run_dir(pred), 'logs', 'prediction_metrics.json'))['per_image']
        assert sorted(per_image[weights]) == sorted(Q.keys(Q.GROUPS_X)) and all(len(v) == 3 for v in per_image[weights].values())
    assert all(per_image['ema'][k] != per_image['raw'][k] for k in Q.keys(Q.GROUPS_X))


def test_cyclegan_cli_quality_metrics_and_native_prediction(tmp_path, monkeypatch):
    from PIL import Image
    from gan_amd import cycle_gan
    from gan_amd import cycle_quality as Q
    rng = np.random.default_rng(0)
    dx, dy, big = (str(tmp_path / d) for d in ('x', 'y', 'big'))
    for d, n, shape in ((dx, 12, (64, 64)), (dy, 10, (64, 64)), (big, 2, (300, 320))):
        os.makedirs(d)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8), 'L').save(os.path.join(d, f"p{i}.png"))
    # 12 - 2 test files: 2 validation and 8 training files of X; 2 and 8 of Y: full batches of 2 throughout
    base = ['--input-images', dx, '--target-images', dy, '--train', '--epochs', '1', '--batch-size', '2', '--img-size', '256', '--logging',
            'false', '--seed', '7', '--test-img', '2', '--validation-size', '0.2', '--data-cache', 'device', '--quality-metrics', 'true']
    logs = []
    for k in range(2):
        out = str(tmp_path / f'out{k}')
        cycle_gan.main(cycle_gan.parse_opt(base + ['--output', out]))
        logs.append(os.path.join(_run_dir(out), 'logs'))
    for name in ('val_quality.json', 'test_quality.json', 'val_metrics.json', 'train_metrics.json'):
        assert _strict(os.path.join(logs[0], name)) == _strict(os.path.join(logs[1], name)), name          # two runs, equal files
    assert not os.path.exists(os.path.join(logs[0], 'val_quality_ema.json'))
    cfg = _strict(os.path.join(logs[0], 'config.json'))
    assert cfg['quality_metrics'] == 'true' and cfg['predict_resolution'] == 'resized' and cfg['tile_overlap'] == 64
    val = _strict(os.path.join(logs[0], 'val_quality.json'))
    assert sorted(val) == sorted(Q.keys()) and all(len(v) == 1 for v in val.values())
    assert all(-1 <= val[k][0] <= 1 for k in val if k.endswith('ssim')) and all(val[k][0] > 0 for k in val if k.endswith('mae'))
    test = _strict(os.path.join(logs[0], 'test_quality.json'))
    assert sorted(test) == ['mean', 'per_image'] and sorted(test['per_image']) == sorted(Q.keys(Q.GROUPS_X))
    assert all(len(v) == 2 for v in test['per_image'].values())
    assert abs(test['mean']['cycle_x_ssim'] - np.mean(test['per_image']['cycle_x_ssim'])) < 1e-9
    # native prediction with the cycle
    ck = os.path.join(os.path.dirname(logs[0]), 'training_checkpoints')
    out = str(tmp_path / 'native')
    shapes = []
    monkeypatch.setattr(cycle_gan, 'save_panels', lambda path, panels, gray: shapes.append([np.asarray(img).shape for _, img in panels]))
    cycle_gan.main(cycle_gan.parse_opt(['--input-images', big, '--predict', '--weights', ck, '--logging', 'false', '--output', out,
                                        '--predict-training', 'false', '--predict-resolution', 'native', '--quality-metrics', 'true']))
    run = _run_dir(out)
    assert shapes == [[(300, 320, 1)] * 2] * 2          # two panels per file, at the source size
    pm = _strict(os.path.join(run, 'logs', 'prediction_metrics.json'))
    assert sorted(pm['per_image']) == sorted(Q.keys(('cycle_x',))) and all(len(v) == 2 for v in pm['per_image'].values())
    assert all(-1 <= s <= 1 for s in pm['per_image']['cycle_x_ssim']) and all(np.isfinite(v) for v in pm['per_image']['cycle_x_psnr'])
    # a file smaller than the tile is an error that names the file
    small = str(tmp_path / 'small')
    os.makedirs(small)
    Image.fromarray(np.zeros((256, 200), np.uint8), 'L').save(os.path.join(small, 'tiny.png'))
    with pytest.raises(ValueError, match='tiny.png'):
        cycle_gan.main(cycle_gan.parse_opt(['--input-images', small, '--predict', '--weights', ck, '--logging', 'false', '--output',
                                            str(tmp_path / 'small_out'), '--predict-training', 'false', '--predict-resolution', 'native']))
