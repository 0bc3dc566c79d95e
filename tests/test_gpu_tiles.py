"""Tiled inference on the GPU: gan_tile_gather_u8 bit-exact against torch on the same device and against
what gan_pack leaves in the pad channels; gan_tile_blend against the fp64 reference tests/tile_ref.py; exactness, launch-split and
ownership properties; both entry points under graph capture; GeneratorModel.infer_tiled and `--predict-resolution native` end to end.

Blend gate: max |err| <= 1e-5 on values in [-1, 1] - at most 9 terms of magnitude <= 1, each with at most 5 fp32 roundings (two
divisions, the product of the weights, the product with the value, the cast of the reference's inputs) plus its addition:
9 * 6 * 2^-24 = 3.2e-6; the rest is margin.  The reference is evaluated on the STORED tile values, so the gate does not depend on
the dtype."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import tile_ref as R

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
BITS = {'f32': torch.int32, 'bf16': torch.int16, 'f16': torch.int16}
SOURCES = [(16, 16), (17, 31), (29, 40)]          # one tile; 2 x 2 with pulled-back last tiles; 3 x 3 (V = 4)
S = 16
GATE = 1e-5


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


def source(h, w, c, seed, right_half=False):
    """-> (uint8 device tensor [h, wfull, c], col0): the part used is [:, col0:col0 + w]."""
    rng = np.random.default_rng(seed)
    wfull, col0 = (2 * w + 3, w + 1) if right_half else (w, 0)
    return torch.from_numpy(rng.integers(0, 256, (h, wfull, c), dtype=np.uint8)).cuda(), col0


def expected_tiles(ctx, src, col0, w, V):
    """lut[src] of every tile, fp32 on the device: [nt, S, S, c]."""
    from gan_amd.tiling import normalize_lut, tile_origins
    part = normalize_lut(ctx)[src[:, col0:col0 + w].long()]
    return torch.stack([part[oy:oy + S, ox:ox + S] for oy in tile_origins(src.shape[0], S, V) for ox in tile_origins(w, S, V)])


def random_tiles(nt, c, pitch, dt, seed):
    """Stored tiles in [-1, 1] with NaN in the pad channels -> (device tensor [nt, S, S, pitch], float64 numpy of the real channels)."""
    rng = np.random.default_rng(seed)
    t = nan_tiles(nt, pitch, dt)
    t[..., :c] = torch.from_numpy(rng.uniform(-1, 1, (nt, S, S, c))).to(TD[dt]).cuda()
    return t, t[..., :c].double().cpu().numpy()


def blend(ctx, t, c, dt, h, w, V, image=None, t0=0, n=None, accumulate=0):
    from gan_amd.tiling import blend_tiles
    nt = t.shape[0]
    n = nt - t0 if n is None else n
    if image is None:
        image = torch.full((h, w, c), float('nan'), device='cuda')
    blend_tiles(ctx, view(t, c, t0, n), image, tile=S, overlap=V, t0=t0, n=n, accumulate=accumulate, dtype=code(dt))
    return image


# ---------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('dt', ['f32', 'bf16', 'f16'])
def test_gather_is_bit_exact_and_leaves_the_pad_channels_as_pack_does(ctx, dt, c):
    from gan_amd import _lib as L
    from gan_amd.tiling import gather_tiles, tile_grid
    for k, (h, w) in enumerate(SOURCES):
        for V in (0, 4, 8):
            for pitch in (8, c):
                for right in (False, True):
                    src, col0 = source(h, w, c, 100 * k + V + pitch, right)
                    ny, nx = tile_grid(h, w, S, V)
                    nt = ny * nx
                    want = expected_tiles(ctx, src, col0, w, V)
                    packed = nan_tiles(nt, pitch, dt)
                    L.check(ctx.lib.gan_pack(code(dt), want.contiguous().data_ptr(), C.byref(view(packed, c)), ctx.stream()), "pack")
                    got = nan_tiles(nt, pitch, dt)
                    gather_tiles(ctx, src, view(got, c), h=h, w=w, tile=S, overlap=V, t0=0, n=nt, col0=col0, dtype=code(dt))
                    what = (h, w, V, pitch, right)
                    assert torch.equal(got[..., :c].view(BITS[dt]), want.to(TD[dt]).view(BITS[dt])), what
                    assert torch.equal(got.view(BITS[dt]), packed.view(BITS[dt])), what          # pad channels included
                    if pitch > c:
                        assert bool(torch.isnan(got[..., c:]).all()), what
                    if nt > 2:      # a sub-range lands at the start of its own view and touches nothing else
                        sub = nan_tiles(nt, pitch, dt)
                        gather_tiles(ctx, src, view(sub, c, 1, nt - 2), h=h, w=w, tile=S, overlap=V, t0=1, n=nt - 2, col0=col0, dtype=code(dt))
                        assert torch.equal(sub[1:nt - 1].view(BITS[dt]), got[1:nt - 1].view(BITS[dt])), what
                        assert bool(torch.isnan(sub[0]).all()) and bool(torch.isnan(sub[nt - 1]).all()), what


# ---------------------------------------------------------------------------------------------------------------------
# blend
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('dt', ['f32', 'bf16', 'f16'])
def test_blend_matches_the_fp64_reference(ctx, dt, c):
    from gan_amd.tiling import tile_grid
    worst = 0.0
    for k, (h, w) in enumerate(SOURCES):
        for V in (0, 4, 8):
            for pitch in (8, c):
                ny, nx = tile_grid(h, w, S, V)
                t, t64 = random_tiles(ny * nx, c, pitch, dt, 7 * k + V + pitch)
                got = blend(ctx, t, c, dt, h, w, V).double().cpu().numpy()
                err = float(np.abs(got - R.blend(t64, h, w, S, V)).max())
                worst = max(worst, err)
                assert np.isfinite(got).all() and err <= GATE, (h, w, V, pitch, err)
    print(f"blend {dt} c={c}: max |err| {worst:.3e} (gate {GATE:.0e})")


@pytest.mark.parametrize('dt', ['f32', 'bf16', 'f16'])
def test_single_tile_comes_back_bit_for_bit_and_constants_stay_constant(ctx, dt):
    from gan_amd.tiling import tile_grid
    for c in (1, 3):
        t, _ = random_tiles(1, c, 8, dt, 3 + c)
        got = blend(ctx, t, c, dt, S, S, 4)
        assert torch.equal(got, t[0, :, :, :c].float())
    for v in (1.0, -0.75, 0.3333333):
        for (h, w), V in (((29, 40), 4), ((17, 31), 8), ((29, 40), 0)):
            ny, nx = tile_grid(h, w, S, V)
            t = nan_tiles(ny * nx, 8, dt)
            t[..., :1] = v
            stored = float(t[0, 0, 0, 0])
            err = float((blend(ctx, t, 1, dt, h, w, V).double() - stored).abs().max())
            print(f"constant {dt} {v} {h}x{w} V={V}: max |err| {err:.3e}")
            assert err <= 2e-7 * abs(stored) * 9, (dt, v, h, w, V, err)


@pytest.mark.parametrize('c', [1, 3])
def test_gather_then_blend_returns_the_image(ctx, c):
    from gan_amd.tiling import gather_tiles, normalize_lut, tile_grid
    for k, (h, w) in enumerate(SOURCES):
        for V in (0, 4, 8):
            src, col0 = source(h, w, c, 50 + k + V, right_half=True)
            nt = int(np.prod(tile_grid(h, w, S, V)))
            t = nan_tiles(nt, 8, 'f32')
            gather_tiles(ctx, src, view(t, c), h=h, w=w, tile=S, overlap=V, t0=0, n=nt, col0=col0, dtype=code('f32'))
            got = blend(ctx, t, c, 'f32', h, w, V)
            err = float((got - normalize_lut(ctx)[src[:, col0:col0 + w].long()]).abs().max())
            assert err <= GATE, (h, w, V, err)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_split_launches_and_repeated_calls_give_the_same_bits(ctx, dt):
    from gan_amd.tiling import tile_grid
    for (h, w), V, c, pitch in (((29, 40), 4, 3, 8), ((29, 40), 8, 1, 8), ((17, 31), 4, 1, 1), ((29, 40), 0, 3, 3)):
        nt = int(np.prod(tile_grid(h, w, S, V)))
        t, _ = random_tiles(nt, c, pitch, dt, 11 + V)
        once = blend(ctx, t, c, dt, h, w, V)
        assert torch.equal(once, blend(ctx, t, c, dt, h, w, V))
        for step in (1, 2):
            img = torch.full((h, w, c), float('nan'), device='cuda')
            for t0 in range(0, nt, step):
                blend(ctx, t, c, dt, h, w, V, image=img, t0=t0, n=min(step, nt - t0), accumulate=int(t0 > 0))
            assert torch.equal(img.view(torch.int32), once.view(torch.int32)), (h, w, V, c, step)


def test_a_launch_owns_only_the_pixels_its_tiles_cover(ctx):
    h, w, V = 29, 40, 4
    t, t64 = random_tiles(9, 1, 8, 'bf16', 5)
    img = torch.full((h, w, 1), 123.0, device='cuda')
    blend(ctx, t, 1, 'bf16', h, w, V, image=img, t0=0, n=1, accumulate=1)
    got = img.cpu().numpy()
    inside = np.zeros((h, w), bool)
    inside[:S, :S] = True
    assert np.array_equal(got[~inside], np.full((~inside).sum() * 1, 123.0, np.float32).reshape(-1, 1))
    want = R.blend(t64[:1], h, w, S, V, t0=0, n=1, start=np.full((h, w, 1), 123.0))
    assert np.abs(got - want)[inside].max() <= 123.0 * 2 ** -23 + GATE          # the sentinel's own rounding in the sum
    img = blend(ctx, t, 1, 'bf16', h, w, V, t0=0, n=1, accumulate=0).cpu().numpy()          # accumulate = 0: the rest becomes 0
    assert not img[~inside].any() and np.abs(img - R.blend(t64[:1], h, w, S, V, t0=0, n=1))[inside].max() <= GATE
    mid = blend(ctx, t, 1, 'bf16', h, w, V, t0=4, n=1, accumulate=0).cpu().numpy()          # the centre tile alone, read at offset 4
    assert np.abs(mid - R.blend(t64[4:5], h, w, S, V, t0=4, n=1)).max() <= GATE


def test_both_entry_points_are_capturable(ctx):
    from gan_amd.tiling import blend_tiles, gather_tiles
    h, w, V, c = 29, 40, 4, 3
    src, col0 = source(h, w, c, 77, right_half=True)
    t = nan_tiles(9, 8, 'bf16')
    img = torch.empty((h, w, c), device='cuda')

    def run():
        gather_tiles(ctx, src, view(t, c), h=h, w=w, tile=S, overlap=V, t0=0, n=9, col0=col0)
        blend_tiles(ctx, view(t, c, 0, 5), img, tile=S, overlap=V, t0=0, n=5, accumulate=0)
        blend_tiles(ctx, view(t, c, 5, 4), img, tile=S, overlap=V, t0=5, n=4, accumulate=1)
    run()
    torch.cuda.synchronize()
    eager_t, eager_img = t.clone(), img.clone()
    gr = ctx.capture_graph(run)
    for _ in range(2):
        t.fill_(float('nan'))
        img.fill_(float('nan'))
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(t.view(torch.int16), eager_t.view(torch.int16)) and torch.equal(img, eager_img)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: the smallest real network, C = 1, S = 256
# ---------------------------------------------------------------------------------------------------------------------
_MODELS = {}
EPS = {'f32': 2.0 ** -23, 'bf16': 2.0 ** -7}          # one ulp of the storage type at 1.0


def _cfg(dt):
    cfg = dict(img_size=256, channels='1', learning_rate=2e-4, beta_1=0.5, beta_2=0.999, seed=3, generator_loss='l1',
               input_img_orient='left', batch_size=1, dtype=dt)
    cfg['lambda'] = 100
    return cfg


def trained(dt):
    """A Pix2Pix whose BatchNorm generator has taken one train step: moving statistics away from (0, 1)."""
    if dt not in _MODELS:
        from gan_amd.pix2pix import Pix2Pix
        p = Pix2Pix(_cfg(dt))
        rng = np.random.default_rng(9)
        x, y = (torch.from_numpy(rng.uniform(-1, 1, (1, 256, 256, 1)).astype(np.float32)) for _ in range(2))
        p.train_step(x, y, True)
        mm = p.generator.net.params.state['down3.moving_mean']
        assert float(mm.abs().max()) > 0
        _MODELS[dt] = p
    return _MODELS[dt]


def check_against_host_cut(model, dt, h, w, V, origins_y, origins_x, seed, batches=(None,)):
    """infer_tiled == fp64 blend of infer(the numpy-cut tiles): the tiles run in the same batch composition (all of them as one
    batch, or the same chunks), so the network sees the same bits either way and only the blend's fp32 arithmetic differs.  Gate
    1e-5 (the blend) + one ulp of the storage type at 1.0 (the typed read)."""
    from gan_amd import data as D
    from gan_amd.tiling import tile_origins
    assert tile_origins(h, 256, V) == origins_y and tile_origins(w, 256, V) == origins_x
    src = np.random.default_rng(seed).integers(0, 256, (h, w, 1), dtype=np.uint8)
    dev = torch.from_numpy(src).cuda()
    tiles = R.cut(D.normalize(src.astype(np.float32)), 256, V)
    model.fold()
    for batch in batches:
        got = model.infer_tiled(dev, tile=256, overlap=V, batch=batch, fold=False)
        chunk = len(tiles) if batch is None else batch
        out = np.concatenate([model.infer(tiles[t0:t0 + chunk], fold=False).double().cpu().numpy() for t0 in range(0, len(tiles), chunk)])
        err = float(np.abs(got.double().cpu().numpy() - R.blend(out, h, w, 256, V)).max())
        print(f"infer_tiled {dt} {h}x{w} V={V} batch={batch}: max |err| {err:.3e} (gate {GATE + EPS[dt]:.3e})")
        assert got.shape == (h, w, 1) and err <= GATE + EPS[dt], (batch, err)


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_infer_tiled_of_a_tile_sized_image_is_infer(dt):
    from gan_amd import data as D
    m = trained(dt).generator
    src = np.random.default_rng(1).integers(0, 256, (256, 256, 1), dtype=np.uint8)
    got = m.infer_tiled(torch.from_numpy(src).cuda(), tile=256, overlap=64)
    want = m.infer(D.normalize(src.astype(np.float32))[None])[0]
    assert torch.equal(got, want)
    pair = np.concatenate([src[:, ::-1], src], axis=1)              # the same image as the right half of a pair
    assert torch.equal(m.infer_tiled(torch.from_numpy(np.ascontiguousarray(pair)).cuda(), tile=256, overlap=0, col0=256), want)


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_infer_tiled_two_tiles(dt):
    check_against_host_cut(trained(dt).generator, dt, 256, 320, 64, [0], [0, 64], 2, batches=(None, 1))


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_infer_tiled_two_by_two(dt):
    check_against_host_cut(trained(dt).generator, dt, 300, 300, 64, [0, 44], [0, 44], 3, batches=(None, 3))


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_infer_tiled_instancenorm_generator(dt):
    from gan_amd.base_gan import GeneratorModel
    from gan_amd.nets import Ctx, GeneratorNet
    m = GeneratorModel(GeneratorNet(Ctx('cuda:0', dt, workspace_mb=64), 1, 'instancenorm', seed=5))
    check_against_host_cut(m, dt, 256, 320, 64, [0], [0, 64], 4)


def test_infer_tiled_refuses_what_it_cannot_tile():
    m = trained('bf16').generator
    small = torch.zeros((200, 300, 1), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError):
        m.infer_tiled(small, tile=256, overlap=64)
    ok = torch.zeros((256, 600, 1), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError):
        m.infer_tiled(ok, tile=256, overlap=129)
    with pytest.raises(ValueError):
        m.infer_tiled(ok, tile=256, overlap=64, col0=400, width=256)
    with pytest.raises(ValueError):
        m.infer_tiled(ok.float(), tile=256, overlap=64)


# ---------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    """Two synthetic 600 x 256 pair files and a checkpoint of the trained bf16 model."""
    from PIL import Image
    from gan_amd.checkpoint import Checkpoint, CheckpointManager
    root = tmp_path_factory.mktemp('tiles')
    data = str(root / 'data')
    os.makedirs(data)
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (256, 600), dtype=np.uint8), 'L').save(os.path.join(data, f"p{i}.png"))
    p = trained('bf16')
    CheckpointManager(Checkpoint(generator=p.generator, discriminator=p.discriminator, generator_optimizer=p.generator_optimizer,
                                 discriminator_optimizer=p.discriminator_optimizer), str(root / 'ck'), max_to_keep=1).save()
    return root, data, str(root / 'ck')


def _restored(args, ck):
    from gan_amd import pix2pix
    from gan_amd.checkpoint import Checkpoint, latest_checkpoint
    p = pix2pix.Pix2Pix(vars(pix2pix.parse_opt(args)))
    Checkpoint(generator=p.generator, discriminator=p.discriminator, generator_optimizer=p.generator_optimizer,
               discriminator_optimizer=p.discriminator_optimizer).restore(latest_checkpoint(ck))
    return p


def _run(out):
    return os.path.join(out, sorted(os.listdir(out))[0])


def test_pix2pix_cli_predicts_at_the_source_resolution(pairs):
    from PIL import Image
    from gan_amd import data as D
    from gan_amd import pix2pix
    from gan_amd.quality import KEYS, image_quality
    root, data, ck = pairs
    out = str(root / 'native')
    args = ['--data', data, '--predict', '--weights', ck, '--logging', 'false', '--output', out, '--predict-resolution', 'native',
            '--predict-training', 'false', '--quality-metrics', 'true', '--input-img-orient', 'right']
    pix2pix.main(pix2pix.parse_opt(args))
    run = _run(out)
    assert sorted(os.listdir(os.path.join(run, 'prediction_images'))) == ['img0.png', 'img1.png']
    cfg = json.load(open(os.path.join(run, 'logs', 'config.json')))
    assert cfg['predict_resolution'] == 'native' and cfg['tile_overlap'] == 64
    pm = json.load(open(os.path.join(run, 'logs', 'prediction_metrics.json')))['per_image']
    assert all(len(pm[k]) == 2 and all(np.isfinite(v) for v in pm[k]) for k in KEYS)
    p = _restored(args, ck)
    lut = torch.from_numpy(D.normalize_table()).cuda()
    for k, f in enumerate(p.image_pipeline(predict=True)[0].files):
        src = torch.from_numpy(D.decode(f, 1).copy()).cuda()
        pred = p.generator.infer_tiled(src, tile=256, overlap=64, col0=300, width=300)          # orient right: the input is the right half
        assert pred.shape == (256, 300, 1)
        row = image_quality(p.ctx, pred[None], lut[src[:, :300].long()][None]).cpu().tolist()[0]
        assert [pm[key][k] for key in KEYS] == row, (k, row)
    # a half smaller than the tile is an error that names the file
    small = str(root / 'small')
    os.makedirs(small)
    Image.fromarray(np.zeros((256, 500), np.uint8), 'L').save(os.path.join(small, 'tiny.png'))
    with pytest.raises(ValueError, match='tiny.png'):
        pix2pix.main(pix2pix.parse_opt(['--data', small, '--predict', '--weights', ck, '--logging', 'false', '--output', str(root / 'small_out'),
                                        '--predict-resolution', 'native', '--predict-training', 'false']))


def test_pix2pix_cli_default_path_is_the_resized_one(pairs):
    from gan_amd import pix2pix
    from gan_amd.quality import KEYS, image_quality
    root, data, ck = pairs
    out = str(root / 'resized')
    args = ['--data', data, '--predict', '--weights', ck, '--logging', 'false', '--output', out, '--predict-training', 'false',
            '--quality-metrics', 'true', '--batch-size', '2']
    pix2pix.main(pix2pix.parse_opt(args))
    run = _run(out)
    assert sorted(os.listdir(os.path.join(run, 'prediction_images'))) == ['img0.png', 'img1.png']
    pm = json.load(open(os.path.join(run, 'logs', 'prediction_metrics.json')))['per_image']
    p = _restored(args, ck)
    ds = p.image_pipeline(predict=True)[0]
    ex = list(ds.unbatch())
    assert all(a.shape == (256, 256, 1) for a, _ in ex)             # every half resized to img_size, as before
    p.generator.fold()
    pred = p.generator.infer(np.stack([a for a, _ in ex]), fold=False)
    rows = image_quality(p.ctx, pred, np.stack([b for _, b in ex])).cpu().tolist()
    for k in range(2):
        assert [pm[key][k] for key in KEYS] == rows[k], k
