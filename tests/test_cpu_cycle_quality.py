"""CPU side of the CycleGAN cycle-consistency metrics and native-size prediction: the new flags of the
CycleGAN parser (declared in the slots of its option class, so vars(opt) keeps the flag set the two drivers are compared on), their
refusals, the argument checks of gan_tile_gather (every descriptor tried here is refused before the launch), the header and the
binding, and the slice restatement of the gathers against tests/tile_ref.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests import tile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = ['--input-images', 'x', '--target-images', 'y', '--output', 'o', '--train', '--epochs', '1']
PRED = ['--input-images', 'x', '--output', 'o', '--predict', '--weights', 'w']
INFER = PRED + ['--predict-training', 'false']


def test_new_flags_defaults_and_where_they_live():
    from gan_amd import cycle_gan
    from gan_amd.runner import config_of
    for argv in (TRAIN, PRED):
        o = cycle_gan.parse_opt(argv)
        assert (o.quality_metrics, o.predict_resolution, o.tile_overlap, o.pool_size) == ('false', 'resized', 64, 0)
        for flag in ('quality_metrics', 'predict_resolution', 'tile_overlap'):
            assert flag not in vars(o), flag
        cfg = config_of(o)
        assert cfg['quality_metrics'] == 'false' and cfg['predict_resolution'] == 'resized' and cfg['tile_overlap'] == 64
    assert cycle_gan.parse_opt(TRAIN + ['--img-size', '512']).tile_overlap == 128
    o = cycle_gan.parse_opt(TRAIN + ['--quality-metrics', 'true'])
    assert 'quality_metrics' not in vars(o) and config_of(o)['quality_metrics'] == 'true'
    o = cycle_gan.parse_opt(INFER + ['--predict-resolution', 'native', '--quality-metrics', 'true', '--tile-overlap', '128'])
    assert config_of(o)['predict_resolution'] == 'native' and config_of(o)['tile_overlap'] == 128 and o.quality_metrics == 'true'
    assert cycle_gan.parse_opt(INFER + ['--tile-overlap', '0']).tile_overlap == 0


def test_refusals(capsys):
    from gan_amd import cycle_gan
    for argv in (PRED + ['--predict-resolution', 'native'], PRED + ['--predict-resolution', 'native', '--predict-training', 'true'],
                 TRAIN + ['--predict-resolution', 'native', '--predict-training', 'false']):
        with pytest.raises(SystemExit):
            cycle_gan.parse_opt(argv)
        assert "--predict-resolution native requires --predict and --predict-training false" in capsys.readouterr().err
    for argv in (PRED + ['--quality-metrics', 'true'], PRED + ['--quality-metrics', 'true', '--predict-training', 'true']):
        with pytest.raises(SystemExit):
            cycle_gan.parse_opt(argv)
        err = capsys.readouterr().err
        assert "--predict-training false" in err and "dropout" in err and "not a deterministic measurement" in err
    for v in ('129', '-1'):
        with pytest.raises(SystemExit):
            cycle_gan.parse_opt(TRAIN + ['--tile-overlap', v])
        assert f"--tile-overlap {v} is outside [0, img-size / 2 = 128]" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cycle_gan.parse_opt(INFER + ['--img-size', '512', '--tile-overlap', '257'])
    for argv in (['--quality-metrics', 'yes'], ['--predict-resolution', 'full']):
        with pytest.raises(SystemExit):
            cycle_gan.parse_opt(INFER + argv)


def test_pix2pix_keeps_the_flags_in_its_dictionary():
    from gan_amd import pix2pix
    o = pix2pix.parse_opt(['--data', 'd', '--output', 'o', '--train', '--epochs', '1'])
    assert {'quality_metrics', 'predict_resolution', 'tile_overlap'} <= set(vars(o))
    assert (o.quality_metrics, o.predict_resolution, o.tile_overlap) == ('false', 'resized', 64)


def test_metric_keys():
    from gan_amd import cycle_quality as Q
    assert Q.keys(Q.GROUPS_X) == ('cycle_x_ssim', 'cycle_x_psnr', 'cycle_x_mae', 'identity_x_ssim', 'identity_x_psnr', 'identity_x_mae')
    assert Q.keys() == Q.keys(Q.GROUPS_X) + ('cycle_y_ssim', 'cycle_y_psnr', 'cycle_y_mae', 'identity_y_ssim', 'identity_y_psnr',
                                             'identity_y_mae')


def test_slice_restatement_of_the_gather_against_the_reference():
    """cut_tiles - what the GPU tests hold the float gather against - cuts what tile_ref.cut cuts, for every side 16..80 at S = 16."""
    from gan_amd.tiling import cut_tiles
    rng = np.random.default_rng(0)
    for V in (0, 4, 8):
        for Ln in range(16, 81):
            for h, w in ((Ln, 16), (16, Ln), (Ln, 97 - Ln)):
                img = rng.uniform(-1, 1, (h, w, 3)).astype(np.float32)
                want = R.cut(img, 16, V)
                assert np.array_equal(cut_tiles(img, 16, V), want), (h, w, V)
                assert np.array_equal(cut_tiles(torch.from_numpy(img), 16, V).numpy(), want), (h, w, V)
                wide = np.concatenate([img[:, ::-1], img, img[:, :2]], axis=1)      # the same image as a column window
                assert np.array_equal(cut_tiles(wide, 16, V, col0=w, width=w), want), (h, w, V)


def test_uncounted_passes_leave_the_later_orders_alone():
    """CycleGAN.evaluate walks the shuffled validation sets once more per epoch: inside data.uncounted_passes the extra passes draw
    the orders that are due, and afterwards the next pass draws the order it draws without them."""
    from gan_amd import data as D
    files = [str(i) for i in range(7)]
    new = lambda: D.Batches(files, lambda f: (np.full((1, 1, 1), float(f), np.float32),), 2, None, shuffle_seed=5)
    order = lambda ds: [int(v) for (b,) in ds for v in b.flatten()]
    plain, extra = new(), new()
    want = [order(plain) for _ in range(3)]
    assert want[0] != want[1] != want[2] and sorted(want[0]) == list(range(7))
    assert order(extra) == want[0]
    with D.uncounted_passes(extra, None, [1, 2]):
        assert [order(extra), order(extra)] == want[1:]
    assert order(extra) == want[1]
    with pytest.raises(RuntimeError):          # the counters come back after an exception too
        with D.uncounted_passes(extra):
            order(extra)
            raise RuntimeError
    assert order(extra) == want[2]
    dev = D.DeviceBatches.__new__(D.DeviceBatches)          # the device-resident surface counts the same way
    dev.epoch = 4
    with D.uncounted_passes(dev):
        dev.epoch += 1
    assert dev.epoch == 4


def _gather(L, **kw):
    """A float gather descriptor that passes every check (29 x 40 image, S = 16, V = 4: a 3 x 3 grid; pointers are never read)."""
    f = dict(src_dtype=L.F32, src=1 << 20, src_elems=29 * 40, src_pitch=40, col0=0, h=29, w=40, c=1, tile=16, overlap=4, t0=0, n=9,
             dst_dtype=L.BF16, dst=L.GanTensor(1 << 22, 9, 16, 16, 1, 8))
    f.update(kw)
    return L.GanTileGatherFDesc(**f)


def test_gather_abi_refuses_bad_descriptors_before_any_launch():
    from gan_amd import _lib as L
    lib = L.load()
    fn = lib.gan_tile_gather
    T = lambda n=9, S=16, c=1, pitch=8, ptr=1 << 22: L.GanTensor(ptr, n, S, S, c, pitch)
    g = lambda **kw: fn(C.byref(_gather(L, **kw)), None)
    assert fn(None, None) == L.E_ARG
    assert L.GanTileGatherFDesc().struct_size == C.sizeof(L.GanTileGatherFDesc)
    for size in (C.sizeof(L.GanTileGatherFDesc) - 4, 0):
        d = _gather(L)
        d.struct_size = size
        assert fn(C.byref(d), None) == L.E_ARG
    assert g(src=None) == L.E_ARG and g(dst=T(ptr=None)) == L.E_ARG
    for dt in (-1, 3, 7):
        assert g(src_dtype=dt) == L.E_ARG and g(dst_dtype=dt) == L.E_ARG
    # a 16-bit source is copied, never converted
    assert g(src_dtype=L.BF16, dst_dtype=L.F16) == L.E_ARG and g(src_dtype=L.F16, dst_dtype=L.BF16) == L.E_ARG
    assert g(src_dtype=L.BF16, dst_dtype=L.F32) == L.E_ARG
    for c in (0, 2, 4):
        assert g(c=c, dst=T(c=c)) == L.E_ARG, c
    assert g(overlap=9) == L.E_SHAPE and g(overlap=-1) == L.E_SHAPE
    assert g(h=15) == L.E_SHAPE and g(w=15) == L.E_SHAPE and g(h=4097) == L.E_SHAPE
    assert g(tile=20, dst=T(S=20)) == L.E_SHAPE and g(tile=8, overlap=0, dst=T(S=8)) == L.E_SHAPE
    assert g(t0=1) == L.E_ARG and g(t0=8, n=2, dst=T(n=2)) == L.E_ARG and g(t0=-1) == L.E_ARG
    assert g(n=0, dst=T(n=0)) == L.E_ARG and g(n=4) == L.E_ARG
    assert g(dst=T(c=3)) == L.E_ARG and g(c=3, dst=T(c=3, pitch=2)) == L.E_ARG
    assert g(dst=T(ptr=(1 << 22) + 1)) == L.E_ARG and g(dst_dtype=L.F32, dst=T(ptr=(1 << 22) + 2)) == L.E_ARG
    assert g(src=(1 << 20) + 2) == L.E_ARG and g(src_dtype=L.BF16, src=(1 << 20) + 1) == L.E_ARG      # the source's own alignment
    assert g(col0=-1) == L.E_ARG and g(col0=1) == L.E_ARG                         # the part used leaves the source row
    assert g(src_pitch=39) == L.E_ARG and g(src_pitch=0) == L.E_ARG
    assert g(src_elems=29 * 40 - 1) == L.E_ARG and g(src_elems=0) == L.E_ARG      # the last row leaves the buffer
    assert g(src_pitch=100, col0=60, src_elems=28 * 100 + 99) == L.E_ARG          # a right half: one element short


def test_header_and_binding_of_the_float_gather_agree():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_binding
    from gan_amd import _lib as L
    fields = gen_binding.parse_structs()['GanTileGatherFDesc']
    want = [(f, getattr(C, t[2:]) if t.startswith('C.') else getattr(L, t)) for f, t in fields]
    assert list(L.GanTileGatherFDesc._fields_) == want and fields[0] == ('struct_size', 'C.c_uint32')
    assert L.SYMBOLS['gan_tile_gather'] == (C.c_int, [C.POINTER(L.GanTileGatherFDesc), C.c_void_p])
    assert hasattr(L.load(), 'gan_tile_gather')
