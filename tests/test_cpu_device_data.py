"""CPU side of the device-resident input pipeline: the index tables against `resize_nearest`, the argument
checks of gan_augment_u8 (no launch without a GPU), the two CLI flags, the size cap and the order of the random draws."""
import ctypes as C

import numpy as np
import pytest

from gan_amd import data as D

SIZES_OUT = (256, 286, 512, 542)


def test_nearest_index_reproduces_resize_nearest():
    """Every n_in in 1..700 and every output length of the pipeline; and the float64 expression is NOT the integer form."""
    differ = 0
    for n_out in SIZES_OUT:
        for n_in in range(1, 701):
            ramp = np.arange(n_in, dtype=np.float32)[:, None, None]
            idx = D.nearest_index(n_in, n_out)
            assert idx.shape == (n_out,) and idx.min() >= 0 and idx.max() < n_in and (np.diff(idx) >= 0).all()
            assert np.array_equal(D.resize_nearest(ramp, n_out, 1)[:, 0, 0], idx.astype(np.float32)), (n_in, n_out)
            if n_in % 50 == 7:                      # the column axis takes the same expression
                assert np.array_equal(D.resize_nearest(ramp.reshape(1, n_in, 1), 1, n_out)[0, :, 0], idx.astype(np.float32))
            differ += not np.array_equal(idx, ((2 * np.arange(n_out) + 1) * n_in) // (2 * n_out))
    assert differ > 0


def test_composed_cyclegan_table_equals_resizing_twice():
    rng = np.random.default_rng(0)
    for size in (256, 512):
        for h, w in ((1, 1), (100, 37), (248, 496), (300, 600), (size, size), (700, 513)):
            img = rng.integers(0, 256, (h, w, 3)).astype(np.float32)
            twice = D.resize_nearest(D.resize_nearest(img, size, size), size + 30, size + 30)
            second = D.nearest_index(size, size + 30)
            rows, cols = D.nearest_index(h, size)[second], D.nearest_index(w, size)[second]
            assert np.array_equal(img[rows][:, cols], twice)
    assert np.array_equal(D.nearest_index(256, 256), np.arange(256))        # the validation form's second resize is the identity


def _good(L):
    """A descriptor that passes every check (device pointers are never read on the host) and its sample array."""
    s = (L.GanAugSample * 2)()
    for k in range(2):
        s[k].src_offset, s[k].src_pitch, s[k].col0, s[k].col0_b = 64 * k, 32, 0, 16
        s[k].row_table, s[k].col_table, s[k].col_table_b, s[k].crop_y, s[k].crop_x, s[k].flip = 0, 1, 1, 30, 0, 1
    d = L.GanAugmentDesc(2, 256, 1, 4096, 1 << 20, 8192, 2, 286, 12288, 16384, 32768, C.addressof(s))
    return d, s


def test_augment_abi_refuses_bad_descriptors_before_any_launch():
    from gan_amd import _lib as L
    lib = L.load()
    call = lambda d: lib.gan_augment_u8(C.byref(d), None)
    assert lib.gan_augment_u8(None, None) == L.E_ARG
    assert C.sizeof(L.GanAugSample) == 48 and L.GanAugmentDesc().struct_size == C.sizeof(L.GanAugmentDesc)

    def bad(code, **fields):
        d, s = _good(L)
        for k, v in fields.items():
            setattr(d, k, v)
        assert call(d) == code, fields

    def bad_sample(code, **fields):
        d, s = _good(L)
        for k, v in fields.items():
            setattr(s[1], k, v)
        assert call(d) == code, fields

    bad(L.E_ARG, struct_size=C.sizeof(L.GanAugmentDesc) - 8)
    for ptr in ('src', 'tables', 'lut', 'dst_a', 'samples'):
        bad(L.E_ARG, **{ptr: None})
    for n in (0, -1, L.AUGMENT_MAX_SAMPLES + 1):
        bad(L.E_ARG, n=n)
    for c in (0, 2, 4):
        bad(L.E_ARG, c=c)
    bad(L.E_ARG, n_tables=0)
    bad(L.E_ARG, src=4100)                      # 16-byte alignment of the source buffer and of both destinations
    bad(L.E_ARG, dst_a=16388)
    bad(L.E_ARG, dst_b=32772)
    bad(L.E_ARG, src_bytes=1000)                # not a multiple of 16
    bad(L.E_ARG, src_bytes=0)
    for out in (0, 128, 255, 1024):
        bad(L.E_SHAPE, out=out)
    bad(L.E_SHAPE, table_len=255)               # shorter than the output
    bad(L.E_SHAPE, out=512)                     # (table_len 286 < 512)
    for t in (-1, 2):
        bad_sample(L.E_ARG, row_table=t)
        bad_sample(L.E_ARG, col_table=t)
        bad_sample(L.E_ARG, col_table_b=t)
    bad_sample(L.E_ARG, src_offset=-16)
    bad_sample(L.E_ARG, src_offset=1 << 20)     # first row outside the buffer
    bad_sample(L.E_ARG, src_pitch=0)
    bad_sample(L.E_ARG, col0=-1)
    bad_sample(L.E_ARG, flip=2)
    for y, x in ((31, 0), (0, 31), (-1, 0), (0, -1)):
        bad_sample(L.E_SHAPE, crop_y=y, crop_x=x)


def test_cli_flags_and_defaults():
    from gan_amd import cycle_gan, pix2pix
    p = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']
    c = ['--input-images', 'x', '--target-images', 'y', '--output', 'o', '--train', '--epochs', '1']
    for mod, base in ((pix2pix, p), (cycle_gan, c)):
        opt = mod.parse_opt(base)
        assert opt.data_cache == 'host' and opt.data_cache_gb == 64
        opt = mod.parse_opt(base + ['--data-cache', 'device', '--data-cache-gb', '1.5'])
        assert opt.data_cache == 'device' and opt.data_cache_gb == 1.5
        with pytest.raises(SystemExit):
            mod.parse_opt(base + ['--data-cache', 'gpu'])


def test_device_dataset_cap_raises_before_touching_the_device(tmp_path, monkeypatch):
    """Sizes come from the image headers: nothing is decoded and nothing is allocated when the cap is exceeded."""
    from PIL import Image
    files = []
    for k in range(3):
        files.append(str(tmp_path / f"{k}.png"))
        Image.fromarray(np.full((40, 100), 7 * k, np.uint8)).save(files[-1])
    monkeypatch.setattr(D, 'decode', lambda *a: pytest.fail("decoded although the cap was exceeded"))
    with pytest.raises(ValueError, match='--data-cache-gb'):
        D.DeviceDataset(files, 1, 256, 'cuda:0', cap_bytes=3 * 4000 - 1)
    with pytest.raises(ValueError, match='--data-cache-gb'):
        D.DeviceDataset(files, 3, 256, 'cuda:0', cap_bytes=3 * 12000 - 1)


def test_draw_jitter_consumes_the_generator_as_random_jitter_pair_does():
    size = 256
    r1, r2, r3 = (np.random.default_rng(77) for _ in range(3))
    ys, xs = np.meshgrid(np.arange(size + 30, dtype=np.float32), np.arange(size + 30, dtype=np.float32), indexing='ij')
    a = (ys * 1000 + xs)[..., None]                    # already size+30: the resize is the identity, every value names its position
    for _ in range(100):
        y, x, flip = D.draw_jitter(r1)
        assert 0 <= y <= 30 and 0 <= x <= 30 and isinstance(flip, bool)
        ja, jb = D.random_jitter_pair(a, -a, size, r2)
        js = D.random_jitter_single(a, size, r3)
        want = a[y:y + size, x:x + size]
        want = want[:, ::-1] if flip else want
        assert np.array_equal(ja, want) and np.array_equal(jb, -want) and np.array_equal(js, want)
    assert r1.random() == r2.random() == r3.random()
