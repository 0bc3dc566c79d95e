"""CPU side of tiled inference: the tile geometry in Python, in C (gan_tile_grid) and in the fp64 reference
tests/tile_ref.py; the argument checks of gan_tile_gather_u8 / gan_tile_blend (nothing is launched without a GPU: every descriptor
tried here is refused before the launch); the header, the binding and the INTEGRATION.md snippet; the CLI flags."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from tests import tile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_grid(lib, h, w, S, V):
    ny, nx = C.c_int32(-7), C.c_int32(-7)
    rc = lib.gan_tile_grid(h, w, S, V, C.byref(ny), C.byref(nx))
    return rc, ny.value, nx.value


def test_tile_origins_hand_written_cases():
    from gan_amd.tiling import tile_grid, tile_origins
    assert tile_origins(16, 16, 4) == [0]
    assert tile_origins(17, 16, 4) == [0, 1]
    assert tile_origins(28, 16, 4) == [0, 12]
    assert tile_origins(29, 16, 4) == [0, 12, 13]
    assert tile_origins(40, 16, 8) == [0, 8, 16, 24]
    assert tile_grid(29, 40, 16, 4) == (3, 3) and tile_grid(512, 640, 256, 64) == (3, 3) and tile_grid(512, 640, 512, 128) == (1, 2)
    for bad in ((15, 16, 4), (16, 16, 9), (16, 16, -1), (40, 20, 4), (16, 8, 0), (2048, 1032, 0), (4097, 16, 0)):
        with pytest.raises(ValueError):
            tile_origins(*bad)


def test_python_c_and_reference_grids_agree_and_every_pixel_is_covered():
    from gan_amd import _lib as L
    from gan_amd.tiling import tile_origins
    lib = L.load()
    for V in (0, 3, 8):
        for Ln in range(16, 81):
            org = tile_origins(Ln, 16, V)
            assert org == R.origins(Ln, 16, V), (Ln, V)
            assert _c_grid(lib, Ln, 16, 16, V) == (0, len(org), 1) and _c_grid(lib, 16, Ln, 16, V) == (0, 1, len(org)), (Ln, V)
            assert org[0] == 0 and org[-1] == Ln - 16 and all(b > a for a, b in zip(org, org[1:])), (Ln, V, org)
            cov = R.cover_counts(Ln, 16, V)
            assert cov.min() >= 1 and cov.max() <= 3, (Ln, V, cov)
            wts = R.axis_weights(Ln, 16, V)
            assert np.abs(wts.sum(axis=0) - 1).max() <= 1e-15, (Ln, V)
    assert _c_grid(lib, 512, 640, 256, 64) == (0, 3, 3) and _c_grid(lib, 4096, 4096, 16, 8) == (0, 511, 511)


def test_tile_grid_refusals():
    from gan_amd import _lib as L
    lib = L.load()
    n = C.c_int32()
    assert lib.gan_tile_grid(32, 32, 16, 4, None, C.byref(n)) == L.E_ARG and lib.gan_tile_grid(32, 32, 16, 4, C.byref(n), None) == L.E_ARG
    for h, w, S, V in ((15, 32, 16, 4), (32, 15, 16, 4), (32, 32, 16, 9), (32, 32, 16, -1), (32, 32, 20, 4), (32, 32, 8, 0),
                       (2048, 2048, 1032, 0), (4097, 32, 16, 4), (32, 4097, 16, 4)):
        assert _c_grid(lib, h, w, S, V) == (L.E_SHAPE, -7, -7), (h, w, S, V)


def _gather(L, **kw):
    """A gather descriptor that passes every check (29 x 40 image, S = 16, V = 4: a 3 x 3 grid; pointers are never read here)."""
    f = dict(dtype=L.BF16, src=1 << 20, src_bytes=29 * 40, src_pitch=40, col0=0, h=29, w=40, c=1, tile=16, overlap=4, t0=0, n=9,
             lut=1 << 16, dst=L.GanTensor(1 << 22, 9, 16, 16, 1, 8))
    f.update(kw)
    return L.GanTileGatherDesc(**f)


def _blend(L, **kw):
    f = dict(dtype=L.BF16, tiles=L.GanTensor(1 << 22, 9, 16, 16, 1, 8), image=1 << 24, h=29, w=40, c=1, tile=16, overlap=4, t0=0, n=9,
             accumulate=0)
    f.update(kw)
    return L.GanTileBlendDesc(**f)


def test_tile_abi_refuses_bad_descriptors_before_any_launch():
    from gan_amd import _lib as L
    lib = L.load()
    for make, fn, view in ((_gather, lib.gan_tile_gather_u8, 'dst'), (_blend, lib.gan_tile_blend, 'tiles')):
        cls = type(make(L))

        def code(d=None, sub=None, **kw):
            d = make(L, **kw) if d is None else d
            for k, v in (sub or {}).items():
                setattr(getattr(d, view), k, v)
            return fn(C.byref(d), None)

        T = lambda n=9, S=16, c=1, pitch=8, ptr=1 << 22: L.GanTensor(ptr, n, S, S, c, pitch)
        assert fn(None, None) == L.E_ARG
        assert cls().struct_size == C.sizeof(cls)
        d = make(L)
        d.struct_size = C.sizeof(cls) - 4
        assert code(d) == L.E_ARG
        d = make(L)
        d.struct_size = 0
        assert code(d) == L.E_ARG
        assert code(sub=dict(ptr=None)) == L.E_ARG
        for dt in (-1, 3, 7):
            assert code(dtype=dt) == L.E_ARG
        for c in (0, 2, 4):
            assert code(c=c, **{view: T(c=c)}) == L.E_ARG, c
        assert code(overlap=9) == L.E_SHAPE                                       # V > S / 2
        assert code(overlap=-1) == L.E_SHAPE
        assert code(h=15) == L.E_SHAPE and code(w=15) == L.E_SHAPE                # image smaller than a tile
        assert code(h=4097) == L.E_SHAPE
        assert code(tile=20, **{view: T(S=20)}) == L.E_SHAPE                      # S not a multiple of 8
        assert code(tile=8, overlap=0, **{view: T(S=8)}) == L.E_SHAPE
        assert code(t0=1) == L.E_ARG                                              # t0 + n past the 3 x 3 grid
        assert code(t0=8, n=2, **{view: T(n=2)}) == L.E_ARG
        assert code(t0=-1) == L.E_ARG and code(n=0, **{view: T(n=0)}) == L.E_ARG
        assert code(n=4) == L.E_ARG                                               # the view holds 9 tiles
        assert code(sub=dict(h=24)) == L.E_ARG and code(sub=dict(w=8)) == L.E_ARG and code(sub=dict(c=3)) == L.E_ARG
        assert code(c=3, **{view: T(c=3, pitch=2)}) == L.E_ARG                    # pitch < c
        assert code(sub=dict(ptr=(1 << 22) + 1)) == L.E_ARG                       # not element-aligned
        assert code(dtype=L.F32, sub=dict(ptr=(1 << 22) + 2)) == L.E_ARG
    g = lambda **kw: lib.gan_tile_gather_u8(C.byref(_gather(L, **kw)), None)
    assert g(src=None) == L.E_ARG and g(lut=None) == L.E_ARG and g(lut=(1 << 16) + 2) == L.E_ARG
    assert g(col0=-1) == L.E_ARG and g(col0=1) == L.E_ARG                         # the part used leaves the source row
    assert g(src_pitch=39) == L.E_ARG and g(src_pitch=0) == L.E_ARG
    assert g(src_bytes=29 * 40 - 1) == L.E_ARG and g(src_bytes=0) == L.E_ARG      # the last row leaves the buffer
    assert g(src_pitch=100, col0=60, src_bytes=28 * 100 + 99) == L.E_ARG          # a right half: one byte short
    b = lambda **kw: lib.gan_tile_blend(C.byref(_blend(L, **kw)), None)
    assert b(image=None) == L.E_ARG and b(image=(1 << 24) + 2) == L.E_ARG
    assert b(accumulate=2) == L.E_ARG and b(accumulate=-1) == L.E_ARG


def test_header_binding_and_integration_snippet_of_the_tile_descriptors_agree():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_binding
    from gan_amd import _lib as L
    structs = gen_binding.parse_structs()
    for name in ('GanTileGatherDesc', 'GanTileBlendDesc'):
        fields = structs[name]
        want = [(f, getattr(C, t[2:]) if t.startswith('C.') else getattr(L, t)) for f, t in fields]
        assert list(getattr(L, name)._fields_) == want and fields[0] == ('struct_size', 'C.c_uint32')
    assert {'gan_tile_grid', 'gan_tile_gather_u8', 'gan_tile_blend'} <= set(L.SYMBOLS)
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    first = re.search(r"```python\nimport ctypes as C\n(.*?)```", text, flags=re.S).group(1)
    code = re.search(r"```python\n(# --- generated from include/gan_amd.h by tools/gen_binding.py GanTileBlendDesc ---\n.*?)```", text,
                     flags=re.S).group(1)
    gen = code[:code.index('# --- end of generated part')]
    assert gen.split('\n', 1)[1].strip() == gen_binding.ctypes_source(['GanTileBlendDesc']).strip()
    ns = {}
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        exec("import ctypes as C\n" + first + code, ns)          # loads the library, binds the symbols
    finally:
        os.chdir(cwd)
    assert C.sizeof(ns['GanTileBlendDesc']) == C.sizeof(L.GanTileBlendDesc) and callable(ns['blend_tiles'])
    d = ns['GanTileBlendDesc'](struct_size=C.sizeof(ns['GanTileBlendDesc']) - 4)
    assert ns['lib'].gan_tile_blend(C.byref(d), None) == -1
    assert ns['tile_grid'](512, 640, 256, 64) == (3, 3)


def test_cli_flags_and_defaults():
    from gan_amd import pix2pix
    train = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']
    pred = ['--data', 'd', '--output', 'o', '--predict', '--weights', 'w']
    o = pix2pix.parse_opt(train)
    assert o.predict_resolution == 'resized' and o.tile_overlap == 64
    assert pix2pix.parse_opt(train + ['--img-size', '512']).tile_overlap == 128
    o = pix2pix.parse_opt(pred)
    assert o.predict_resolution == 'resized' and o.tile_overlap == 64 and o.predict_training == 'true'
    o = pix2pix.parse_opt(pred + ['--predict-resolution', 'native', '--predict-training', 'false', '--tile-overlap', '128'])
    assert o.predict_resolution == 'native' and o.tile_overlap == 128
    assert pix2pix.parse_opt(pred + ['--tile-overlap', '0']).tile_overlap == 0
    with pytest.raises(SystemExit):           # tiles are only meaningful in inference mode
        pix2pix.parse_opt(pred + ['--predict-resolution', 'native'])
    with pytest.raises(SystemExit):
        pix2pix.parse_opt(pred + ['--predict-resolution', 'native', '--predict-training', 'true'])
    with pytest.raises(SystemExit):
        pix2pix.parse_opt(train + ['--predict-resolution', 'native', '--predict-training', 'false'])
    for v in ('129', '-1'):
        with pytest.raises(SystemExit):
            pix2pix.parse_opt(pred + ['--tile-overlap', v])
    with pytest.raises(SystemExit):
        pix2pix.parse_opt(pred + ['--img-size', '512', '--tile-overlap', '257'])
    with pytest.raises(SystemExit):
        pix2pix.parse_opt(pred + ['--predict-resolution', 'full'])
