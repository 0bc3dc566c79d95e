"""Image preprocessing on the host: Preprocess.apply_host against the scalar restatement of
tests/preprocess_ref.py, hand-checked known answers, the independence of the two halves of a pair, header / binding /
INTEGRATION.md snippet, the command line and --resume.  Every comparison is exact."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from gan_amd.preprocess import Preprocess, blur_radius, blur_taps, parse_stages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_ref as R  # noqa: E402

CHAINS = ('clahe', 'blur', 'sharpen', 'clahe,blur,sharpen')


def _image(kind, h, w, c, seed):
    rng = np.random.default_rng(seed)
    if kind == 'random':
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == 'constant':
        return np.full((h, w, c), 93, np.uint8)
    if kind == 'two':
        return np.where(rng.random((h, w, c)) < 0.3, 200, 17).astype(np.uint8)
    return np.broadcast_to(((np.arange(w)[None, :] * 3 + np.arange(h)[:, None]) % 256).astype(np.uint8)[..., None], (h, w, c)).copy()


# (image kind, H, W, c, region (y0, x0, h, w), clip, grid, sigma)
CASES = [
    ('random', 41, 64, 1, (2, 7, 37, 53), 1.0, 15, 0.5),           # non-zero x0, a pitch larger than the width
    ('two', 37, 53, 1, (0, 0, 37, 53), 40.0, 4, 1.0),
    ('ramp', 37, 53, 3, (0, 0, 37, 53), 0.0, 1, 0.5),
    ('random', 16, 16, 1, (0, 0, 16, 16), 1.0, 16, 0.5),            # grid == width: no padding, tiles of one pixel
    ('constant', 16, 16, 3, (0, 0, 16, 16), 1.0, 4, 1.0),
    ('random', 16, 16, 1, (0, 0, 16, 16), 40.0, 15, 1.5),           # padded to 30 x 30
    ('random', 15, 31, 1, (0, 0, 15, 31), 1.0, 15, 0.5),            # tiles of 3 x 1: int(clip * area / 256) == 0, the limit is 1
    ('two', 15, 31, 3, (0, 0, 15, 31), 0.0, 4, 0.5),
    ('ramp', 20, 40, 1, (3, 9, 15, 31), 40.0, 15, 1.0),
]


@pytest.mark.parametrize('case', CASES, ids=[f"{c[0]}-{c[4][2]}x{c[4][3]}-c{c[3]}-g{c[6]}-clip{c[5]:g}" for c in CASES])
def test_apply_host_equals_the_scalar_reference(case):
    kind, H, W, c, region, clip, grid, sigma = case
    img = _image(kind, H, W, c, seed=H + 3 * W + c)
    for chain in CHAINS:
        got = Preprocess(chain, clip, grid, sigma).apply_host(img, [region])
        want = R.apply(img, [region], chain.split(','), clip, grid, sigma)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (chain, np.argwhere(got != want)[:4])
        y0, x0, h, w = region
        mask = np.ones(img.shape, bool)
        mask[y0:y0 + h, x0:x0 + w] = False
        assert np.array_equal(got[mask], img[mask])                 # nothing outside the region moves


def test_tap_tables():
    """sigma 0.5: r = (rint(4) | 1) // 2 = 2; w = (1, e^-2, e^-8) = (1, .135335, .000335), sum 1.271341; 256 w / sum = (.., 27.25,
    0.068) -> (27, 0), centre 256 - 54 = 202.  sigma 1.0: r = (7 | 1) // 2 = 3; w = (1, .606531, .135335, .011109), sum 2.505950;
    256 w / sum = (.., 61.96, 13.83, 1.13) -> (62, 14, 1), centre 256 - 154 = 102."""
    assert blur_taps(0.5) == (0, 27, 202, 27, 0) and blur_radius(0.5) == 2
    assert blur_taps(1.0) == (1, 14, 62, 102, 62, 14, 1) and blur_radius(1.0) == 3
    assert blur_radius(1.5) == 5 and sum(blur_taps(1.5)) == 256 and len(blur_taps(1.5)) == 11
    assert tuple(R.blur_taps(0.5)) == blur_taps(0.5) and tuple(R.blur_taps(1.0)) == blur_taps(1.0) and tuple(R.blur_taps(1.5)) == blur_taps(1.5)
    for s in (0.0, -1.0, 1.51, float('nan')):
        with pytest.raises(ValueError):
            Preprocess('blur', sigma=s)


def test_constant_images_are_fixed_points_of_blur_and_sharpen():
    img = np.full((9, 12, 3), 201, np.uint8)
    for chain in ('blur', 'sharpen', 'blur,sharpen'):
        for sigma in (0.5, 1.0, 1.5):
            assert np.array_equal(Preprocess(chain, sigma=sigma).apply_host(img), img)      # 256 * 256 * v + 32768 >> 16 = v; 5v - 4v = v


def test_constant_image_under_clahe():
    """16 x 16 of value 93, grid 2, clip 1.0: tiles of 8 x 8, area 64, limit max(int(64 / 256), 1) = 1.  The one occupied bin holds
    64: clipped = 63, the bin keeps 1.  batch = 63 // 256 = 0, residual = 63, step = 256 // 63 = 4: the bins 0, 4, ..., 248 (63 of
    them) gain one.  Up to bin 93 that is 0, 4, ..., 92 = 24 bins, plus the 1 of bin 93: cumsum[93] = 25 and
    lut[93] = rint(25 * 255 / 64) = rint(99.609) = 100 in every tile, so every pixel becomes 100.  Without clipping (clip 0)
    cumsum[93] = 64 = area: 255."""
    img = np.full((16, 16, 1), 93, np.uint8)
    assert np.array_equal(Preprocess('clahe', 1.0, 2).apply_host(img), np.full_like(img, 100))
    assert np.array_equal(Preprocess('clahe', 0.0, 2).apply_host(img), np.full_like(img, 255))
    assert np.array_equal(R.apply(img, [(0, 0, 16, 16)], ['clahe'], 1.0, 2), np.full_like(img, 100))


def test_8x8_grid_2_by_hand():
    """Columns 0 .. 3 hold 10, columns 4 .. 7 hold 200; grid 2, clip 1.0: tiles of 4 x 4, area 16, limit 1, scale 255 / 16 = 15.9375.
    A tile of the left column: bin 10 holds 16 -> keeps 1, clipped 15, batch 0, residual 15, step 256 // 15 = 17: bins 0, 17, ...,
    238 gain one.  L[10] = rint(15.9375 * (1 [bin 0] + 1 [bin 10])) = rint(31.875) = 32;
    L[200] = rint(15.9375 * (12 [bins 0 .. 187] + 1 [bin 10])) = rint(207.19) = 207.
    A tile of the right column (bin 200 keeps 1): R[10] = rint(15.9375 * 1) = 16; R[200] = rint(15.9375 * (12 + 1)) = 207.
    Both tile rows are alike, so y does not matter.  txf = x / 4 - 0.5 = -.5, -.25, 0, .25, .5, .75, 1, 1.25:
      x = 0, 1: tx1 = -1 -> 0, tx2 = 0: L[10] = 32;  x = 2: xa = 0: L[10] = 32;  x = 3: .75 L[10] + .25 R[10] = 24 + 4 = 28;
      x = 4: .5 L[200] + .5 R[200] = 207;  x = 5: .25 L[200] + .75 R[200] = 207;  x = 6, 7: tx1 = tx2 = 1: R[200] = 207."""
    img = np.zeros((8, 8, 1), np.uint8)
    img[:, :4], img[:, 4:] = 10, 200
    want = np.broadcast_to(np.array([32, 32, 32, 28, 207, 207, 207, 207], np.uint8)[None, :, None], (8, 8, 1))
    assert np.array_equal(Preprocess('clahe', 1.0, 2).apply_host(img), want)
    assert np.array_equal(R.apply(img, [(0, 0, 8, 8)], ['clahe'], 1.0, 2), want)


def test_sharpen_and_blur_by_hand():
    """One bright pixel of 100 at the centre of a 5 x 5 of zeros.  sharpen: centre 500 -> 255, its four neighbours -100 -> 0.
    blur sigma 0.5, taps (27, 202, 27): centre (202 * 202 * 100 + 32768) >> 16 = 62, edge neighbours (27 * 202 * 100 + 32768) >> 16 = 8,
    diagonal (27 * 27 * 100 + 32768) >> 16 = 1."""
    img = np.zeros((5, 5, 1), np.uint8)
    img[2, 2] = 100
    s = Preprocess('sharpen').apply_host(img)[..., 0]
    assert s[2, 2] == 255 and s.sum() == 255
    b = Preprocess('blur', sigma=0.5).apply_host(img)[..., 0]
    assert b[2, 2] == 62 and b[1, 2] == b[2, 1] == b[3, 2] == b[2, 3] == 8 and b[1, 1] == b[3, 3] == 1 and b[0].sum() == 0
    # reflect-101: a bright corner pixel is seen once by itself, and its neighbours see it once
    img = np.zeros((4, 4, 1), np.uint8)
    img[0, 0] = 100
    b = Preprocess('blur', sigma=0.5).apply_host(img)[..., 0]
    assert b[0, 0] == 62 and b[0, 1] == b[1, 0] == 8 and b[1, 1] == 1


def test_the_halves_of_a_pair_are_independent():
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (33, 71, 3), dtype=np.uint8)              # halves of 35 and 36 columns
    a, b = (0, 0, 33, 35), (0, 35, 33, 36)
    for chain in CHAINS:
        pre = Preprocess(chain, 1.0, 15, 0.5)
        alone = pre.apply_host(np.ascontiguousarray(img[:, :35]))
        only_a = pre.apply_host(img, [a])
        both = Preprocess('clahe', 2.0, 4).apply_host(only_a, [b])
        for got in (only_a, both):
            assert np.array_equal(got[:, :35], alone), chain             # half A alone == half A inside the pair
        assert np.array_equal(only_a[:, 35:], img[:, 35:])               # the other half stays
        assert np.array_equal(both[:, 35:], Preprocess('clahe', 2.0, 4).apply_host(np.ascontiguousarray(img[:, 35:])))
    # a region with padding around it, in a larger array: everything else stays
    big = rng.integers(0, 256, (40, 90, 1), dtype=np.uint8)
    got = Preprocess('clahe,blur,sharpen').apply_host(big, [(3, 11, 30, 40)])
    mask = np.ones(big.shape, bool)
    mask[3:33, 11:51] = False
    assert np.array_equal(got[mask], big[mask]) and not np.array_equal(got, big)
    assert np.array_equal(got[3:33, 11:51], Preprocess('clahe,blur,sharpen').apply_host(np.ascontiguousarray(big[3:33, 11:51])))


def test_small_regions_and_bad_parameters_are_refused():
    img = np.zeros((14, 40, 1), np.uint8)
    with pytest.raises(ValueError, match='smaller'):
        Preprocess('clahe', grid=15).apply_host(img)
    with pytest.raises(ValueError, match='smaller'):
        Preprocess('blur', sigma=1.5).apply_host(img[:5])
    with pytest.raises(ValueError, match='outside'):
        Preprocess('sharpen').apply_host(img, [(0, 30, 14, 11)])
    for kw in (dict(grid=0), dict(grid=33), dict(grid=2.5), dict(clip=-1.0), dict(clip=float('inf')), dict(clip=float('nan'))):
        with pytest.raises(ValueError):
            Preprocess('clahe', **kw)
    with pytest.raises(ValueError):
        parse_stages('clahe,median')
    with pytest.raises(ValueError):
        parse_stages('blur,blur')


def test_canonical_string_round_trips():
    p = Preprocess(('sharpen', 'clahe'), 2, 8, 1.0)
    assert p.stages == ('clahe', 'sharpen') and str(p) == 'clahe,sharpen:clip=2.0,grid=8,sigma=1.0'
    assert Preprocess.parse(str(p)) == p and str(Preprocess.parse('blur')) == 'blur:clip=1.0,grid=15,sigma=0.5'
    assert str(Preprocess()) == '' and not Preprocess() and Preprocess.parse('') == Preprocess() and bool(p)
    assert Preprocess('clahe', clip=0.1).clip == float(np.float32(0.1))        # held as the float the device receives
    assert np.array_equal(Preprocess().apply_host(np.arange(12, dtype=np.uint8).reshape(3, 4)), np.arange(12, dtype=np.uint8).reshape(3, 4))


# ---- header, binding, snippet -----------------------------------------------------------------------------------------------------
def test_header_binding_and_integration_snippet_agree():
    from gan_amd import _lib as L
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_binding
    structs = gen_binding.parse_structs()
    for name in ('GanPreRegion', 'GanPreprocessDesc'):
        want = [(f, getattr(C, t[2:]) if t.startswith('C.') else getattr(L, t)) for f, t in structs[name]]
        assert list(getattr(L, name)._fields_) == want, name
    assert structs['GanPreprocessDesc'][0] == ('struct_size', 'C.c_uint32')
    hdr = open(os.path.join(ROOT, 'include', 'gan_amd.h')).read()
    for proto in (r'size_t gan_preprocess_workspace_bytes\(const GanPreprocessDesc\* d\);',
                  r'int gan_preprocess_u8\(const GanPreprocessDesc\* d, gan_stream_t stream\);',
                  r'GAN_PREPROCESS_MAX_REGIONS = 64', r'GAN_PRE_CLAHE = 1, GAN_PRE_BLUR = 2, GAN_PRE_SHARPEN = 4'):
        assert re.search(proto, hdr), proto
    assert (L.PREPROCESS_MAX_REGIONS, L.PRE_CLAHE, L.PRE_BLUR, L.PRE_SHARPEN) == (64, 1, 2, 4)
    assert L.SYMBOLS['gan_preprocess_u8'] == (C.c_int, [C.POINTER(L.GanPreprocessDesc), C.c_void_p])
    assert L.SYMBOLS['gan_preprocess_workspace_bytes'] == (C.c_size_t, [C.POINTER(L.GanPreprocessDesc)])
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    first = re.search(r"```python\nimport ctypes as C\n(.*?)```", text, flags=re.S).group(1)
    code = re.search(r"```python\n(# --- generated from include/gan_amd.h by tools/gen_binding.py GanPreRegion GanPreprocessDesc ---\n.*?)```",
                     text, flags=re.S).group(1)
    gen = code[:code.index('# --- end of generated part')]
    assert gen.split('\n', 1)[1].strip() == gen_binding.ctypes_source(['GanPreRegion', 'GanPreprocessDesc']).strip()
    ns = {}
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        exec("import ctypes as C\n" + first + code, ns)
    finally:
        os.chdir(cwd)
    assert C.sizeof(ns['GanPreprocessDesc']) == C.sizeof(L.GanPreprocessDesc) and callable(ns['preprocess_regions'])
    d = ns['GanPreprocessDesc'](struct_size=C.sizeof(ns['GanPreprocessDesc']) - 8)
    assert ns['lib'].gan_preprocess_u8(C.byref(d), None) == -1
    assert 'preprocess.hip' in open(os.path.join(ROOT, 'gan_amd', 'csrc', 'Makefile')).read()


def test_workspace_query_and_refusals_without_a_gpu():
    """The checks come before any launch and before the buffers are looked at, so the size query answers them without a GPU."""
    from gan_amd import _lib as L
    lib = L.load()

    def need(pre, regions, c=1, **fields):
        d, keep = pre.descriptor(c, regions)
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.gan_preprocess_workspace_bytes(C.byref(d))

    full = Preprocess('clahe,blur,sharpen', 1.0, 8, 0.5)
    assert need(full, [(0, 48, 40, 48)]) == 8 * 8 * 256 + 40 * 48
    assert need(Preprocess('clahe', grid=15), [(0, 640, 512, 640)]) == 225 * 256                  # in place: tables only
    assert need(Preprocess('sharpen'), [(0, 150, 10, 50)], c=3) == 10 * 152                       # dense rows, rounded up to 4 bytes
    assert need(full, [(0, 48, 40, 48)] * 65) == 64 * (8 * 8 * 256 + 40 * 48)                     # the larger of the two groups
    assert lib.gan_preprocess_workspace_bytes(None) == 0
    for bad in (dict(n=0), dict(c=2), dict(stages=0), dict(stages=9), dict(grid=0), dict(grid=33), dict(sigma=0.0), dict(sigma=1.6),
                dict(clip=-1.0), dict(clip=float('inf')), dict(struct_size=8)):
        assert need(full, [(0, 48, 40, 48)], **bad) == 0, bad
    assert need(full, [(0, 47, 40, 48)]) == 0 and need(full, [(0, 48, 7, 48)]) == 0 and need(full, [(0, 48, 40, 7)]) == 0
    assert need(Preprocess('blur', sigma=1.5), [(0, 48, 5, 48)]) == 0 and need(Preprocess('blur', sigma=1.5), [(0, 48, 6, 48)]) > 0


# ---- command line, config, resume ---------------------------------------------------------------------------------------------------
BASE = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']


def test_cli_defaults_and_validation(capsys):
    from gan_amd import pix2pix
    from gan_amd.runner import config_of
    o = pix2pix.parse_opt(BASE)
    cfg = config_of(o)
    assert (cfg['preprocess_input'], cfg['preprocess_target'], cfg['clahe_clip'], cfg['clahe_grid'], cfg['blur_sigma']) == ('', '', 1.0, 15, 0.5)
    assert 'preprocess_input' not in vars(o) and 'clahe_grid' not in vars(o)          # beside the flags both drivers are compared on
    o = pix2pix.parse_opt(BASE + ['--preprocess-input', 'sharpen, clahe,blur', '--preprocess-target', 'clahe', '--clahe-clip', '2',
                                  '--clahe-grid', '8', '--blur-sigma', '1.0'])
    cfg = config_of(o)
    assert cfg['preprocess_input'] == 'clahe,blur,sharpen' and cfg['preprocess_target'] == 'clahe'      # canonical order
    assert (cfg['clahe_clip'], cfg['clahe_grid'], cfg['blur_sigma']) == (2.0, 8, 1.0)
    o = pix2pix.parse_opt(['--data', 'd', '--output', 'o', '--predict', '--weights', 'w', '--preprocess-input', 'clahe'])
    assert config_of(o)['preprocess_input'] == 'clahe'                                                  # --predict carries them too
    for bad in (['--preprocess-input', 'clahe,median'], ['--preprocess-target', 'blur,blur'], ['--clahe-grid', '0'], ['--clahe-grid', '33'],
                ['--blur-sigma', '0'], ['--blur-sigma', '1.6'], ['--blur-sigma', 'nan'], ['--clahe-clip', '-1'], ['--clahe-clip', 'inf']):
        with pytest.raises(SystemExit):
            pix2pix.parse_opt(BASE + bad)
        assert bad[0] in capsys.readouterr().err
    with pytest.raises(SystemExit):
        pix2pix.parse_opt(['--help'])
    out = ' '.join(capsys.readouterr().out.split())
    assert 'per-channel equalisation' in out and 'no colour-space conversion' in out


def test_model_without_the_flags_reads_files_as_before(tmp_path):
    """A config without the keys (a model built from vars(opt), an older config.json) has no preprocessing."""
    from PIL import Image
    from gan_amd import data as D
    from gan_amd.pix2pix import Pix2Pix
    rng = np.random.default_rng(1)
    f = str(tmp_path / 'a.png')
    Image.fromarray(rng.integers(0, 256, (32, 70), dtype=np.uint8)).save(f)

    class Stub(Pix2Pix):
        def __init__(self, config):
            self.config, self._preprocessors = config, None

    plain = Stub({'channels': 1, 'input_img_orient': 'left', 'img_size': 256})
    a, b = plain.split_img(f)
    wa, wb = D.split_img(D.load(f, 1), 'left')
    assert np.array_equal(a, wa) and np.array_equal(b, wb) and not any(plain.preprocessors())
    for orient in ('left', 'right'):
        m = Stub({'channels': 1, 'input_img_orient': orient, 'img_size': 256, 'preprocess_input': 'clahe,blur,sharpen',
                  'preprocess_target': 'clahe', 'clahe_clip': 1.0, 'clahe_grid': 15, 'blur_sigma': 0.5})
        a, b = m.split_img(f)
        img = D.decode(f, 1)
        halves = (img[:, :35], img[:, 35:]) if orient == 'left' else (img[:, 35:], img[:, :35])
        assert a.dtype == np.float32 and np.array_equal(a, Preprocess('clahe,blur,sharpen').apply_host(np.ascontiguousarray(halves[0])).astype(np.float32))
        assert np.array_equal(b, Preprocess('clahe').apply_host(np.ascontiguousarray(halves[1])).astype(np.float32))


def test_resume_refuses_other_preprocessing_by_name(tmp_path):
    from gan_amd import tfbundle
    from gan_amd import train_state as T
    from tests.test_cpu_resume import CONFIG, _bundle
    assert T.run_config(CONFIG)['preprocess_input'] == '' and T.run_config(CONFIG)['clahe_grid'] == 15.0
    with_pre = {**CONFIG, 'preprocess_input': 'clahe,blur,sharpen', 'preprocess_target': 'clahe'}
    prefix = _bundle(tmp_path / 'p', with_pre)
    assert T.check_resume(prefix, with_pre) == prefix
    for key, other in (('preprocess_input', 'clahe'), ('preprocess_input', ''), ('preprocess_target', ''), ('clahe_clip', 2.0),
                       ('clahe_grid', 8), ('blur_sigma', 1.0)):
        with pytest.raises(T.ResumeRefused) as e:
            T.check_resume(prefix, {**with_pre, key: other})
        assert f' {key} ' in str(e.value), key
    # a checkpoint written before the keys existed resumes with the defaults, and refuses a run that preprocesses
    stored = T.run_config(CONFIG)
    for k in ('preprocess_input', 'preprocess_target', 'clahe_clip', 'clahe_grid', 'blur_sigma'):
        del stored[k]
    os.makedirs(tmp_path / 'old')
    old = tfbundle.write_bundle(os.path.join(str(tmp_path / 'old'), 'ckpt-1'),
                                {'generator/layer_with_weights-15/bias/.ATTRIBUTES/VARIABLE_VALUE': np.zeros(1, np.float32),
                                 'train_state/epoch': np.array(2, np.int64), 'train_state/config': T._json_array(stored)})
    assert T.check_resume(old, CONFIG) == old
    assert T.check_resume(old, {**CONFIG, 'preprocess_input': '', 'clahe_clip': 1.0, 'clahe_grid': 15, 'blur_sigma': 0.5}) == old
    with pytest.raises(T.ResumeRefused) as e:
        T.check_resume(old, with_pre)
    assert ' preprocess_input ' in str(e.value)
