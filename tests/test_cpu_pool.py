"""Image history pool, the parts that need no GPU: the decision traces of the numpy reference, the entry
point's declaration and refusals, the --pool-size flag."""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

from gan_amd import _lib as L
from tests import pool_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(traces):
    return Counter(kind for t in traces for kind, _ in t)


def test_decision_traces_have_the_quoted_figures():
    t = R.run_trace(3, 2, 123, R.STREAM_X, 6)
    assert _counts(t) == {'fill': 3, 'swap': 7, 'keep': 2}
    assert [k for k, _ in t[1]] == ['fill', 'swap']                    # launch 2: a fill and a swap in one batch
    t = R.run_trace(1, 4, 123, R.STREAM_Y, 6)
    assert (_counts(t)['swap'], _counts(t)['keep']) == (9, 14)
    assert sum(R.same_slot_swaps(x) for x in t) == 3
    assert sum(R.same_slot_swaps(x) for x in R.run_trace(1, 4, 123, R.STREAM_X, 6)) == 5
    for sid in (R.STREAM_Y, R.STREAM_X):
        assert sum(R.same_slot_swaps(x) for x in R.run_trace(4, 16, 123, sid, 6)) == 6


def test_the_gpu_parameter_sets_reach_every_branch():
    """What keeps tests/test_gpu_pool.py honest, asserted on the reference alone."""
    traces = [t for P, B in R.GPU_CASES for sid in (R.STREAM_Y, R.STREAM_X) for t in R.run_trace(P, B, R.GPU_SEED, sid, R.GPU_LAUNCHES)]
    assert any({'fill', 'swap'} <= {k for k, _ in t} for t in traces)
    assert any(k == 'keep' for t in traces for k, _ in t)
    assert any(R.same_slot_swaps(t) for t in traces)
    assert all(0 <= j < P for P, B in R.GPU_CASES for t in R.run_trace(P, B, R.GPU_SEED, R.STREAM_Y, R.GPU_LAUNCHES)
               for k, j in t if k != 'keep')


def test_reference_query_is_the_sequential_loop():
    """Two swaps of one slot in a batch: the second one hands out the FIRST image of this batch, not the old slot content."""
    P, B, sid = 1, 4, R.STREAM_X
    imgs = np.arange(B * 2, dtype=np.float32).reshape(B, 2) + 100
    pool, state = np.zeros((P, 2), np.float32), (0, 0)
    out, pool, state, trace = R.query(imgs, pool, state, 123, sid)          # launch 0: fill, keep, swap, keep
    assert [k for k, _ in trace] == ['fill', 'keep', 'swap', 'keep'] and state == (1, 1)
    assert (out[2] == imgs[0]).all() and (pool[0] == imgs[2]).all() and (out[[0, 1, 3]] == imgs[[0, 1, 3]]).all()
    imgs2 = imgs + 50
    out, pool2, state, trace = R.query(imgs2, pool, state, 123, sid)        # launch 1: four swaps of slot 0
    assert [k for k, _ in trace] == ['swap'] * 4 and state == (1, 2)
    assert (out[0] == pool[0]).all() and (out[1:] == imgs2[:-1]).all() and (pool2[0] == imgs2[3]).all()


def test_header_declares_and_the_binding_lists_the_entry_point_and_its_struct():
    hdr = open(os.path.join(ROOT, 'include', 'gan_amd.h')).read()
    assert re.search(r'\bint gan_pool_exchange\(const GanPoolDesc\* d, gan_stream_t stream\);', hdr)
    assert re.search(r'typedef struct GanPoolDesc \{.*?\} GanPoolDesc;', hdr, flags=re.S)
    assert L.SYMBOLS['gan_pool_exchange'] == (C.c_int, [C.POINTER(L.GanPoolDesc), C.c_void_p])
    assert [f for f, _ in L.GanPoolDesc._fields_] == ['struct_size', 'dtype', 'src', 'dst', 'pool', 'capacity', 'stream_id', 'seed', 'state']
    assert hasattr(L.load(), 'gan_pool_exchange')


def test_every_bad_argument_is_refused_before_any_launch():
    """No device memory is behind these pointers and no GPU need be present: the error code comes back before anything is enqueued."""
    lib = L.load()
    A = 4096                                     # a non-NULL, 16-byte aligned address that is never dereferenced

    def call(src=None, dst=None, **fields):
        view = lambda **kw: L.GanTensor(**{**dict(ptr=A, n=2, h=8, w=8, c=3, pitch=8), **kw})
        d = L.GanPoolDesc(L.BF16, view(**(src or {})), view(**(dst or {})), A, 3, 32, 123, A)
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.gan_pool_exchange(C.byref(d), None)

    assert lib.gan_pool_exchange(None, None) == L.E_ARG
    for size in (0, C.sizeof(L.GanPoolDesc) - 8, C.sizeof(L.GanPoolDesc) + 8):
        assert call(struct_size=size) == L.E_ARG
    assert call(dtype=3) == L.E_ARG and call(dtype=-1) == L.E_ARG
    assert call(capacity=0) == L.E_ARG and call(capacity=-5) == L.E_ARG          # P = 0
    assert call(pool=None) == L.E_ARG and call(state=None) == L.E_ARG
    assert call(src=dict(ptr=None)) == L.E_ARG and call(dst=dict(ptr=None)) == L.E_ARG
    for field, bad in (('n', 3), ('h', 9), ('w', 4), ('c', 1)):                  # mismatched views
        assert call(dst={field: bad}) == L.E_ARG, field
        assert call(src={field: bad}) == L.E_ARG, field
    assert call(src=dict(n=0), dst=dict(n=0)) == L.E_ARG
    assert call(src=dict(pitch=2)) == L.E_ARG and call(dst=dict(pitch=2)) == L.E_ARG      # pitch < c
    assert call(src=dict(ptr=A + 1)) == L.E_ARG and call(pool=A + 1) == L.E_ARG and call(state=A + 2) == L.E_ARG
    assert call(dtype=L.F32, dst=dict(ptr=A + 2)) == L.E_ARG
    big = dict(h=1 << 15, w=1 << 15, pitch=8)                                    # 2^30 pixels of pitch 8: past 32-bit offsets
    assert call(src=big, dst=big) == L.E_SHAPE


# ---- command line ---------------------------------------------------------------------------------------------------------------------
CG = ['--input-images', 'x', '--target-images', 'y', '--output', 'o', '--train', '--epochs', '1']


def test_pool_size_flag():
    from gan_amd import cycle_gan
    o = cycle_gan.parse_opt(CG)
    assert o.pool_size == 0 and isinstance(o.pool_size, int)                     # the default: no pool
    from gan_amd.runner import config_of
    assert config_of(o)['pool_size'] == 0 and config_of(o)['input_images'] == 'x'
    o = cycle_gan.parse_opt(CG + ['--pool-size', '50'])
    assert o.pool_size == 50 and config_of(o)['pool_size'] == 50                 # config_of(opt) is the model's config (runner.drive)
    assert 'pool_size' not in vars(o)                                            # ... beside the flags both drivers are compared on


def test_negative_pool_size_is_refused(capsys):
    from gan_amd import cycle_gan
    with pytest.raises(SystemExit):
        cycle_gan.parse_opt(CG + ['--pool-size', '-1'])
    assert '--pool-size -1 is negative' in capsys.readouterr().err


def test_pix2pix_does_not_know_the_flag(capsys):
    from gan_amd import pix2pix
    base = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']
    assert not hasattr(pix2pix.parse_opt(base), 'pool_size')
    with pytest.raises(SystemExit):
        pix2pix.parse_opt(base + ['--pool-size', '2'])
    assert 'unrecognized arguments: --pool-size' in capsys.readouterr().err
