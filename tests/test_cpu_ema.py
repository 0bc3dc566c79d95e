"""CPU tests of the generator weight average (gan_ema_update, gan_amd/ema.py, --ema-decay): the fp64 reference and its gate
(tests/ema_ref.py) on a float32 model of the kernel and on the named wrong variants, the argument checks of the entry point, the
header / binding agreement, the CLI flags and the checkpoint object - no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import ema_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_reference_first_step_from_a_seeded_shadow():
    """The shadow is seeded with the weights: a first update towards moved weights goes (1 - d_t) of the way, towards unmoved
    ones nowhere."""
    w0 = np.array([1.0, -2.0, 0.5, 0.0], F32)
    w1 = np.array([2.0, -2.0, 0.0, 4.0], F32)
    d = F32(0.75)
    assert np.array_equal(R.reference(w0, w1, d), np.array([1.25, -2.0, 0.375, 1.0]))          # s + (w - s) / 4, exact
    assert np.array_equal(R.reference(w0, w0, d), w0.astype(np.float64))
    t1 = R.decay_at(0.75, 1)                                                                    # warm-up, step 1: 2 / 11
    assert t1 == 2.0 / 11.0
    assert np.allclose(R.reference(w0, w1, F32(t1)), w0 + (w1.astype(np.float64) - w0) * (9.0 / 11.0), rtol=1e-7, atol=0)


def test_recurrence_matches_the_closed_form_over_five_steps():
    rng = np.random.default_rng(3)
    for decay in (0.999, 0.5):
        s0 = rng.standard_normal(257)
        ws = [rng.standard_normal(257) for _ in range(5)]
        d = float(F32(decay))
        s = s0.copy()
        for w in ws:
            s = s + (w - s) * (1.0 - d)
        assert np.allclose(s, R.closed_form(s0, ws, decay), rtol=1e-12, atol=1e-14)
        # ... and the float32 model stays within the gate of the fp64 recurrence, step by step
        s32 = s0.astype(F32)
        for w in ws:
            w32 = w.astype(F32)
            new, du = R.model_f32(s32, w32, decay)
            assert R.passes(s32, w32, new, du, decay)
            s32 = new


def test_warm_up_decay_values():
    d = float(F32(0.999))
    assert R.decay_at(0.999, 0) == 0.1
    assert R.decay_at(0.999, 1) == 2.0 / 11.0
    assert R.decay_at(0.999, 10) == 11.0 / 20.0
    # the crossover: (1 + t) / (10 + t) = 0.999 at t = 8990 exactly; the fp32 0.999 lies a little above the real number, so the
    # ratio still wins there (by 1.3e-8, a fifth of an fp32 ulp) and the decay from the next step on
    assert (1 + 8990) * 1000 == 999 * (10 + 8990)
    assert 0.999 < d < 0.999 + 2.0 ** -25
    assert R.decay_at(0.999, 8989) == 8990.0 / 8999.0 < R.decay_at(0.999, 8990) == 8991.0 / 9000.0 < d
    assert R.decay_at(0.999, 8991) == d < 8992.0 / 9001.0
    assert F32(R.decay_at(0.999, 8990)) == F32(0.999)                     # ... and rounds to the same fp32 number
    assert R.decay_at(0.999, 10 ** 6) == d
    assert R.decay_at(0.999) == d and R.decay_at(0.5, 100000) == 0.5
    for t in (0, 1, 10, 8990, 10 ** 6):
        assert R.decay_ok(F32(R.decay_at(0.999, t)), 0.999, t)
    assert not R.decay_ok(F32(0.55) + F32(2.0 ** -22), 0.999, 10)          # two ulps off


def test_gate_passes_the_float32_model_of_the_kernel():
    for count in (4, 64, 1028):
        s, w = R.planted(count, seed=count)
        for decay in (0.999, 0.5):
            for step in (None, 1, 10, 8990, 100000):
                got, du = R.model_f32(s, w, decay, step)
                assert R.decay_ok(du, decay, step)
                bad = R.element_failures(s, w, got, du)
                assert bad.size == 0, (count, decay, step, bad[:5], s[bad[:5]], w[bad[:5]], got[bad[:5]])
                assert R.worst_ratio(s, w, got, du) <= 1.0
    # the IEEE exception the bitwise rule leaves out: -0 against -0 gives +0
    got, du = R.model_f32(F32([-0.0]), F32([-0.0]), 0.5)
    assert got.view(np.uint32)[0] == 0 and not R.bitwise_rule_mask(F32([-0.0]), F32([-0.0]))[0]
    assert R.bitwise_rule_mask(F32([0.0, 1.5]), F32([0.0, 1.5])).all()


def _variant(name, s, w, decay, step):
    """Wrong kernels: -> (new shadow, reported d_t)."""
    s, w = np.asarray(s, F32), np.asarray(w, F32)
    d = F32(R.decay_at(decay, step))
    t = None if step is None else float(step)
    if name == 'decay and 1 - decay swapped':
        return (s + (w - s) * d).astype(F32), d
    if name == 'warm-up ignored':
        d = F32(decay)
    elif name == 't - 1 in place of t':
        d = F32(min(float(F32(decay)), t / (9.0 + t)))
    elif name == 'max in place of min':
        d = F32(max(float(F32(decay)), (1.0 + t) / (10.0 + t)))
    elif name == 'shadow and param swapped':
        return (w + (s - w) * (F32(1.0) - d)).astype(F32), d
    return (s + (w - s) * (F32(1.0) - d)).astype(F32), d


@pytest.mark.parametrize('name', ['decay and 1 - decay swapped', 'warm-up ignored', 't - 1 in place of t', 'max in place of min',
                                  'shadow and param swapped'])
def test_gate_rejects_wrong_variants(name):
    s, w = R.planted(1028, seed=7)
    cases = [(0.999, 1), (0.999, 10), (0.999, 8000), (0.5, 1)]            # inside the warm-up: every variant differs from the kernel
    if name in ('decay and 1 - decay swapped', 'max in place of min', 'shadow and param swapped'):
        cases.append((0.999, 100000))                                      # ... and these three past the crossover as well
    for decay, step in cases:
        good, dg = R.model_f32(s, w, decay, step)
        assert R.passes(s, w, good, dg, decay, step)
        got, du = _variant(name, s, w, decay, step)
        assert not R.passes(s, w, got, du, decay, step), (name, decay, step)


def test_ema_abi_refuses_bad_arguments_before_any_launch():
    from gan_amd import _lib as L
    lib = L.load()
    P, Q = 1 << 22, 1 << 23                                  # (never dereferenced: every call here is refused on the host)
    call = lambda s=P, w=Q, n=64, d=0.999, step=None, used=None: lib.gan_ema_update(s, w, n, d, step, used, None)
    assert call(s=None) == L.E_ARG and call(w=None) == L.E_ARG
    for n in (0, 6, -4, -1):
        assert call(n=n) == L.E_ARG, n
    for off in (4, 8, 12, 1):
        assert call(s=P + off) == L.E_ARG and call(w=Q + off) == L.E_ARG, off
    for d in (-0.1, 1.0, 1.5, float('nan')):
        assert call(d=d) == L.E_ARG, d
    assert call(d=-0.1, step=P, used=Q) == L.E_ARG


def test_header_and_binding_name_gan_ema_update():
    from gan_amd import _lib as L
    hdr = open(os.path.join(ROOT, 'include', 'gan_amd.h')).read()
    m = re.search(r'int gan_ema_update\(([^)]*)\)', hdr)
    assert m, "include/gan_amd.h does not declare gan_ema_update"
    args = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
    assert [a.rsplit(' ', 1)[0].strip() for a in args] == ['float*', 'const float*', 'int64_t', 'float', 'const int32_t*', 'float*', 'gan_stream_t']
    res, argtypes = L.SYMBOLS['gan_ema_update']
    assert res is C.c_int and argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    assert hasattr(L.load(), 'gan_ema_update')
    assert 'gan_ema_update' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_both_clis_parse_the_ema_flags():
    from gan_amd import cycle_gan, pix2pix
    p = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']
    c = ['--input-images', 'x', '--target-images', 'y', '--output', 'o', '--train', '--epochs', '1']
    for mod, base in ((pix2pix, p), (cycle_gan, c)):
        o = mod.parse_opt(base)
        assert (o.ema_decay, o.ema_warmup, o.predict_weights) == (0.0, 'true', 'raw')
        o = mod.parse_opt(base + ['--ema-decay', '0.999', '--ema-warmup', 'false', '--predict-weights', 'ema'])
        assert (o.ema_decay, o.ema_warmup, o.predict_weights) == (0.999, 'false', 'ema')
        for bad in (['--ema-decay', '1.0'], ['--ema-decay', '-0.1'], ['--ema-warmup', 'yes'], ['--predict-weights', 'mean']):
            with pytest.raises(SystemExit):
                mod.parse_opt(base + bad)


class _Params:
    """What WeightAverage touches of a ParamSet, on the host."""

    def __init__(self, seed):
        self.entries = {'down0.kernel': (0, (4, 4, 1, 64)), 'down1.kernel': (1024, (4, 4, 2, 3)), 'down1.gamma': (1152, (3,))}
        self.total = 1216
        self.master = torch.from_numpy(np.random.default_rng(seed).standard_normal(self.total).astype(F32))
        self.step = torch.zeros(1, dtype=torch.int32)

    def prepare(self):
        pass


class _Model:
    def __init__(self, seed):
        from gan_amd.checkpoint import GEN_LAYERS
        self.layers, self.obj_name = GEN_LAYERS, 'generator'
        self.net = type('Net', (), {})()
        self.net.params = _Params(seed)

    def param_names(self):
        return list(self.net.params.entries)

    def state_dict(self):
        from gan_amd.checkpoint import tf_variable_key
        ps = self.net.params
        return {tf_variable_key('generator', self.layers, k).split('/', 1)[1]: ps.master[o:o + int(np.prod(sh))].view(sh).numpy().copy()
                for k, (o, sh) in ps.entries.items()}

    def load_state_dict(self, sd):
        from gan_amd.checkpoint import tf_variable_key
        ps = self.net.params
        for k, (o, sh) in ps.entries.items():
            key = tf_variable_key('generator', self.layers, k).split('/', 1)[1]
            if key in sd:
                ps.master[o:o + int(np.prod(sh))].copy_(torch.from_numpy(np.array(sd[key])).reshape(-1))


def test_checkpoint_stores_the_average_under_the_models_variable_names(tmp_path):
    from gan_amd import tfbundle as TB
    from gan_amd.checkpoint import Checkpoint
    from gan_amd.ema import WeightAverage
    m = _Model(1)
    e = WeightAverage(m, 0.99, True)
    assert torch.equal(e.shadow, m.net.params.master) and e.shadow.data_ptr() != m.net.params.master.data_ptr() and not e.loaded
    e.shadow.mul_(0.5)                                         # an average that differs from the weights
    prefix = str(tmp_path / 'ckpt-1')
    Checkpoint(generator=m, generator_ema=e).write(prefix)
    keys = set(TB.read_bundle(prefix)[0])
    V = '/.ATTRIBUTES/VARIABLE_VALUE'
    assert 'generator_ema/layer_with_weights-0/layer_with_weights-0/kernel' + V in keys
    assert 'generator_ema/layer_with_weights-1/layer_with_weights-1/gamma' + V in keys and 'generator_ema/decay' + V in keys
    assert sum(k.startswith('generator_ema/') for k in keys) == 4          # the three trainable variables and the decay
    # round trip into a fresh pair: the generator first, then its average
    m2 = _Model(2)
    e2 = WeightAverage(m2, 0.99, True)
    Checkpoint(generator=m2, generator_ema=e2).restore(prefix)
    assert e2.loaded and torch.equal(m2.net.params.master[:1024], m.net.params.master[:1024])
    for name, (o, sh) in m.net.params.entries.items():
        n = int(np.prod(sh))
        assert torch.equal(e2.shadow[o:o + n], e.shadow[o:o + n]), name
    # a checkpoint without averaged weights: the average starts over from the restored generator
    prefix2 = str(tmp_path / 'ckpt-2')
    Checkpoint(generator=m).write(prefix2)
    assert not any('_ema' in k for k in TB.read_bundle(prefix2)[0])
    m3 = _Model(3)
    e3 = WeightAverage(m3, 0.99, True)
    e3.loaded = True
    Checkpoint(generator=m3, generator_ema=e3).restore(prefix2)
    assert e3.loaded is False
    for name, (o, sh) in m.net.params.entries.items():
        n = int(np.prod(sh))
        assert torch.equal(e3.shadow[o:o + n], m.net.params.master[o:o + n]), name
    with pytest.raises(ValueError):
        WeightAverage(m, 1.0)


def test_averaged_exchanges_contents_in_place_and_restores_after_an_exception():
    from gan_amd.ema import WeightAverage
    m = _Model(4)
    ps = m.net.params
    e = WeightAverage(m, 0.9, False)
    e.shadow.add_(1.0)
    raw, avg, ptr = ps.master.clone(), e.shadow.clone(), ps.master.data_ptr()
    with e.averaged():
        assert torch.equal(ps.master, avg) and torch.equal(e.shadow, raw) and ps.master.data_ptr() == ptr
    assert torch.equal(ps.master, raw) and torch.equal(e.shadow, avg)
    with pytest.raises(RuntimeError, match='boom'):
        with e.averaged():
            raise RuntimeError('boom')
    assert torch.equal(ps.master, raw) and torch.equal(e.shadow, avg) and ps.master.data_ptr() == ptr
