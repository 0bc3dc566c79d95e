"""CPU side of the learning-rate schedule: the numpy model of gan_adam_begin_sched's arithmetic and the host
restatement LrSchedule.factor against the extended-precision reference of tests/lr_schedule_ref.py, the declarations, every argument
refusal through the loaded library (they come before any launch: no GPU), and the command-line surface of both drivers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from gan_amd import _lib as L
from tests import elementwise_ref as E
from tests import lr_schedule_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _cases():
    return [(d0, d1, ef, i) for d0, d1 in R.CPU_SCHEDULES for ef in R.CPU_END_FACTORS for i in R.boundary_indices(d0, d1, 2)]


def test_sweep_reaches_every_branch_on_both_sides_of_both_boundaries():
    for d0, d1 in R.CPU_SCHEDULES:
        idx = R.boundary_indices(d0, d1, 2)
        assert {0, d0, d0 + 1, d0 + 2, d1 - 1, d1, d1 + 1, d1 + 2, d1 + 5} <= set(idx) and min(idx) == 0
        assert {d0 - 2, d0 - 1} & set(idx) == {i for i in (d0 - 2, d0 - 1) if i >= 0}         # update indices start at 0
    assert len(_cases()) == sum(3 * len(R.boundary_indices(d0, d1, 2)) for d0, d1 in R.CPU_SCHEDULES)


def test_model_of_the_kernel_is_within_one_ulp_of_the_reference():
    worst = {'lr_t': 0, 'lr_now': 0}
    for d0, d1, ef, i in _cases():
        t = i + 1
        lr_t, lr_now = R.model(E.LR, ef, d0, d1, E.BETA1, E.BETA2, t)
        for k, v in R.check(E.LR, ef, d0, d1, E.BETA1, E.BETA2, t, lr_t, lr_now).items():
            worst[k] = max(worst[k], v)
            assert v <= R.GATE_ULPS, (k, d0, d1, ef, i, v)
        if ef == 0.0 and i >= d1:               # the floor of a decay to zero: +0.0f exactly, both outputs
            assert lr_t.view(np.uint32) == 0 and lr_now.view(np.uint32) == 0
        if i < d0 or ef == 1.0:                 # f = 1: the bits of the constant-rate kernel's model
            assert lr_t.view(np.uint32) == E.lr_t_model(E.LR, E.BETA1, E.BETA2, t).view(np.uint32)
            assert lr_now.view(np.uint32) == F32(E.LR).view(np.uint32)
    print(f"model against reference, worst ulps of fp32: {worst}")


def test_reference_has_the_shape_the_schedule_promises():
    for d0, d1 in R.CPU_SCHEDULES:
        for ef in R.CPU_END_FACTORS:
            f = lambda i: R.factor_ref(ef, d0, d1, i)
            assert f(d0) == 1 and f(max(d0 - 1, 0)) == 1 and f(d1) == R.LD(F32(ef)) and f(d1 + 5) == R.LD(F32(ef))
            if ef < 1.0:
                assert f(d1 - 1) > f(d1)        # the last decayed update is still above the floor
            assert R.lr_t_ref(E.LR, ef, d0, d1, E.BETA1, E.BETA2, d0 + 1) == E.lr_t_ref(E.LR, E.BETA1, E.BETA2, d0 + 1)
    # the reference can tell a wrong schedule: one update early, one late, and a jump to the floor at decay_start
    d0, d1, ef = 1000, 2000, 0.1
    i = 1500
    right = R.lr_now_ref(E.LR, ef, d0, d1, i)
    for wrong in (R.lr_now_ref(E.LR, ef, d0, d1, i + 1), R.lr_now_ref(E.LR, ef, d0, d1, i - 1), F32(E.LR * ef)):
        assert R.ulps(wrong, right) > R.GATE_ULPS
    assert R.ulps(F32(-0.0), F32(0.0)) == math.inf and R.ulps(F32(0.0), F32(0.0)) == 0 and R.ulps(F32(1e-45), F32(0.0)) == math.inf


def test_host_restatement_agrees_with_the_reference():
    from gan_amd.nets import LrSchedule
    for d0, d1 in R.CPU_SCHEDULES:
        for ef in R.CPU_END_FACTORS:
            s = LrSchedule(E.LR, ef, d0, d1).validate()
            idx = list(range(0, d1 + 8)) if d1 <= 4096 else R.boundary_indices(d0, d1, 2)
            vals = [s.factor(i) for i in idx]
            for i, v in zip(idx, vals):
                ref = R.factor_ref(ef, d0, d1, i)
                assert abs(R.LD(v) - ref) <= 4 * 2.0 ** -53, (d0, d1, ef, i, v, ref)
                assert R.ulps(F32(s.lr_at(i)), R.lr_now_ref(E.LR, ef, d0, d1, i)) <= R.GATE_ULPS
            assert all(a >= b for a, b in zip(vals, vals[1:])), (d0, d1, ef)          # non-increasing
            assert s.factor(d0) == 1.0 and s.factor(d1) == float(F32(ef))
    d = LrSchedule(2e-4, 0.1, 42, 70).desc()
    assert (d.struct_size, d.decay_start, d.decay_end) == (C.sizeof(L.GanLrSchedule), 42, 70)
    assert F32(d.lr) == F32(2e-4) and F32(d.end_factor) == F32(0.1)
    for bad in ((0.0, 0, 1, 2), (-1e-4, 0, 1, 2), (math.nan, 0, 1, 2), (math.inf, 0, 1, 2), (1e39, 0, 1, 2), (2e-4, -0.1, 1, 2),
                (2e-4, 1.5, 1, 2), (2e-4, math.nan, 1, 2), (2e-4, 0, -1, 2), (2e-4, 0, 2, 2), (2e-4, 0, 3, 2), (2e-4, 0, 1, 1 << 31),
                (2e-4, 0, 1.5, 2)):
        with pytest.raises(ValueError):
            LrSchedule(*bad).validate()


def test_header_declares_and_the_binding_lists_the_entry_point_and_its_struct():
    hdr = open(os.path.join(ROOT, 'include', 'gan_amd.h')).read()
    assert re.search(r'\bint gan_adam_begin_sched\(int32_t\* step, float\* lr_t, float\* lr_now, const GanLrSchedule\* s,', hdr)
    assert re.search(r'typedef struct GanLrSchedule \{.*?\} GanLrSchedule;', hdr, flags=re.S)
    res, args = L.SYMBOLS['gan_adam_begin_sched']
    assert res is C.c_int and len(args) == 8 and args[3] == C.POINTER(L.GanLrSchedule) and args[4:6] == [C.c_float, C.c_float]
    assert [f for f, _ in L.GanLrSchedule._fields_] == ['struct_size', 'lr', 'end_factor', 'decay_start', 'decay_end']
    assert C.sizeof(L.GanLrSchedule) == 20 and L.GanLrSchedule(2e-4, 0.0, 1, 3).struct_size == 20
    assert hasattr(L.load(), 'gan_adam_begin_sched')
    # the constant-rate entry point keeps its signature
    assert L.SYMBOLS['gan_adam_begin'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p])


def test_every_bad_argument_is_refused_before_any_launch():
    """No device memory is behind these pointers and no GPU need be present: GAN_E_ARG comes back before anything is enqueued."""
    lib = L.load()
    P = 4096                                     # a non-NULL address that is never dereferenced
    ok = lambda: L.GanLrSchedule(2e-4, 0.1, 10, 20)

    def call(step=P, lr_t=P, lr_now=P, s='ok', **fields):
        d = ok()
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.gan_adam_begin_sched(step, lr_t, lr_now, None if s is None else C.byref(d), 0.5, 0.999, None, None)

    assert call(step=None) == L.E_ARG
    assert call(lr_t=None) == L.E_ARG
    assert call(s=None) == L.E_ARG
    for size in (0, C.sizeof(L.GanLrSchedule) - 4, C.sizeof(L.GanLrSchedule) + 4):
        assert call(struct_size=size) == L.E_ARG
    for lr in (math.nan, math.inf, -math.inf, 0.0, -0.0, -2e-4):
        assert call(lr=lr) == L.E_ARG, lr
    for ef in (-0.1, -1e-30, 1.0000001, 2.0, math.nan, math.inf, -math.inf):
        assert call(end_factor=ef) == L.E_ARG, ef
    assert call(decay_start=-1) == L.E_ARG
    assert call(decay_start=-2 ** 31, decay_end=-5) == L.E_ARG
    assert call(decay_end=10) == L.E_ARG         # == decay_start
    assert call(decay_end=9) == L.E_ARG
    assert call(decay_start=0, decay_end=0) == L.E_ARG
    assert call(lr_now=None, lr=math.nan) == L.E_ARG            # (a NULL lr_now is allowed: the other checks still come first)


# ---- command lines -------------------------------------------------------------------------------------------------------------------
def _parsers():
    from gan_amd import cycle_gan, pix2pix
    return ((pix2pix.parse_opt, ['--data', 'd', '--output', 'o']),
            (cycle_gan.parse_opt, ['--input-images', 'x', '--target-images', 'y', '--output', 'o']))


def test_cli_defaults_build_no_schedule():
    from gan_amd.runner import lr_schedule_for
    for parse, base in _parsers():
        o = parse(base + ['--train', '--epochs', '10'])
        assert (o.lr_decay_epochs, o.lr_end_factor) == (0, 0.0) and isinstance(o.lr_decay_epochs, int)
        assert lr_schedule_for(vars(o), 7) is None
        p = parse(base + ['--predict', '--weights', 'w'])
        assert (p.lr_decay_epochs, p.lr_end_factor) == (0, 0.0) and lr_schedule_for(vars(p), 7) is None
    assert lr_schedule_for({'learning_rate': 2e-4}, 7) is None         # a config from before the flags


def test_cli_places_the_decay_over_the_last_epochs():
    from gan_amd.nets import LrSchedule
    from gan_amd.runner import lr_schedule_for
    for parse, base in _parsers():
        o = parse(base + ['--train', '--epochs', '10', '--lr-decay-epochs', '4'])
        s = lr_schedule_for(vars(o), 7)
        assert isinstance(s, LrSchedule) and (s.decay_start, s.decay_end, s.end_factor, s.lr) == (42, 70, 0.0, 2e-4)
        o = parse(base + ['--train', '--epochs', '10', '--lr-decay-epochs', '10', '--lr-end-factor', '0.1', '--learning-rate', '1e-4'])
        s = lr_schedule_for(vars(o), 3)
        assert (s.decay_start, s.decay_end, s.end_factor, s.lr) == (0, 30, 0.1, 1e-4)
        o = parse(base + ['--train', '--epochs', '2', '--lr-end-factor', '0.5'])           # a floor without a decay: constant rate
        assert lr_schedule_for(vars(o), 3) is None
        with pytest.raises(ValueError):
            lr_schedule_for(vars(parse(base + ['--train', '--epochs', '10', '--lr-decay-epochs', '4'])), 0)


@pytest.mark.parametrize("extra, message", [
    (['--train', '--epochs', '5', '--lr-decay-epochs', '-1'], '--lr-decay-epochs -1 is negative'),
    (['--train', '--epochs', '5', '--lr-decay-epochs', '6'], '--lr-decay-epochs 6 is more than --epochs 5'),
    (['--train', '--epochs', '5', '--lr-decay-epochs', '2', '--lr-end-factor', '-0.1'], '--lr-end-factor -0.1 is outside [0, 1]'),
    (['--train', '--epochs', '5', '--lr-decay-epochs', '2', '--lr-end-factor', '1.5'], '--lr-end-factor 1.5 is outside [0, 1]'),
    (['--train', '--epochs', '5', '--lr-end-factor', 'nan'], '--lr-end-factor nan is outside [0, 1]'),
    (['--predict', '--weights', 'w', '--lr-decay-epochs', '2'], '--lr-decay-epochs: the learning-rate schedule belongs to --train'),
    (['--predict', '--weights', 'w', '--lr-decay-epochs', '0'], '--lr-decay-epochs: the learning-rate schedule belongs to --train'),
    (['--predict', '--weights', 'w', '--lr-end-factor', '0.5'], '--lr-end-factor: the learning-rate schedule belongs to --train'),
])
def test_cli_refusals(extra, message, capsys):
    for parse, base in _parsers():
        with pytest.raises(SystemExit):
            parse(base + extra)
        assert message in capsys.readouterr().err
