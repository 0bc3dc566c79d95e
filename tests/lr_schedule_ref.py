"""Reference of the linear learning-rate decay (include/gan_amd.h, GanLrSchedule / gan_adam_begin_sched), written
from the formula and not from the kernel (helper of tests/test_cpu_lr_schedule.py and tests/test_gpu_lr_schedule.py; not a conftest).

Update index i = t - 1 (0-based) runs at lr * f(i):
    f(i) = 1                                                    i <  decay_start
         = (ef * (i - decay_start) + (decay_end - i)) / (decay_end - decay_start)      decay_start <= i < decay_end
         = ef                                                   i >= decay_end
The middle line is ef + (1 - ef) * (decay_end - i) / (decay_end - decay_start) over one denominator: with ef an fp32 value and the
indices below 2^31 its numerator is exact in np.longdouble (24 + 31 bits of a 64-bit significand on x86-64; where longdouble is the
53-bit double it carries one rounding of 2^-53, far below the gate), so f costs one rounding, the division.  lr_now = lr * f and
lr_t = lr * f * sqrt(1 - b2^t) / (1 - b1^t) continue in extended precision from the fp32 arguments - the construction of
elementwise_ref.lr_t_ref - and are rounded once to fp32.

Gate: one ulp of fp32 on both outputs, the gate gan_adam_begin is held to (tests/test_gpu_elementwise.py::test_adam_begin): the
kernel's double arithmetic is a few 2^-53 off the exact value, so its one rounding to fp32 lands on the reference or, where the exact
value sits within that distance of a rounding boundary, on its neighbour.  Where the reference is exactly 0 (end_factor 0 from
decay_end on) the output must be +0.0f, bit for bit."""
import math

import numpy as np

from tests import elementwise_ref as E

F32 = np.float32
LD = np.longdouble
GATE_ULPS = 1

CPU_SCHEDULES = ((0, 1), (1, 3), (1000, 2000), (99999, 100003))       # (decay_start, decay_end)
CPU_END_FACTORS = (0.0, 0.1, 1.0)
GPU_SCHEDULES = ((1, 3), (1000, 2000), (99999, 100003))
GPU_END_FACTORS = (0.0, 0.1)
RUN_SCHEDULE = (20, 40, 0.25)                                         # (decay_start, decay_end, end_factor): 64 launches on one counter
RUN_LAUNCHES = 64
STEP_SCHEDULE = (1, 3, 0.0)                                           # the captured steps: updates 0, 1 at lr, 2 at lr / 2, then 0
OFF_START = 1 << 30                                                   # a schedule that never starts: the constant rate


def factor_ref(end_factor, decay_start, decay_end, i):
    """f(i) in extended precision from the fp32-rounded end_factor."""
    ef = LD(F32(end_factor))
    if i < decay_start:
        return LD(1)
    if i >= decay_end:
        return ef
    return (ef * LD(i - decay_start) + LD(decay_end - i)) / LD(decay_end - decay_start)


def lr_now_ref(lr, end_factor, decay_start, decay_end, i):
    """(float)(lr * f(i)): the rate of update i."""
    return F32(LD(F32(lr)) * factor_ref(end_factor, decay_start, decay_end, i))


def lr_t_ref(lr, end_factor, decay_start, decay_end, b1, b2, t):
    """(float)(lr * f(t - 1) * sqrt(1 - b2^t) / (1 - b1^t)): elementwise_ref.lr_t_ref's expression with the factor in it."""
    lr_, b1_, b2_ = LD(F32(lr)), LD(F32(b1)), LD(F32(b2))
    f = factor_ref(end_factor, decay_start, decay_end, t - 1)
    return F32(lr_ * f * np.sqrt(LD(1) - b2_ ** LD(t)) / (LD(1) - b1_ ** LD(t)))


def model(lr, end_factor, decay_start, decay_end, b1, b2, t):
    """The kernel's arithmetic in numpy / Python doubles: double from the fp32 arguments, one rounding per output -> (lr_t, lr_now)."""
    lr, ef, b1, b2 = E.f32c(lr), E.f32c(end_factor), E.f32c(b1), E.f32c(b2)
    i = t - 1
    f = 1.0
    if i >= decay_end:
        f = ef
    elif i >= decay_start:
        f = ef + (1.0 - ef) * float(decay_end - i) / float(decay_end - decay_start)
    return F32(lr * f * math.sqrt(1.0 - math.pow(b2, t)) / (1.0 - math.pow(b1, t))), F32(lr * f)


def ulps(got, ref):
    """Distance of an output from its reference in ulps of fp32; a reference of exactly 0 demands +0.0f (else inf)."""
    got, ref = np.asarray(got, F32), np.asarray(ref, F32)
    if not np.isfinite(got):
        return math.inf
    if ref == 0:
        return 0 if int(got.view(np.uint32)) == 0 else math.inf
    if not got > 0:
        return math.inf
    return E.ulps_apart32(got, ref)


def boundary_indices(decay_start, decay_end, reach):
    """Every update index within `reach` of either boundary, plus 0 and decay_end + 5 (update indices start at 0)."""
    out = {0, decay_end + 5}
    for b in (decay_start, decay_end):
        out |= {b + k for k in range(-reach, reach + 1)}
    return sorted(i for i in out if i >= 0)


def check(lr, end_factor, decay_start, decay_end, b1, b2, t, lr_t, lr_now=None):
    """{item: ulps} of one launch's outputs against the reference."""
    res = {'lr_t': ulps(lr_t, lr_t_ref(lr, end_factor, decay_start, decay_end, b1, b2, t))}
    if lr_now is not None:
        res['lr_now'] = ulps(lr_now, lr_now_ref(lr, end_factor, decay_start, decay_end, t - 1))
    return res
