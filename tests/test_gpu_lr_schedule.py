"""The learning-rate schedule on the GPU: gan_adam_begin_sched per launch against the extended-precision
reference and the one-ulp gate of tests/lr_schedule_ref.py (proven on the CPU by tests/test_cpu_lr_schedule.py), its bit equality with
gan_adam_begin where the factor is 1, a counter walked across a whole schedule, captured Pix2Pix and CycleGAN steps whose rate the
device takes to zero under graph replay (one GPU, and the data-parallel schedules behind a stub exchange), a schedule that never
starts against no schedule, and one command-line run per model."""
import ctypes as C
import gc
import json
import os
import types

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from tests import elementwise_ref as E
from tests import launch_audit as A
from tests import lr_schedule_ref as R
from tests.test_gpu_elementwise import Guarded, scale_state, sync
from tests.test_gpu_step import _FakeSync

pytestmark = pytest.mark.gpu

F32 = np.float32
LR, B1, B2 = E.LR, E.BETA1, E.BETA2
WORST = {}


@pytest.fixture(scope="module")
def dev(request):
    request.addfinalizer(lambda: print('\n' + E.table(WORST, 'learning-rate schedule (ulps of fp32, gate 1)')))
    d = torch.device('cuda:0')
    return types.SimpleNamespace(lib=L.load(), device=d, stream=lambda: torch.cuda.current_stream(d).cuda_stream)


def gate(name, item, value):
    E.note(WORST, name, item, value)
    assert value <= R.GATE_ULPS, (name, item, value)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- the kernel, per launch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ef", R.GPU_END_FACTORS)
@pytest.mark.parametrize("sched", R.GPU_SCHEDULES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_adam_begin_sched(dev, sched, ef):
    """Counters at, one before and one after both boundaries, 0 and decay_end + 5, without a scale state, with one and with its flag
    raised, lr_now given and NULL: step + 1, lr_t and lr_now within the gate (exactly +0 where the reference is 0), the guards and the
    scale state intact; a skipped step keeps all three words."""
    d0, d1 = sched
    desc = L.GanLrSchedule(LR, ef, d0, d1)
    starts = R.boundary_indices(d0, d1, 1)
    assert {0, d0 - 1, d0, d0 + 1, d1 - 1, d1, d1 + 1, d1 + 5} == set(starts)
    for step0 in starts:
        for ls in (None, E.LS_ON, E.LS_SKIP):
            for with_now in (True, False):
                st = scale_state(dev, ls)
                step = Guarded(dev.device, 1, torch.int32, data=torch.tensor([step0], dtype=torch.int32), fill=-1)
                lr_t = Guarded(dev.device, 1, data=torch.tensor([0.125]))
                lr_now = Guarded(dev.device, 1, data=torch.tensor([0.375]))
                rc = dev.lib.gan_adam_begin_sched(step.ptr, lr_t.ptr, lr_now.ptr if with_now else None, C.byref(desc), B1, B2,
                                                  st.ptr if st else None, dev.stream())
                assert rc == 0
                sync()
                if ls is E.LS_SKIP:
                    assert step.untouched() and lr_t.untouched() and lr_now.untouched()
                else:
                    assert int(step.host()[0]) == step0 + 1
                    got_t = lr_t.host().numpy()[0]
                    got_now = lr_now.host().numpy()[0] if with_now else None
                    for k, v in R.check(LR, ef, d0, d1, B1, B2, step0 + 1, got_t, got_now).items():
                        gate('gan_adam_begin_sched', f'{k} {d0}-{d1} ef={ef:g}', v)
                    if ef == 0.0 and step0 >= d1:
                        assert got_t.view(np.uint32) == 0 and (got_now is None or got_now.view(np.uint32) == 0)
                    step.changed(), lr_t.changed()                  # (assert the guards)
                    assert lr_now.changed().all() if with_now else lr_now.untouched()
                assert st is None or st.untouched()


@pytest.mark.parametrize("step0", E.ADAM_BEGIN_STEPS)
def test_a_schedule_that_never_starts_writes_the_bits_of_adam_begin(dev, step0):
    desc = L.GanLrSchedule(LR, 0.0, R.OFF_START, R.OFF_START + 1)
    out = []
    for sched in (False, True):
        step = Guarded(dev.device, 1, torch.int32, data=torch.tensor([step0], dtype=torch.int32), fill=-1)
        lr_t = Guarded(dev.device, 1, data=torch.tensor([0.125]))
        lr_now = Guarded(dev.device, 1, data=torch.tensor([0.375]))
        if sched:
            assert dev.lib.gan_adam_begin_sched(step.ptr, lr_t.ptr, lr_now.ptr, C.byref(desc), B1, B2, None, dev.stream()) == 0
        else:
            assert dev.lib.gan_adam_begin(step.ptr, lr_t.ptr, LR, B1, B2, None, dev.stream()) == 0
        sync()
        assert int(step.host()[0]) == step0 + 1
        step.changed(), lr_t.changed(), lr_now.changed()
        out.append((lr_t.host().numpy()[0], lr_now.host().numpy()[0]))
    assert out[0][0].view(np.uint32) == out[1][0].view(np.uint32), (step0, out)
    assert out[1][1].view(np.uint32) == F32(LR).view(np.uint32) and out[0][1].view(np.uint32) == F32(0.375).view(np.uint32)


def test_launch_log_names_the_kernel(dev):
    """The diagnostic launch log (tools/class_profile.py joins it with the op labels) records the launch under its own symbol."""
    desc = L.GanLrSchedule(LR, 0.0, 1, 3)
    step = Guarded(dev.device, 1, torch.int32, data=torch.tensor([0], dtype=torch.int32), fill=-1)
    lr_t = Guarded(dev.device, 1, data=torch.tensor([0.125]))
    old = L.set_option('diag.launch_log', 1)
    try:
        n0 = len(L.launch_log())
        assert dev.lib.gan_adam_begin_sched(step.ptr, lr_t.ptr, None, C.byref(desc), B1, B2, None, dev.stream()) == 0
        assert dev.lib.gan_adam_begin(step.ptr, lr_t.ptr, LR, B1, B2, None, dev.stream()) == 0
        log = L.launch_log()[n0:]
    finally:
        L.set_option('diag.launch_log', old)
    sync()
    assert len(log) == 2 and 'adam_begin_sched_kernel' in log[0] and 'adam_begin_kernel' in log[1] and 'sched' not in log[1], log
    assert int(step.host()[0]) == 2


def test_one_counter_walks_the_whole_schedule(dev):
    d0, d1, ef = R.RUN_SCHEDULE
    desc = L.GanLrSchedule(LR, ef, d0, d1)
    step = Guarded(dev.device, 1, torch.int32, data=torch.tensor([0], dtype=torch.int32), fill=-1)
    lr_t = Guarded(dev.device, 1, data=torch.tensor([0.125]))
    lr_now = Guarded(dev.device, 1, data=torch.tensor([0.375]))
    rates = []
    for k in range(1, R.RUN_LAUNCHES + 1):              # launch k runs update k - 1
        assert dev.lib.gan_adam_begin_sched(step.ptr, lr_t.ptr, lr_now.ptr, C.byref(desc), B1, B2, None, dev.stream()) == 0
        sync()
        assert int(step.host()[0]) == k
        rates.append(lr_now.host().numpy()[0])
        for item, v in R.check(LR, ef, d0, d1, B1, B2, k, lr_t.host().numpy()[0], rates[-1]).items():
            gate('gan_adam_begin_sched', f'{item} walk {d0}-{d1} ef={ef:g}', v)
    step.changed(), lr_t.changed(), lr_now.changed()
    assert int(step.host()[0]) == R.RUN_LAUNCHES == 64
    assert all(a >= b for a, b in zip(rates, rates[1:]))
    floor = F32(float(F32(LR)) * 0.25)
    assert all(r.view(np.uint32) == F32(LR).view(np.uint32) for r in rates[:d0 + 1])            # updates 0 .. 20
    assert all(r.view(np.uint32) == floor.view(np.uint32) for r in rates[d1:])                  # updates 40 .. 63
    assert rates[d0 + 1] < rates[d0] and rates[d1 - 1] > rates[d1]


# ---- captured steps ---------------------------------------------------------------------------------------------------------------------
def _inputs(ctx, seed):
    from oracle import gan_oracle as O
    inp, tar = O.synthetic_pair(1, 256, 1, seed=seed)
    return torch.from_numpy(inp).to(ctx.device), torch.from_numpy(tar).to(ctx.device)


def _start_over(st, w0):
    """Weights back to those before capture()'s warm-up steps, Adam state and the step counters to zero."""
    for net, w in zip(st.nets(), w0):
        P = net.params
        P.master.copy_(w)
        P.m.zero_(); P.v.zero_(); P.step.zero_()
        P.prepare()
    torch.cuda.synchronize()


def _replay_to_zero(st, replay, w0, x, y, tags):
    """Five replays of a step captured with R.STEP_SCHEDULE on fixed inputs: after each, every network's counter, lr_t and lr_now
    against the reference of that update; weights bit-equal from the third replay on; the step itself goes on (Adam moments move)."""
    d0, d1, ef = R.STEP_SCHEDULE
    _start_over(st, w0)
    snaps = []
    for k in range(1, 6):
        losses = replay(x, y).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(losses).all()
        for tag, net in zip(tags, st.nets()):
            P = net.params
            assert int(P.step.item()) == k, (tag, k)
            for item, v in R.check(LR, ef, d0, d1, B1, B2, k, P.lr_t.cpu().numpy()[0], P.lr_now.cpu().numpy()[0]).items():
                gate('captured step', f'{tag} {item}', v)
        gate('captured step', 'current_lr()', R.ulps(F32(st.current_lr()), R.lr_now_ref(LR, ef, d0, d1, k - 1)))
        snaps.append([(net.params.master.clone(), net.params.m.clone()) for net in st.nets()])
    assert st.current_lr() == 0.0
    for i, tag in enumerate(tags):
        assert not _same_bits(snaps[0][i][0], w0[i]) and not _same_bits(snaps[2][i][0], snaps[1][i][0]), tag     # rates lr and lr / 2 move it
        assert _same_bits(snaps[3][i][0], snaps[2][i][0]) and _same_bits(snaps[4][i][0], snaps[2][i][0]), tag  # rate 0: not one bit
    assert any(not _same_bits(snaps[4][i][1], snaps[2][i][1]) for i in range(len(tags)))                       # the step still ran


@pytest.mark.parametrize("dtype, mode", [('bf16', 'graph'), ('f32', 'graph'), ('f32', 'bucketed'), ('f32', 'phased')])
def test_captured_pix2pix_step_decays_to_zero_under_replay(dtype, mode):
    """mode 'graph': the one-GPU step (bf16: the wgrad launches carry Adam, gan_adam_prepare_multi and gan_adam_tf do the rest; f32:
    gan_adam_prepare_multi + gan_adam_tf alone).  'bucketed' / 'phased': the data-parallel schedules, forced on one GPU by
    test_gpu_step.py's world-2 stub exchange - their Adam graphs go through ParamSet.adam / adam_begin_ops / adam_segment_ops."""
    from gan_amd.nets import Ctx, LrSchedule
    from gan_amd.steps import Pix2PixStep
    d0, d1, ef = R.STEP_SCHEDULE
    ctx = Ctx('cuda:0', dtype)
    st = Pix2PixStep(ctx, 1, 256, 1, lam=100.0, lr=LR, beta_1=B1, beta_2=B2, seed=123, lr_schedule=LrSchedule(LR, ef, d0, d1))
    assert all(n.params.lr_schedule == LrSchedule(LR, ef, d0, d1) for n in st.nets())
    if mode != 'graph':
        st.sync = _FakeSync()
        st.ddp_buckets = mode == 'bucketed'
    w0 = [n.params.master.clone() for n in st.nets()]
    replay = st.capture(training=True)
    assert hasattr(st, 'buckets') == (mode == 'bucketed')
    _replay_to_zero(st, replay, w0, *_inputs(ctx, 123), tags=('G', 'D'))


def test_captured_cyclegan_step_decays_to_zero_under_replay():
    from gan_amd.nets import Ctx, LrSchedule
    from gan_amd.steps import CycleGANStep
    d0, d1, ef = R.STEP_SCHEDULE
    ctx = Ctx('cuda:0', 'bf16')
    st = CycleGANStep(ctx, 1, 256, 1, lam=10.0, lr=LR, beta_1=B1, beta_2=B2, seed=7, lr_schedule=LrSchedule(LR, ef, d0, d1))
    assert len(st.nets()) == 4 and all(n.params.lr_schedule is not None for n in st.nets())
    w0 = [n.params.master.clone() for n in st.nets()]
    replay = st.capture(training=True)
    _replay_to_zero(st, replay, w0, *_inputs(ctx, 9), tags=('Gg', 'Gf', 'Dx', 'Dy'))


def _recorded_pix2pix(monkeypatch, lr_schedule):
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    gc.collect()
    torch.cuda.synchronize()
    rec = A.Recorder(monkeypatch)
    rec.hook_capture(monkeypatch)
    ctx = Ctx('cuda:0', 'bf16')
    st = Pix2PixStep(ctx, 1, 256, 1, lam=100.0, lr=LR, beta_1=B1, beta_2=B2, seed=123, lr_schedule=lr_schedule)
    w0 = [n.params.master.clone() for n in st.nets()]
    replay = st.capture(training=True)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return ctx, st, replay, w0, [c.name for c in rec.calls]


def test_off_means_off(monkeypatch):
    """A schedule that never starts and no schedule: the same weights, Adam moments and loss vectors after each of 3 replays, bit for
    bit; the recorded launch lists differ in the two begin launches alone, exchanged in place."""
    from gan_amd.nets import LrSchedule
    off = _recorded_pix2pix(monkeypatch, None)
    on = _recorded_pix2pix(monkeypatch, LrSchedule(LR, 0.0, R.OFF_START, R.OFF_START + 1))
    assert off[1].lr_schedule is None and all(n.params.lr_schedule is None and n.params.lr_now is None for n in off[1].nets())
    assert off[4].count('gan_adam_begin') == 2 and 'gan_adam_begin_sched' not in off[4]
    assert on[4].count('gan_adam_begin_sched') == 2 and 'gan_adam_begin' not in on[4]
    assert [n.replace('gan_adam_begin_sched', 'gan_adam_begin') for n in on[4]] == off[4]
    assert off[1].current_lr() == LR
    for a, b in zip(off[3], on[3]):
        assert _same_bits(a, b)
    x, y = _inputs(off[0], 123)
    for _, st, _, w0, _ in (off, on):
        _start_over(st, w0)
    for k in range(3):
        la = off[2](x, y).clone()
        lb = on[2](x, y).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(la).all() and _same_bits(la, lb), (k, la, lb)
        for na, nb in zip(off[1].nets(), on[1].nets()):
            for which in ('master', 'm', 'v', 'lr_t', 'step'):
                assert _same_bits(getattr(na.params, which), getattr(nb.params, which)), (k, which)
    assert on[1].current_lr() == float(F32(LR))


# ---- command lines ------------------------------------------------------------------------------------------------------------------------
def _strict(p):
    return json.loads(open(p).read(), parse_constant=lambda s: pytest.fail(f"not strict JSON: {s} in {p}"))


def _logs(out):
    return os.path.join(out, sorted(os.listdir(out))[0], 'logs')


def _write_images(folder, n, width, seed):
    from PIL import Image
    os.makedirs(folder)
    rng = np.random.default_rng(seed)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (64, width), dtype=np.uint8), 'L').save(os.path.join(folder, f"p{i}.png"))


def test_pix2pix_cli_logs_the_rate_of_every_epoch(tmp_path, capsys):
    from gan_amd import data as D
    from gan_amd import pix2pix
    data = str(tmp_path / 'data')
    _write_images(data, 6, 128, 3)
    base = ['--data', data, '--train', '--epochs', '3', '--batch-size', '1', '--test-img', '1', '--logging', 'false']
    out = str(tmp_path / 'out')
    pix2pix.main(pix2pix.parse_opt(base + ['--output', out, '--lr-decay-epochs', '2']))
    assert 'learning rate: ' in capsys.readouterr().out
    cfg = _strict(os.path.join(_logs(out), 'config.json'))
    assert cfg['lr_decay_epochs'] == 2 and cfg['lr_end_factor'] == 0.0 and cfg['learning_rate'] == LR
    spe = len(D.pix2pix_split(sorted(os.listdir(data)), cfg['seed'], 1, cfg['validation_size'])[0])          # batch size 1
    assert spe == 4
    rates = _strict(os.path.join(_logs(out), 'learning_rate.json'))
    assert len(rates) == 3
    for epoch, got in enumerate(rates, 1):
        ref = R.lr_now_ref(LR, 0.0, spe, 3 * spe, epoch * spe - 1)
        print(f"epoch {epoch}: logged {got!r}, reference {float(ref)!r}")
        assert float(F32(got)) == got and R.ulps(F32(got), ref) <= R.GATE_ULPS, (epoch, got, float(ref))
    assert rates[0] == float(F32(LR)) and rates[0] > rates[1] > rates[2] > 0.0
    plain = str(tmp_path / 'plain')
    pix2pix.main(pix2pix.parse_opt(base + ['--output', plain]))
    assert 'learning rate: ' not in capsys.readouterr().out
    assert not os.path.exists(os.path.join(_logs(plain), 'learning_rate.json'))
    cfg = _strict(os.path.join(_logs(plain), 'config.json'))
    assert cfg['lr_decay_epochs'] == 0 and cfg['lr_end_factor'] == 0.0


def test_cyclegan_cli_logs_the_rate_of_generator_g(tmp_path):
    from gan_amd import cycle_gan
    dx, dy, out = str(tmp_path / 'X'), str(tmp_path / 'Y'), str(tmp_path / 'out')
    _write_images(dx, 5, 64, 4)
    _write_images(dy, 4, 64, 5)
    cycle_gan.main(cycle_gan.parse_opt(['--input-images', dx, '--target-images', dy, '--output', out, '--train', '--epochs', '2',
                                        '--test-img', '1', '--validation-size', '0.25', '--logging', 'false', '--lr-decay-epochs', '1',
                                        '--lr-end-factor', '0.5']))
    cfg = _strict(os.path.join(_logs(out), 'config.json'))
    assert cfg['lr_decay_epochs'] == 1 and cfg['lr_end_factor'] == 0.5
    spe = 3                                   # X: 5 - 1 test - 1 validation = 3 training images, Y: 4 - 1 = 3; batch size 1
    rates = _strict(os.path.join(_logs(out), 'learning_rate.json'))
    assert len(rates) == 2
    for epoch, got in enumerate(rates, 1):
        assert R.ulps(F32(got), R.lr_now_ref(LR, 0.5, spe, 2 * spe, epoch * spe - 1)) <= R.GATE_ULPS, (epoch, got)
    assert rates[0] == float(F32(LR)) > rates[1] > 0.5 * LR
