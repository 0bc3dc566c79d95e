"""The step cache of the two model front-ends (GAN._step_for, gan_amd/base_gan.py): building and capturing a step runs warm-up
passes of the whole step, and none of what they move may stay moved - the weights, Adam's moments and counters, BatchNorm's moving
statistics, the fp16 loss-scale state, the rate a scheduled update reports and the dropout draw counters.  fp16, so that the
loss-scale state exists, and a learning-rate schedule, so that lr_now does; no step is replayed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 2e-4


def _model(name, tmp):
    from gan_amd import cycle_gan, pix2pix
    common = ['--output', str(tmp), '--train', '--epochs', '1', '--img-size', '256', '--channels', '1', '--dtype', 'f16',
              '--lr-decay-epochs', '1']
    if name == 'pix2pix':
        return pix2pix.Pix2Pix(vars(pix2pix.parse_opt(['--data', str(tmp)] + common)))
    return cycle_gan.CycleGAN(vars(cycle_gan.parse_opt(['--input-images', str(tmp), '--target-images', str(tmp)] + common)))


def _param_sets(m, name):
    models = ((m.generator, m.discriminator) if name == 'pix2pix'
              else (m.generator_g, m.generator_f, m.discriminator_x, m.discriminator_y))
    return [mod.net.params for mod in models]


def _mask_draws(st):
    return [c.mask_draws for c in vars(st).values() if isinstance(getattr(c, 'mask_draws', None), torch.Tensor)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("name", ['pix2pix', 'cyclegan'])
def test_a_capture_leaves_no_trace(name, tmp_path):
    from gan_amd.runner import lr_schedule_for
    m = _model(name, tmp_path)
    m.lr_schedule = lr_schedule_for(m.config, 4)
    assert m.lr_schedule is not None and m.ctx.ls is not None
    sets = _param_sets(m, name)
    assert len(sets) == (2 if name == 'pix2pix' else 4)
    if name == 'pix2pix':
        assert all(ps.state for ps in sets)                   # BatchNorm's moving statistics: a warm-up pass moves them
    before = [dict(master=ps.master.clone(), m=ps.m.clone(), v=ps.v.clone(), step=ps.step.clone(),
                   **{'state ' + k: t.clone() for k, t in ps.state.items()}) for ps in sets]
    ls0 = m.ctx.ls.clone()
    torch.cuda.synchronize()

    def untouched(after):
        torch.cuda.synchronize()
        assert _same(m.ctx.ls, ls0), (after, m.ctx.ls.tolist(), ls0.tolist())
        for i, (ps, want) in enumerate(zip(sets, before)):
            for k, t in want.items():
                got = ps.state[k[6:]] if k.startswith('state ') else getattr(ps, k)
                assert _same(got, t), (after, i, k)
            # created with the base rate by the first training step: no update has run, so that is what it still reports
            assert ps.lr_now is not None and ps.lr_now.tolist() == [float(np.float32(LR))], (after, i, ps.lr_now.tolist())

    steps = []
    for batch, training in ((1, True), (2, True), (1, False)):
        st, replay = m._step_for(batch, training)
        assert callable(replay) and m._steps[(batch, training)] == (st, replay) and m._step_for(batch, training)[0] is st
        steps.append(st)
        untouched((batch, training))
        for s in steps:                                       # the counters start at zero: not one draw is left on any step so far
            draws = _mask_draws(s)
            assert draws, "no dropout draw counter found on the step"
            for d in draws:
                assert d.dtype == torch.int32 and not d.any().item(), ((batch, training), d.tolist())
    assert len({id(s) for s in steps}) == 3 and len(m._steps) == 3
    for st in steps:
        assert len(st.nets()) == len(sets) and all(net.params is ps for net, ps in zip(st.nets(), sets))
    assert steps[0].ema == () and steps[1].ema == () and steps[2].ema == ()      # no --ema-decay: nothing to move
    assert steps[0].lr_schedule == m.lr_schedule and steps[1].lr_schedule == m.lr_schedule and steps[2].lr_schedule is None
    assert all(s.sync is None for s in steps)
