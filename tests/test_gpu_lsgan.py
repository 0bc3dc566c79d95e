"""The least-squares GAN loss on the GPU: both entry points per element against the fp64 references and
gates of tests/lsgan_ref.py (proven on the CPU by tests/test_cpu_lsgan.py), one training step per model with gan_loss='lsgan'
against an fp64 autograd reference under the gates of tests/test_gpu_step.py, the recorded launch lists, the bucketed and phased
data-parallel schedules behind a stub exchange, and one command-line run per model."""
import json
import os

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from tests import elementwise_ref as E
from tests import launch_audit as A
from tests import lsgan_ref as R
from tests.test_gpu_elementwise import Guarded, View, _int_view, scale_state, sync
from tests.test_gpu_step import _FakeSync, check_grads

pytestmark = pytest.mark.gpu

F32 = np.float32
WORST = {}


@pytest.fixture(scope="module", params=['f32', 'bf16', 'f16'])
def ctx(request):
    from gan_amd.nets import Ctx
    request.addfinalizer(lambda: print('\n' + E.table(WORST.get(request.param, {}), 'least-squares loss ' + request.param)))
    return Ctx('cuda:0', request.param)


def gate(c, name, item, value):
    E.note(WORST.setdefault(c.dtype, {}), name, item, value)
    print(f"    [{c.dtype}] {name} {item}: {value:.3f}")
    assert value <= 1.0, (name, item, value)


# ---- the two entry points, per element -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", R.LSQ_COUNTS)
def test_lsq_logits(ctx, count):
    """gan_lsq_logits: gradient per element (pitch 8, the seven pad elements per pixel untouched) and loss scalar against their gates;
    dx null; loss_accumulate from a non-zero loss_out (exactly the fp32 sum); with a scale state the gradient is scaled and the loss
    is not; a raised overflow flag changes nothing and stays raised, as with gan_bce_logits."""
    x = R.logits(count, count)
    xd = Guarded(ctx.device, count, data=torch.from_numpy(x))
    for target in (1.0, 0.0):
        ls_, gs_ = R.lsq_args(target)
        for ls in (None, R.LS_ON, R.LS_SKIP):
            st = scale_state(ctx, ls)
            ls0 = ls[0] if ls else 1.0
            dx = View(ctx.device, (1, 1, count, 1), 8, 0, ctx.tdtype)
            loss = Guarded(ctx.device, 1, data=torch.tensor([7.25]))
            rc = ctx.lib.gan_lsq_logits(xd.ptr, count, target, ls_, 0, loss.ptr, gs_, ctx.dt, dx.ptr, 8, ctx.ws_ptr, st.ptr if st else None,
                                        ctx.stream())
            assert rc == 0
            sync()
            got = float(loss.host()[0])
            tag = f't={target:g} ls={ls0:g}' + (' flag' if ls is R.LS_SKIP else '')
            for k, v in R.check_lsq(x, target, gs_, ls0, ctx.dt, got, dx.dense().reshape(-1), ls_).items():
                gate(ctx, 'gan_lsq_logits', f'{k} {tag}', v)
            assert dx.outside_untouched() and xd.untouched() and (st is None or st.untouched())
            # dx null, accumulate onto 1.5: the same deterministic loss, added in fp32
            acc = Guarded(ctx.device, 1, data=torch.tensor([1.5]))
            rc = ctx.lib.gan_lsq_logits(xd.ptr, count, target, ls_, 1, acc.ptr, gs_, ctx.dt, None, 8, ctx.ws_ptr, st.ptr if st else None,
                                        ctx.stream())
            assert rc == 0
            sync()
            assert R.check_accumulate(1.5, got, acc.host().numpy()[0]) == 0.0
            acc.changed()
            if ls is R.LS_SKIP and target == 1.0:
                # the cross-entropy kernel under the same raised flag: it too writes its whole gradient row and leaves the state alone
                bx = View(ctx.device, (1, 1, count, 1), 8, 0, ctx.tdtype)
                bl = Guarded(ctx.device, 1, data=torch.tensor([7.25]))
                assert ctx.lib.gan_bce_logits(xd.ptr, count, target, ls_, 0, bl.ptr, gs_, ctx.dt, bx.ptr, 8, ctx.ws_ptr, st.ptr,
                                              ctx.stream()) == 0
                sync()
                assert bool(bx.changed().view(count, 8)[:, 0].all()) and bx.outside_untouched() and st.untouched()
                assert bool(dx.changed().view(count, 8)[:, 0].all())


@pytest.mark.parametrize("count", R.FUSED_COUNTS)
def test_patchgan_losses_lsq(ctx, count):
    """gan_patchgan_losses_lsq: all three gradient maps, each pointer null in turn, l1 / gen_total null and non-null, with and without
    a scale state and with its flag raised; gan and disc against their gates, gen_total exactly the fp32 gan + lambda * l1."""
    real, fake = R.logits(count, count), R.logits(count, count + 1, -0.5)
    rd, fd = Guarded(ctx.device, count, data=torch.from_numpy(real)), Guarded(ctx.device, count, data=torch.from_numpy(fake))
    lam, l1v = R.LAM, R.L1V
    names = ('g_dfake', 'd_dreal', 'd_dfake')
    # (index of the null gradient or -1, scalars: both / none / gen_total without l1, scale state)
    for null, scalars, ls in ((-1, 'both', None), (0, 'none', R.LS_ON), (1, 'both', R.LS_ON), (2, 'gen', None), (-1, 'gen', R.LS_ON),
                              (-1, 'both', R.LS_SKIP)):
        st = scale_state(ctx, ls)
        ls0 = ls[0] if ls else 1.0
        maps = [View(ctx.device, (1, 1, count, 1), 8, 0, ctx.tdtype) if i != null else None for i in range(3)]
        losses = Guarded(ctx.device, 4)                    # [gen_total, gan, l1, disc], NaN
        losses.t[losses.lo + 2] = l1v
        losses.snap = _int_view(losses.t).cpu().clone()
        lp = losses.ptr
        rc = ctx.lib.gan_patchgan_losses_lsq(rd.ptr, fd.ptr, count, ctx.dt, *[m.ptr if m else None for m in maps], 8, lam,
                                             lp + 8 if scalars == 'both' else None, lp if scalars != 'none' else None, lp + 4, lp + 12,
                                             ctx.ws_ptr, st.ptr if st else None, ctx.stream())
        assert rc == 0
        sync()
        out = losses.host().numpy()
        got = dict(gan=out[1], disc=out[3], gen_total=out[0] if scalars != 'none' else None)
        got.update({k: m.dense().reshape(-1) if m else None for k, m in zip(names, maps)})
        tag = f'ls={ls0:g}' + (' flag' if ls is R.LS_SKIP else '')
        for k, v in R.check_fused(real, fake, ls0, ctx.dt, got, lam, l1v if scalars == 'both' else 0.0).items():
            gate(ctx, 'gan_patchgan_losses_lsq', f'{k} {tag}', v)
        ch = losses.changed()
        assert not ch[2] and (scalars != 'none' or not ch[0])            # l1 is only read; a null gen_total is not written
        assert all(m.outside_untouched() for m in maps if m) and rd.untouched() and fd.untouched() and (st is None or st.untouched())


# ---- one step per model against fp64 autograd ----------------------------------------------------------------------------------------
def _p2p_step(dtype, **kw):
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    ctx = Ctx('cuda:0', dtype)
    Gp, Dp, inp, tar, masks = R.p2p_setup()
    st = Pix2PixStep(ctx, 1, 256, 1, lam=100.0, seed=123, dropout=True, **kw)
    st.G.params.load_numpy(Gp)
    st.D.params.load_numpy(Dp)
    st.g.set_dropmasks(masks)
    return ctx, st, Gp, Dp, torch.from_numpy(inp).to(ctx.device), torch.from_numpy(tar).to(ctx.device)


@pytest.mark.parametrize("dtype", ['f32', 'bf16'])
def test_pix2pix_lsgan_step_against_fp64_autograd(dtype):
    """Pix2Pix, 256^2, batch 1, one channel, gan_loss='lsgan': the four losses, the generator output and every parameter gradient
    under the gates of test_gpu_step.py::test_pix2pix_train_step_parity (only the loss node differs).
    At batch 1 BatchNorm sees ONE value per channel at the 1 x 1 bottleneck: down7's normalised output is beta whatever its input,
    and the fp64 gradients of down7.kernel / down7.gamma are identically zero.  check_grads' error relative to max|ref| is not
    defined for such a tensor (that test runs at batch 2, where none exists), so these - and only tensors whose reference is
    exactly zero - are held to the same tolerance at the scale of their network's gradients: |got| <= f32_tol * the largest
    max|ref| of the network's tensors.  Measured on an MI355X: fp32 rounding noise of 1.1e-7 in G.down7.kernel."""
    ref = R.p2p_step_ref()
    ctx, st, Gp, Dp, ti, tt = _p2p_step(dtype, gan_loss='lsgan')
    assert st.gan_loss == 'lsgan'
    losses = st.train_step(ti, tt, True).cpu().numpy()
    gen = st.g.output_f32().cpu().numpy()
    err = float(np.abs(gen - ref['gen']).max())
    print(f"[{dtype}] lsgan pix2pix: generator max-abs err {err:.3e}; losses {losses} ref {ref['losses']}; reference max |logit| "
          f"{ref['logit_max']:.3f}; loss rel err {np.abs(losses / ref['losses'] - 1).max():.3e}")
    gG, gD = st.G.params.to_numpy('grad'), st.D.params.to_numpy('grad')
    pairs = [('G.' + k, gG[k], ref['gG'][k]) for k in ref['gG']] + [('D.' + k, gD[k], ref['gD'][k]) for k in ref['gD']]
    if dtype == 'f32':
        assert err < 1e-3 and np.allclose(losses, ref['losses'], rtol=2e-4)
    else:
        assert err < 0.04 and np.allclose(losses, ref['losses'], rtol=5e-3)
    zero = [p for p in pairs if not np.abs(p[2]).max() > 0]
    assert {n.split('.')[1] for n, _, _ in zero} <= {'down7'} and len(zero) <= 3, [n for n, _, _ in zero]
    check_grads(dtype, [p for p in pairs if np.abs(p[2]).max() > 0], 2e-2)
    for name, got, _ in zero:
        scale = max(np.abs(r).max() for n, _, r in pairs if n[0] == name[0])
        print(f"    [{dtype}] {name}: reference identically zero, max |got| {np.abs(got).max():.3e} against {2e-2 * scale:.3e}")
        if dtype == 'f32':
            assert np.abs(got).max() <= 2e-2 * scale, (name, float(np.abs(got).max()), scale)
    before = st.G.params.master.clone()          # training=False: the same loss, no update
    val = st.train_step(ti, tt, False).cpu().numpy()
    assert torch.equal(before, st.G.params.master) and np.isfinite(val).all()


@pytest.mark.parametrize("dtype", ['f32', 'bf16'])
def test_cyclegan_lsgan_step_against_fp64_autograd(dtype):
    """CycleGAN, 256^2, batch 1, one channel, gan_loss='lsgan': the seven losses, fake_y and the gradients of all four networks
    under the gates of test_gpu_step.py::test_cyclegan_train_step_parity."""
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep
    ref = R.cyc_step_ref()
    Ps, rx, ry, masks = R.cyc_setup()
    ctx = Ctx('cuda:0', dtype)
    st = CycleGANStep(ctx, 1, 256, 1, lam=10.0, seed=7, dropout=True, gan_loss='lsgan')
    for net, P in zip(st.nets(), Ps):
        net.params.load_numpy(P)
    for k, call in st.gen_calls().items():
        call.set_dropmasks(masks[k])
    losses = st.train_step(torch.from_numpy(rx).to(ctx.device), torch.from_numpy(ry).to(ctx.device), True).cpu().numpy()
    fy = st.fy.output_f32().cpu().numpy()
    err = float(np.abs(fy - ref['fake_y']).max())
    print(f"[{dtype}] lsgan cyclegan: fake_y max-abs err {err:.3e}; losses {losses} ref {ref['losses']}; reference max |logit| "
          f"{ref['logit_max']:.3f}; loss rel err {np.abs(losses / ref['losses'] - 1).max():.3e}")
    if dtype == 'f32':
        assert err < 1e-3 and np.allclose(losses, ref['losses'], rtol=5e-4)
    else:
        assert err < 0.025 and np.allclose(losses, ref['losses'], rtol=5e-3)
    pairs = []
    for nm, net, g in zip(('Gg', 'Gf', 'Dx', 'Dy'), st.nets(), ref['grads']):
        got = net.params.to_numpy('grad')
        pairs += [(nm + '.' + k, got[k], g[k]) for k in g]
    check_grads(dtype, pairs, 1e-1)


# ---- launch lists --------------------------------------------------------------------------------------------------------------------------
OLD, NEW = ('gan_bce_logits', 'gan_patchgan_losses'), ('gan_lsq_logits', 'gan_patchgan_losses_lsq')
BACK = dict(zip(NEW, OLD))


def _scalars(call):
    """The non-pointer arguments of a loss call (buffers differ from one step object to the next)."""
    return tuple(a for a in call.args if isinstance(a, (int, float)) and not (isinstance(a, int) and a > 1 << 20))


def _captured(model, monkeypatch, **kw):
    import gc
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep, Pix2PixStep
    gc.collect()
    torch.cuda.synchronize()
    rec = A.Recorder(monkeypatch)
    rec.hook_capture(monkeypatch)
    ctx = Ctx('cuda:0', 'bf16')
    st = Pix2PixStep(ctx, 1, 256, 1, lam=100.0, seed=123, **kw) if model == 'pix2pix' else CycleGANStep(ctx, 1, 256, 1, lam=10.0, seed=123, **kw)
    st.capture(training=True)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return [(c.name, _scalars(c) if c.name in OLD + NEW else None) for c in rec.calls]


@pytest.mark.parametrize("model", ['pix2pix', 'cyclegan'])
def test_launch_lists(model, monkeypatch):
    """A captured 'lsgan' step records the new entry points and none of the cross-entropy ones; the default and an explicit 'bce'
    record one and the same sequence, cross-entropy calls only; and the 'lsgan' sequence is that sequence with the loss entry points
    exchanged one for one - same positions, same scalar arguments: neither schedule changes shape."""
    default = _captured(model, monkeypatch)
    explicit = _captured(model, monkeypatch, gan_loss='bce')
    lsgan = _captured(model, monkeypatch, gan_loss='lsgan')
    names = lambda seq: [n for n, _ in seq]
    assert default == explicit and not set(names(default)) & set(NEW)
    n_old = sum(n in OLD for n in names(default))
    assert n_old == (1 if model == 'pix2pix' else 6) and names(default).count(OLD[model == 'pix2pix']) == n_old
    assert not set(names(lsgan)) & set(OLD) and sum(n in NEW for n in names(lsgan)) == n_old
    assert [(BACK.get(n, n), a) for n, a in lsgan] == default
    print(f"[{model}] {len(default)} recorded calls, {n_old} loss calls exchanged")


def test_pix2pix_lsgan_with_dssim_captures_and_matches_the_eager_losses(tmp_path):
    """gan_loss='lsgan' with generator_loss='dssim' (the dSSIM call replaces only the L1 call): the model's captured step replays with
    finite losses equal to the eager generator_loss / discriminator_loss on the step's own logits and output, within the fp32 step
    gate (rtol 2e-4, test_gpu_step.py)."""
    from gan_amd import pix2pix
    m = pix2pix.Pix2Pix(vars(pix2pix.parse_opt(['--data', str(tmp_path), '--output', str(tmp_path), '--train', '--epochs', '1', '--dtype', 'f32',
                                               '--gan-loss', 'lsgan', '--generator-loss', 'dssim'])))
    _, _, inp, tar, _ = R.p2p_setup()
    x, y = torch.from_numpy(inp).to(m.ctx.device), torch.from_numpy(tar).to(m.ctx.device)
    first = torch.stack(m.train_step(x, y, training=False)).cpu().numpy()
    again = torch.stack(m.train_step(x, y, training=False)).cpu().numpy()            # a second replay of the same graph: new dropout masks,
                                                                                     # and it is its logits and output the buffers hold
    st = m._steps[(1, False)][0]
    assert st.gan_loss == 'lsgan' and st.generator_loss == 'dssim'
    torch.cuda.synchronize()
    real = A.read(*st.d.logits_view(0)).to(m.ctx.device)
    fake = A.read(*st.d.logits_view(1)).to(m.ctx.device)
    gen = st.g.output_f32()
    total, gan, second = m.generator_loss(fake, gen, y, x)
    disc = m.discriminator_loss(real, fake, 0.5)
    eager = np.array([float(total), float(gan), float(second), float(disc)])
    print(f"lsgan + dssim f32: replayed {first} then {again}; eager on the second replay's buffers {eager}")
    assert np.isfinite(first).all() and np.isfinite(again).all()
    assert np.allclose(again, eager, rtol=2e-4) and 0.0 < again[2] < 2.0
    # the eager adversarial terms are the least-squares ones of these very logits
    assert abs(eager[1] - float(((fake.double() - 1) ** 2).mean())) <= 2e-4 * eager[1]
    trained = torch.stack(m.train_step(x, y, training=True)).cpu().numpy()
    assert np.isfinite(trained).all()


# ---- data parallel: the bucketed and the phased schedule behind a stub exchange ------------------------------------------------------
@pytest.mark.parametrize("buckets", ['1', '0'])
def test_ddp_schedules_with_lsgan_match_the_one_gpu_step(buckets):
    """Pix2Pix f32, batch 1, gan_loss='lsgan': the bucketed (4 compute graphs) and the phased data-parallel schedule, forced on one GPU
    by test_gpu_step.py's world-2 stub exchange (gradients unchanged), against the one-GPU 'lsgan' step: the same losses, the same
    gradients and the same weights after the update (the gates of test_ddp_schedules_match_single_graph)."""
    ctx, st, Gp, Dp, ti, tt = _p2p_step('f32', gan_loss='lsgan')
    l_ref = st.train_step(ti, tt, True).cpu().numpy().copy()
    g_ref = [n.params.grad.clone() for n in st.nets()]
    w_ref = [n.params.master.clone() for n in st.nets()]
    ctx2, st2, *_ = _p2p_step('f32', gan_loss='lsgan')
    st2.sync = _FakeSync()
    st2.ddp_buckets = buckets == '1'
    replay = st2.capture(training=True)
    st2.G.params.load_numpy(Gp); st2.D.params.load_numpy(Dp)
    for ps in (st2.G.params, st2.D.params):
        ps.m.zero_(); ps.v.zero_(); ps.step.zero_()
    losses = replay(ti, tt)[:4].cpu().numpy()
    torch.cuda.synchronize()
    assert hasattr(st2, 'buckets') == (buckets == '1')
    assert np.allclose(losses, l_ref, rtol=1e-5), (losses, l_ref)
    for a, b in zip(g_ref, (n.params.grad for n in st2.nets())):
        assert float((a - b).norm() / a.norm()) <= 1e-6
    for a, b in zip(w_ref, (n.params.master for n in st2.nets())):
        assert torch.allclose(a, b, atol=1e-6), float((a - b).abs().max())


# ---- one command-line run per model ---------------------------------------------------------------------------------------------------
def _strict(p):
    return json.loads(open(p).read(), parse_constant=lambda s: pytest.fail(f"not strict JSON: {s} in {p}"))


def _examples():
    return np.load(os.path.join(R.ROOT, 'tests', 'golden', 'example_pairs_256.npz'))


def _check_run(out, losses_file_keys=None):
    run = os.path.join(out, sorted(os.listdir(out))[0])
    logs = os.path.join(run, 'logs')
    assert _strict(os.path.join(logs, 'config.json'))['gan_loss'] == 'lsgan'
    for name in ('train_metrics.json', 'val_metrics.json'):
        metrics = _strict(os.path.join(logs, name))
        assert metrics
        for key, vals in metrics.items():
            assert len(vals) == 1 and all(np.isfinite(v) for v in vals), (name, key, vals)
    return os.path.join(run, 'training_checkpoints')


def test_pix2pix_cli_trains_with_gan_loss_lsgan(tmp_path):
    from PIL import Image
    from gan_amd import pix2pix
    from gan_amd.checkpoint import Checkpoint, latest_checkpoint
    ex = _examples()
    data, out = str(tmp_path / 'data'), str(tmp_path / 'out')
    os.makedirs(data)
    for i in range(8):
        a, b = ex['input_u8'][i % 2, :, :, 0], ex['target_u8'][i % 2, :, :, 0]
        a, b = (a[:, ::-1], b[:, ::-1]) if (i // 2) % 2 else (a, b)
        Image.fromarray(np.concatenate([np.roll(a, 16 * (i // 4), 0), np.roll(b, 16 * (i // 4), 0)], axis=1), 'L').save(os.path.join(data, f"p{i}.png"))
    args = ['--data', data, '--output', out, '--train', '--epochs', '1', '--batch-size', '2', '--test-img', '1', '--logging', 'false',
            '--seed', '7', '--gan-loss', 'lsgan']
    pix2pix.main(pix2pix.parse_opt(args))
    ck = _check_run(out)
    p = pix2pix.Pix2Pix(vars(pix2pix.parse_opt(args)))
    before = p.generator.net.params.master.clone()
    Checkpoint(generator=p.generator, discriminator=p.discriminator, generator_optimizer=p.generator_optimizer,
               discriminator_optimizer=p.discriminator_optimizer).restore(latest_checkpoint(ck))
    after = p.generator.net.params.master
    assert torch.isfinite(after).all() and not torch.equal(before, after) and int(p.generator_optimizer.params.step) > 0


def test_cyclegan_cli_trains_with_gan_loss_lsgan(tmp_path):
    from PIL import Image
    from gan_amd import cycle_gan
    from gan_amd.checkpoint import Checkpoint, latest_checkpoint
    ex = _examples()
    dx, dy, out = str(tmp_path / 'X'), str(tmp_path / 'Y'), str(tmp_path / 'out')
    for d, key in ((dx, 'input_u8'), (dy, 'target_u8')):
        os.makedirs(d)
        for i in range(6):
            a = ex[key][i % 2, :, :, 0]
            Image.fromarray(np.roll(a[:, ::-1] if (i // 2) % 2 else a, 16 * (i // 4), 0), 'L').save(os.path.join(d, f"s{i}.png"))
    args = ['--input-images', dx, '--target-images', dy, '--output', out, '--train', '--epochs', '1', '--test-img', '1',
            '--validation-size', '0.2', '--logging', 'false', '--gan-loss', 'lsgan']
    cycle_gan.main(cycle_gan.parse_opt(args))
    ck = _check_run(out)
    c = cycle_gan.CycleGAN(vars(cycle_gan.parse_opt(args)))
    names = ('generator_g', 'generator_f', 'discriminator_x', 'discriminator_y')
    objects = {n: getattr(c, n) for n in names}
    objects.update({n + '_optimizer': getattr(c, n + '_optimizer') for n in names})
    before = c.generator_g.net.params.master.clone()
    Checkpoint(**objects).restore(latest_checkpoint(ck))
    after = c.generator_g.net.params.master
    assert torch.isfinite(after).all() and not torch.equal(before, after) and int(c.generator_g_optimizer.params.step) > 0
