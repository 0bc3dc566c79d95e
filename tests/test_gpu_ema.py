"""Generator weight averaging on the GPU: gan_ema_update per element against the fp64 reference and gate of tests/ema_ref.py
(proven on the CPU by tests/test_cpu_ema.py), the step hook (it must not perturb training), WeightAverage.averaged(), the
checkpoint object on the device and the three CLI flags end to end."""
import json
import os

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from tests import ema_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one vector; one arena unit; a ragged last block; one vector more than the capped grid covers in a trip (the stride loop runs twice)
COUNTS = (4, 64, 1028, 4096 * 256 * 4 + 4)


def bits(t):
    return t.detach().view(torch.int32).cpu().numpy().copy()


def _guarded(data, dev):
    t = torch.full((GUARD + data.size + GUARD,), float('nan'), dtype=torch.float32, device=dev)
    t[GUARD:GUARD + data.size] = torch.from_numpy(data).to(dev)
    return t


@pytest.mark.parametrize("count", COUNTS)
def test_kernel_per_element_against_fp64(count):
    """gan_ema_update: every element within the gate, the reported d_t within one ulp, for constant decay and the warm-up form on
    both sides of the crossover; guards unwritten, param unchanged, a second call from the same inputs gives the same bits, and a
    refused call writes nothing."""
    lib, dev = L.load(), torch.device('cuda:0')
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    s, w = R.planted(count, seed=count)
    wt = _guarded(w, dev)
    w_bits = bits(wt)
    worst = 0.0
    for decay in (0.999, 0.5):
        for step in (None, 1, 10, 8990, 100000):
            outs = []
            for _ in range(2):
                st = _guarded(s, dev)
                used = torch.full((3,), float('nan'), dtype=torch.float32, device=dev)
                stp = torch.tensor([step if step is not None else -7], dtype=torch.int32, device=dev)
                rc = lib.gan_ema_update(st.data_ptr() + 4 * GUARD, wt.data_ptr() + 4 * GUARD, count, decay,
                                        stp.data_ptr() if step is not None else None, used.data_ptr() + 4, stream())
                assert rc == 0
                torch.cuda.synchronize()
                outs.append((bits(st), used.cpu().numpy(), int(stp.item())))
            (b0, u0, t0), (b1, u1, _) = outs
            assert np.array_equal(b0, b1) and np.array_equal(u0.view(np.uint32), u1.view(np.uint32)), "two calls, different bits"
            assert np.isnan(u0[0]) and np.isnan(u0[2]) and t0 == (step if step is not None else -7)      # one float written; *step only read
            full = b0.view(F32)
            assert np.isnan(full[:GUARD]).all() and np.isnan(full[GUARD + count:]).all(), "a guard word of shadow was written"
            assert np.array_equal(bits(wt), w_bits), "param was written"
            got, du = full[GUARD:GUARD + count], F32(u0[1])
            assert R.decay_ok(du, decay, step), (decay, step, du, R.decay_at(decay, step))
            bad = R.element_failures(s, w, got, du)
            ratio = R.worst_ratio(s, w, got, du)
            worst = max(worst, ratio)
            assert bad.size == 0, (count, decay, step, ratio, bad[:4], s[bad[:4]], w[bad[:4]], got[bad[:4]])
    print(f"gan_ema_update count {count}: worst |got - ref| / gate {worst:.3f}")
    # refused calls: nothing is written
    st = _guarded(s, dev)
    used = torch.full((1,), float('nan'), dtype=torch.float32, device=dev)
    before = bits(st)
    p, q = st.data_ptr() + 4 * GUARD, wt.data_ptr() + 4 * GUARD
    for args in ((p + 4, q, 4, 0.5), (p, q + 8, 4, 0.5), (p, q, count + 2, 0.5), (p, q, 0, 0.5), (p, q, count, 1.0), (p, q, count, -0.1),
                 (None, q, count, 0.5), (p, None, count, 0.5)):
        assert lib.gan_ema_update(args[0], args[1], args[2], args[3], None, used.data_ptr(), stream()) == L.E_ARG, args
    torch.cuda.synchronize()
    assert np.array_equal(bits(st), before) and np.isnan(used.item()) and np.array_equal(bits(wt), w_bits)


# ---- the step hook -----------------------------------------------------------------------------------------------------------------
DECAY = 0.999


def _inputs(dev, batch, seed=5):
    rng = np.random.default_rng(seed)
    mk = lambda: torch.from_numpy(rng.uniform(-1, 1, (batch, 256, 256, 1)).astype(F32)).to(dev)
    return mk(), mk()


def _check_update(prev, master, new, t, what):
    """`new` is one update of the fp32 shadow `prev` towards `master` at step count t, per element within the gate."""
    du = F32(R.decay_at(DECAY, t))              # the kernel rounds the fp64 d_t once (checked in test_kernel_per_element_against_fp64)
    bad = R.element_failures(prev, master, new, du)
    assert bad.size == 0, (what, t, R.worst_ratio(prev, master, new, du), bad[:4])
    assert not np.array_equal(prev, new), what


@pytest.fixture(scope="module")
def hooked():
    """Two captured Pix2Pix steps from the same seed, three replays each on the same inputs; the second carries a weight average."""
    from gan_amd.base_gan import GeneratorModel
    from gan_amd.ema import WeightAverage
    from gan_amd.nets import Ctx, workspace_mb_for
    from gan_amd.steps import Pix2PixStep
    dev = torch.device('cuda:0')
    x, y = _inputs(dev, 2)
    runs = []
    for with_ema in (False, True):
        ctx = Ctx('cuda:0', 'bf16', workspace_mb=workspace_mb_for(2, 256, 1))
        st = Pix2PixStep(ctx, 2, 256, 1, seed=123)
        replay = st.capture(training=True)
        model = GeneratorModel(st.G)
        ema, trace = None, []
        if with_ema:
            ema = WeightAverage(model, DECAY, True)           # (after the capture's warm-up steps: seeded from the weights as they are now)
            st.ema = (ema,)
            trace.append((ema.shadow.cpu().numpy(), None, None))
        losses = []
        for _ in range(3):
            losses.append(replay(x, y).clone())
            torch.cuda.synchronize()
            if with_ema:
                trace.append((ema.shadow.cpu().numpy(), st.G.params.master.cpu().numpy(), int(st.G.params.step.item())))
        runs.append(dict(ctx=ctx, st=st, model=model, ema=ema, trace=trace, losses=torch.stack(losses).cpu(), x=x, y=y))
    return runs


def test_hook_does_not_perturb_training(hooked):
    plain, avg = hooked
    assert torch.equal(plain['losses'].view(torch.int32), avg['losses'].view(torch.int32))
    for net in ('G', 'D'):
        pa, pb = getattr(plain['st'], net).params, getattr(avg['st'], net).params
        for which in ('master', 'm', 'v', 'step'):
            assert np.array_equal(bits(getattr(pa, which)), bits(getattr(pb, which))), (net, which)
    trace = avg['trace']
    steps = [t for _, _, t in trace[1:]]
    assert steps == [steps[0], steps[0] + 1, steps[0] + 2]
    for k in range(1, 4):
        _check_update(trace[k - 1][0], trace[k][1], trace[k][0], trace[k][2], f'replay {k}')
    assert not hasattr(plain['st'].D, 'ema') and plain['st'].ema == ()


def test_validation_replay_leaves_the_shadow_alone(hooked):
    from gan_amd.steps import Pix2PixStep
    avg = hooked[1]
    st = avg['st']
    ps = (st.G.params, st.D.params)
    saved = [(p.master.clone(), p.m.clone(), p.v.clone(), p.step.clone(), {k: v.clone() for k, v in p.state.items()}) for p in ps]
    val = Pix2PixStep(avg['ctx'], 2, 256, 1, seed=123, nets=(st.G, st.D), mask_stream=16)
    val.ema = (avg['ema'],)                                   # even when handed one, a training=False replay never updates
    replay = val.capture(training=False)
    before = bits(avg['ema'].shadow)
    replay(avg['x'], avg['y'])
    torch.cuda.synchronize()
    assert np.array_equal(bits(avg['ema'].shadow), before)
    for p, (w, m, v, step, state) in zip(ps, saved):          # (undo the capture's warm-up pass for the tests that follow)
        p.master.copy_(w); p.m.copy_(m); p.v.copy_(v); p.step.copy_(step)
        for k, t in state.items():
            p.state[k].copy_(t)
        p.prepare()
    torch.cuda.synchronize()


def test_averaged_lends_the_shadow_and_gives_the_weights_back(hooked):
    """Inside averaged(): infer == a fresh model loaded with the shadow (moving statistics copied), bit for bit; afterwards, also
    after an exception, master and every typed copy are what they were."""
    from gan_amd.base_gan import GeneratorModel
    from gan_amd.nets import GeneratorNet
    avg = hooked[1]
    st, model, ema, x = avg['st'], avg['model'], avg['ema'], avg['x']
    ps = st.G.params
    replay_state = lambda: [bits(ps.master)] + [bits(ps.nat[k]) for k in ps.nat] + [bits(ps.tr[k]) for k in ps.tr]
    before, shadow_before = replay_state(), bits(ema.shadow)
    raw = model.infer(x).clone()
    fresh = GeneratorModel(GeneratorNet(avg['ctx'], 1, 'batchnorm', seed=77))
    fresh.net.params.master.copy_(ema.shadow)
    for k, t in ps.state.items():
        fresh.net.params.state[k].copy_(t)
    fresh.net.params.prepare()
    want = fresh.infer(x).clone()
    with ema.averaged() as m:
        assert m is model and np.array_equal(bits(ps.master), shadow_before)
        got = model.infer(x).clone()
        with pytest.raises(L.GanAmdError):
            ema.update()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got, raw)
    after = replay_state()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and np.array_equal(bits(ema.shadow), shadow_before)
    assert torch.equal(model.infer(x).view(torch.int32), raw.view(torch.int32))
    with pytest.raises(RuntimeError, match='boom'):
        with ema.averaged():
            raise RuntimeError('boom')
    after = replay_state()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and np.array_equal(bits(ema.shadow), shadow_before)


def test_cyclegan_step_moves_both_generator_averages():
    from gan_amd.base_gan import GeneratorModel
    from gan_amd.ema import WeightAverage
    from gan_amd.nets import Ctx, workspace_mb_for
    from gan_amd.steps import CycleGANStep
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=workspace_mb_for(1, 256, 1))
    st = CycleGANStep(ctx, 1, 256, 1, seed=123)
    replay = st.capture(training=True)
    emas = tuple(WeightAverage(GeneratorModel(net, name), DECAY, True) for net, name in ((st.Gg, 'generator_g'), (st.Gf, 'generator_f')))
    st.ema = emas
    x, y = _inputs(ctx.device, 1, seed=9)
    prev = [e.shadow.cpu().numpy() for e in emas]
    d_before = [bits(n.params.master) for n in (st.Dx, st.Dy)]
    for k in range(2):
        replay(x, y)
        torch.cuda.synchronize()
        for i, (e, net) in enumerate(zip(emas, (st.Gg, st.Gf))):
            new = e.shadow.cpu().numpy()
            _check_update(prev[i], net.params.master.cpu().numpy(), new, int(net.params.step.item()), f'generator {i} replay {k}')
            prev[i] = new
    assert len(st.ema) == 2 and all(e.params in (st.Gg.params, st.Gf.params) for e in st.ema)      # the discriminators have none
    assert all(not np.array_equal(b, bits(n.params.master)) for b, n in zip(d_before, (st.Dx, st.Dy)))   # (they did train)


# ---- classes, checkpoints, CLI -----------------------------------------------------------------------------------------------------
def _dataset(root, n=8):
    """n pair images (input | target, 256 x 512) from the two committed example pairs, mirrored and shifted."""
    from PIL import Image
    ex = np.load(os.path.join(ROOT, 'tests', 'golden', 'example_pairs_256.npz'))
    data = os.path.join(root, 'data')
    os.makedirs(data)
    for i in range(n):
        a, b = ex['input_u8'][i % 2, :, :, 0], ex['target_u8'][i % 2, :, :, 0]
        if (i // 2) % 2:
            a, b = a[:, ::-1], b[:, ::-1]
        a, b = np.roll(a, 16 * (i // 4), axis=0), np.roll(b, 16 * (i // 4), axis=0)
        Image.fromarray(np.concatenate([a, b], axis=1), 'L').save(os.path.join(data, f"p{i}.png"))
    return data


def _p2p(tmp, extra=()):
    from gan_amd import pix2pix
    return pix2pix.Pix2Pix(vars(pix2pix.parse_opt(['--data', str(tmp), '--output', str(tmp), '--train', '--epochs', '1', '--batch-size', '2',
                                                   *extra])))


def _checkpoint(m):
    from gan_amd.checkpoint import Checkpoint
    objects = dict(generator_optimizer=m.generator_optimizer, discriminator_optimizer=m.discriminator_optimizer,
                   generator=m.generator, discriminator=m.discriminator)
    if m.generator_ema is not None:
        objects['generator_ema'] = m.generator_ema
    return Checkpoint(**objects)


def test_checkpoint_round_trip_on_the_device(tmp_path):
    from gan_amd import tfbundle as TB
    x, y = _inputs(torch.device('cuda:0'), 2, seed=11)
    m = _p2p(tmp_path, ['--ema-decay', '0.9'])
    assert m.generator_ema is not None and m.generator_ema.decay == 0.9 and m.generator_ema.warmup
    assert _p2p(tmp_path).generator_ema is None
    for _ in range(3):
        m.train_step(x, y)
    assert m._steps[(2, True)][0].ema == (m.generator_ema,)
    torch.cuda.synchronize()
    assert not torch.equal(m.generator_ema.shadow, m.generator.net.params.master)
    with_ema = str(tmp_path / 'with' / 'ckpt-1')
    os.makedirs(os.path.dirname(with_ema))
    _checkpoint(m).write(with_ema)
    keys = set(TB.read_bundle(with_ema)[0])
    assert 'generator_ema/layer_with_weights-0/layer_with_weights-0/kernel/.ATTRIBUTES/VARIABLE_VALUE' in keys
    assert not any('moving' in k for k in keys if k.startswith('generator_ema/'))            # trainable variables only
    fresh = _p2p(tmp_path, ['--ema-decay', '0.9', '--seed', '5'])
    _checkpoint(fresh).restore(with_ema)
    assert fresh.generator_ema.loaded is True
    assert np.array_equal(bits(fresh.generator_ema.shadow), bits(m.generator_ema.shadow))
    assert np.array_equal(bits(fresh.generator.net.params.master), bits(m.generator.net.params.master))
    # a checkpoint written without the average: exactly the keys of a run without the feature, and the average starts over
    plain = _p2p(tmp_path)
    without = str(tmp_path / 'without' / 'ckpt-1')
    os.makedirs(os.path.dirname(without))
    _checkpoint(plain).write(without)
    assert not any('_ema' in k for k in TB.read_bundle(without)[0])
    assert keys - set(TB.read_bundle(without)[0]) == {k for k in keys if k.startswith('generator_ema/')}
    late = _p2p(tmp_path, ['--ema-decay', '0.9', '--seed', '6'])
    late.generator_ema.loaded = True
    _checkpoint(late).restore(without)
    assert late.generator_ema.loaded is False
    assert np.array_equal(bits(late.generator_ema.shadow), bits(plain.generator.net.params.master))
    assert np.array_equal(bits(late.generator.net.params.master), bits(plain.generator.net.params.master))


def _run_dir(out):
    return os.path.join(out, sorted(os.listdir(out))[0])


def test_cli_end_to_end(tmp_path, capsys):
    from gan_amd import pix2pix
    from gan_amd import tfbundle as TB
    from gan_amd.checkpoint import latest_checkpoint
    data = _dataset(str(tmp_path))
    base = ['--data', data, '--train', '--epochs', '1', '--batch-size', '2', '--test-img', '2', '--logging', 'false', '--seed', '7']
    strict = lambda p: json.loads(open(p).read(), parse_constant=lambda s: pytest.fail(f"not strict JSON: {s} in {p}"))
    out = str(tmp_path / 'out_ema')
    pix2pix.main(pix2pix.parse_opt(base + ['--output', out, '--ema-decay', '0.9', '--quality-metrics', 'true']))
    logs = os.path.join(_run_dir(out), 'logs')
    val, val_ema = strict(os.path.join(logs, 'val_quality.json')), strict(os.path.join(logs, 'val_quality_ema.json'))
    assert sorted(val_ema) == sorted(val) == ['MAE', 'PSNR', 'SSIM'] and all(len(v) == 1 and np.isfinite(v[0]) for v in val_ema.values())
    test, test_ema = strict(os.path.join(logs, 'test_quality.json')), strict(os.path.join(logs, 'test_quality_ema.json'))
    assert sorted(test_ema) == sorted(test) == ['mean', 'per_image']
    assert all(len(test_ema['per_image'][k]) == 2 and np.isfinite(test_ema['per_image'][k]).all() for k in ('SSIM', 'PSNR', 'MAE', 'MSE'))
    assert test_ema['per_image'] != test['per_image']                      # a different set of weights made them
    ck = os.path.join(_run_dir(out), 'training_checkpoints')
    assert any(k.startswith('generator_ema/') for k in TB.read_bundle(latest_checkpoint(ck))[0])
    pred = str(tmp_path / 'pred_ema')
    pix2pix.main(pix2pix.parse_opt(['--data', data, '--predict', '--weights', ck, '--logging', 'false', '--batch-size', '4', '--output', pred,
                                    '--predict-weights', 'ema', '--predict-training', 'false']))
    imgs = os.listdir(os.path.join(_run_dir(pred), 'prediction_images'))
    assert sorted(imgs) == sorted(f'img{k}.png' for k in range(8))
    # default flags: no averaged weights in the checkpoint, and predicting from them is refused before any image is written
    out2 = str(tmp_path / 'out_plain')
    pix2pix.main(pix2pix.parse_opt(base + ['--output', out2]))
    ck2 = os.path.join(_run_dir(out2), 'training_checkpoints')
    assert not any('_ema' in k for k in TB.read_bundle(latest_checkpoint(ck2))[0])
    assert not os.path.exists(os.path.join(_run_dir(out2), 'logs', 'val_quality_ema.json'))
    pred2 = str(tmp_path / 'pred_refused')
    with pytest.raises(SystemExit) as exc:
        pix2pix.main(pix2pix.parse_opt(['--data', data, '--predict', '--weights', ck2, '--logging', 'false', '--output', pred2,
                                        '--predict-weights', 'ema', '--predict-training', 'false']))
    assert exc.value.code not in (0, None) and 'checkpoint holds no averaged weights' in str(exc.value.code)
    assert not any(f.endswith('.png') for _, _, fs in os.walk(pred2) for f in fs)
