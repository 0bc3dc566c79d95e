"""Inference mode (`model(x, training=False)`): Keras BatchNormalization with its moving statistics, Dropout as the identity.
BatchNorm layers run as one convolution each on weights folded with the moving statistics (gan_bn_fold_multi).

The reference for inference mode lives in tests/inference_ref.py: an fp64 numpy forward built from the oracle's primitives
(O.conv2d_fwd, O.convT2d_fwd, O.act_fwd, O.BN_EPS) with BN in its inference form and no dropout.  tests/test_cpu_inference.py
checks it against torch.nn.functional.batch_norm(training=False)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import gan_oracle as O
from tests.inference_ref import (_f64, _np_fold, bn_eval, calibrated, disc_params, discriminator_eval_ref, gen_params,      # noqa: F401
                                 generator_eval_ref)

pytestmark = pytest.mark.gpu

G_BN = [f'down{i}' for i in range(1, 8)] + [f'up{j}' for j in range(7)]
D_BN = ['down1', 'down2', 'conv']


def _gen(dtype, P=None, norm='batchnorm'):
    from gan_amd.base_gan import GeneratorModel
    from gan_amd.nets import Ctx, GeneratorNet, workspace_mb_for
    ctx = Ctx('cuda:0', dtype, workspace_mb=workspace_mb_for(4, 512))
    net = GeneratorNet(ctx, 1, norm, seed=5)
    if P is not None:
        net.params.load_numpy(P)
    return GeneratorModel(net)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the fold kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16', 'f16'])
def test_bn_fold_multi_matches_numpy(dtype):
    from gan_amd import _lib as L
    from gan_amd.nets import Ctx, pad8
    ctx = Ctx('cuda:0', dtype)
    rng = np.random.default_rng(3)
    # (A, B, transposed): Conv2D entries have A = Cin, B = Cout; Conv2DTranspose entries A = Cout, B = Cin
    shapes = [(12, 70, 1), (64, 128, 1), (96, 20, 0), (128, 64, 0), (5, 3, 0)]
    ents, tiles, keep, exp = [], 0, [], []
    for A, B, tr in shapes:
        co, ci = (B, A) if tr else (A, B)
        master = (0.05 * rng.standard_normal((4, 4, A, B))).astype(np.float32)
        gamma = (rng.uniform(0.5, 1.5, co) * rng.choice([-1, 1], co)).astype(np.float32)
        beta = rng.normal(0, 0.3, co).astype(np.float32)
        mean = rng.normal(0, 0.5, co).astype(np.float32)
        var = rng.uniform(0.01, 3.0, co).astype(np.float32)
        dev = [torch.from_numpy(a).cuda() for a in (master, gamma, beta, mean, var)]
        bias = torch.full((co,), 7.0, dtype=torch.float32, device='cuda')
        nk = torch.full((16, co, pad8(ci)), 3.0, dtype=ctx.tdtype, device='cuda')      # pad columns must be overwritten with 0
        tk = (pad8(ci) + 63) // 64
        ents.append(L.GanFoldEntry(*[t.data_ptr() for t in dev], bias.data_ptr(), nk.data_ptr(), A, B, tr, tiles, tk))
        tiles += 16 * ((co + 63) // 64) * tk
        keep += dev + [bias, nk]
        exp.append((dev, bias, nk, _np_fold(master, gamma, beta, mean, var, tr), (master, gamma, beta, mean, var), ci))
    arr = (L.GanFoldEntry * len(ents))(*ents)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    L.check(ctx.lib.gan_bn_fold_multi(table.data_ptr(), len(ents), tiles, ctx.dt, O.BN_EPS, ctx.stream()), "bn_fold_multi")
    torch.cuda.synchronize()
    for dev, bias, nk, (s, b_ref, w_ref), host, ci in exp:
        assert np.array_equal(bias.cpu().numpy().view(np.uint32), b_ref.view(np.uint32))          # fp32 bias: bit-exact
        got = nk.float().cpu().numpy()
        assert not got[:, :, ci:].any()                                                           # pad8 columns: zeros
        got = got[:, :, :ci]
        if dtype == 'f32':
            ulp = np.spacing(np.abs(w_ref)).astype(np.float64)
            assert (np.abs(got.astype(np.float64) - w_ref) <= ulp).all()                          # within 1 ulp
        else:                                                                                     # one rounding of the fp32 product
            want = torch.from_numpy(w_ref).to(ctx.tdtype).float().numpy()
            assert np.array_equal(got, want)
        for t, h in zip(dev, host):                                                               # inputs untouched
            assert np.array_equal(t.cpu().numpy(), h)


def test_fold_leaves_the_training_weights_untouched():
    """The fold of a whole network writes only its own buffers: master, the NK copies the training step reads (nat / tr) and the
    moving statistics are unchanged; the folded weights of a Conv2D and a Conv2DTranspose layer match numpy."""
    m = _gen('bf16', gen_params())
    ps = m.net.params
    before = (ps.master.clone(), {k: v.clone() for k, v in ps.nat.items()}, {k: v.clone() for k, v in ps.tr.items()},
              {k: v.clone() for k, v in ps.state.items()})
    m.fold()
    torch.cuda.synchronize()
    assert torch.equal(before[0], ps.master)
    assert all(torch.equal(before[1][k], ps.nat[k]) and torch.equal(before[2][k], ps.tr[k]) for k in ps.nat)
    assert all(torch.equal(before[3][k], ps.state[k]) for k in ps.state)
    P = ps.to_numpy()
    F = m.net.folded()
    for name, tr in (('down3', 1), ('up2', 0)):
        _, b_ref, w_ref = _np_fold(P[name + '.kernel'], P[name + '.gamma'], P[name + '.beta'], P[name + '.moving_mean'],
                                   P[name + '.moving_variance'], tr)
        assert np.array_equal(F.bias[name].cpu().numpy(), b_ref)
        assert np.array_equal(F.nk[name].float().cpu().numpy(), torch.from_numpy(w_ref).bfloat16().float().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# 2. generator parity against the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,S', [(1, 256), (4, 256), (2, 512)])
def test_generator_eval_parity_batchnorm(B, S):
    P = gen_params(S=S)
    x = O.synthetic_pair(B, S, 1, seed=40 + B)[0]
    ref, a7_ref = generator_eval_ref(P, x)
    errs = {}
    for dtype, gate in (('f32', 1e-4), ('bf16', 5e-2)):
        m = _gen(dtype, P)
        out = m(torch.from_numpy(x), training=False).cpu().numpy()
        errs[dtype] = float(np.abs(out - ref).max())
        if dtype == 'f32':
            a7 = m._eval_calls[(B, S)].a7.t.float().cpu().numpy()
            assert np.abs(a7 - a7_ref).max() < 1e-4 * max(1.0, np.abs(a7_ref).max())
            if B == 1:     # training mode at batch 1: the 1x1 bottleneck BN outputs beta; inference mode does not
                beta = P['down7.beta']
                assert np.abs(a7.reshape(512) - O.act_fwd(beta, 'lrelu')).max() > 0.1
        assert errs[dtype] <= gate, (dtype, errs)
        del m
    print(f"generator eval B={B} S={S}: max-abs error vs fp64 reference {errs}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. batch independence, determinism, no state written
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_is_batch_independent_deterministic_and_stateless():
    P = gen_params()
    m = _gen('f32', P)
    x = torch.from_numpy(O.synthetic_pair(3, 256, 1, seed=9)[0])
    m(x, training=True)                               # a training-mode call: its dropout draw counter must not move below
    ps = m.net.params
    tcall = m._calls[(3, 256)]
    saved = ({k: v.clone() for k, v in ps.state.items()}, ps.step.clone(), tcall.mask_draws.clone())
    y = m(x, training=False)
    y2 = m(x, training=False)
    assert torch.equal(y, y2)                         # bit-identical
    for k in range(3):
        yk = m(x[k:k + 1], training=False)
        assert float((yk[0] - y[k]).abs().max()) < 2e-5
    torch.cuda.synchronize()
    assert all(torch.equal(saved[0][k], ps.state[k]) for k in ps.state)
    assert torch.equal(saved[1], ps.step) and torch.equal(saved[2], tcall.mask_draws)


# ---------------------------------------------------------------------------------------------------------------------
# 4. consistency with the training path
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_with_batch_statistics_as_moving_statistics_equals_training_forward():
    from gan_amd.nets import BN_EPS
    P = gen_params()
    m = _gen('f32', P)
    x = torch.from_numpy(O.synthetic_pair(2, 256, 1, seed=21)[0]).cuda()
    call = m.net.new_call(2, 256, dropout=False)
    call.set_input(x)
    call.forward()
    ref = call.output_f32()
    torch.cuda.synchronize()
    ps = m.net.params
    for name in G_BN:                                 # batch mean / biased variance of the training forward -> moving statistics
        mean, rstd = call.stats[name]
        var = 1.0 / rstd.double() ** 2 - BN_EPS
        ps.state[name + '.moving_mean'].copy_(mean)
        ps.state[name + '.moving_variance'].copy_(var.float())
    out = m(x, training=False)
    assert float((out - ref).abs().max()) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 5. discriminator
# ---------------------------------------------------------------------------------------------------------------------
def test_discriminator_eval_parity_batchnorm():
    from gan_amd.base_gan import DiscriminatorModel
    from gan_amd.nets import Ctx, DiscriminatorNet
    P = disc_params()
    inp, tar = O.synthetic_pair(2, 256, 1, seed=31)
    ref = discriminator_eval_ref(P, inp, tar)
    for dtype, gate in (('f32', 1e-4), ('bf16', 5e-2)):
        net = DiscriminatorNet(Ctx('cuda:0', dtype), 1, True, 'batchnorm', seed=2)
        net.params.load_numpy(P)
        d = DiscriminatorModel(net)
        out = d([torch.from_numpy(inp), torch.from_numpy(tar)], training=False).cpu().numpy()
        err = float(np.abs(out - ref).max()) / max(1.0, float(np.abs(ref).max()))
        assert out.shape == ref.shape and err <= gate, (dtype, err)
        out1 = d([torch.from_numpy(inp[1:]), torch.from_numpy(tar[1:])], training=False).cpu().numpy()
        assert np.abs(out1[0] - out[1]).max() <= (1e-5 if dtype == 'f32' else 1e-2) * max(1.0, float(np.abs(ref).max()))


# ---------------------------------------------------------------------------------------------------------------------
# 6. CycleGAN (InstanceNorm): only the dropout differs
# ---------------------------------------------------------------------------------------------------------------------
def test_instancenorm_generator_eval():
    P = O.init_generator(1, 'instancenorm', seed=13)
    x = O.synthetic_pair(1, 256, 1, seed=14)[0]
    ref, _ = O.generator_fwd(_f64(P), x.astype(np.float64), 'instancenorm', dropmasks=None)
    m = _gen('f32', P, norm='instancenorm')
    y = m(torch.from_numpy(x), training=False)
    y2 = m(torch.from_numpy(x), training=False)
    assert torch.equal(y, y2)
    assert float(np.abs(y.cpu().numpy() - ref).max()) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 7. after training steps and after a checkpoint restore: the fold reads the current weights
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_after_train_steps_and_checkpoint_restore(tmp_path):
    from gan_amd.checkpoint import Checkpoint, CheckpointManager, latest_checkpoint
    from gan_amd.pix2pix import Pix2Pix
    cfg = dict(img_size=256, channels='1', learning_rate=2e-4, beta_1=0.5, beta_2=0.999, seed=3, generator_loss='l1',
               input_img_orient='left', batch_size=2, dtype='f32')
    cfg['lambda'] = 100
    p = Pix2Pix(cfg)
    p.generator.net.params.load_numpy(gen_params())
    x = torch.from_numpy(O.synthetic_pair(2, 256, 1, seed=51)[0])
    y = torch.from_numpy(O.synthetic_pair(2, 256, 1, seed=52)[1])
    first = p.generator(x, training=False).cpu().numpy()          # folds the initial weights
    P0 = p.generator.net.params.to_numpy()
    for _ in range(2):
        p.train_step(x, y, True)
    P1 = p.generator.net.params.to_numpy()
    assert not np.array_equal(P0['down3.kernel'], P1['down3.kernel'])
    assert not np.array_equal(P0['down3.moving_mean'], P1['down3.moving_mean'])
    ref, _ = generator_eval_ref(P1, x.numpy())
    out = p.generator(x, training=False).cpu().numpy()
    assert np.abs(out - ref).max() < 1e-4 and np.abs(out - first).max() > 1e-3
    objs = lambda q: dict(generator=q.generator, discriminator=q.discriminator, generator_optimizer=q.generator_optimizer,
                          discriminator_optimizer=q.discriminator_optimizer)
    CheckpointManager(Checkpoint(**objs(p)), str(tmp_path / 'ck'), max_to_keep=1).save()
    q = Pix2Pix(dict(cfg, seed=77))
    q.generator(x, training=False)                                # a fold of the fresh weights before the restore
    Checkpoint(**objs(q)).restore(latest_checkpoint(str(tmp_path / 'ck')))
    outq = q.generator(x, training=False).cpu().numpy()
    assert np.abs(outq - ref).max() < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 8. an eval forward is the fold plus convolutions: no normalisation launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,B', [('bf16', 1), ('bf16', 16), ('f32', 2)])
def test_eval_forward_launches_fold_and_convolutions_only(dtype, B):
    from gan_amd import _lib as L
    m = _gen(dtype, gen_params())
    x = torch.zeros(B, 256, 256, 1)
    m(x, training=False)                                          # builds the call (plans, tables)
    call = m._eval_calls[(B, 256)]
    torch.cuda.synchronize()
    L.set_option('diag.launch_log', 1)
    try:
        call.infer(fold=True)
        torch.cuda.synchronize()
        log = L.launch_log()
    finally:
        L.set_option('diag.launch_log', 0)
    assert 'bn_fold_multi_kernel' in log[0] and sum('bn_fold' in s for s in log) == 1
    bad = [s for s in log[1:] if any(k in s for k in ('norm', 'stats', 'reduce_partial', 'dropout')) or 'conv' not in s and 'splitk_reduce' not in s]
    assert not bad, bad
    assert len(call.fwd_ops) == 16
    print(f"eval forward {dtype} B={B}: {len(log)} launches")


# ---------------------------------------------------------------------------------------------------------------------
# 9. CLI: --predict --predict-training false
# ---------------------------------------------------------------------------------------------------------------------
def _pngs(d):
    from PIL import Image
    return {f: np.asarray(Image.open(os.path.join(d, f))) for f in sorted(os.listdir(d))}


def _predict_dir(out):
    return os.path.join(out, sorted(os.listdir(out))[0], 'prediction_images')


def test_pix2pix_cli_predict_in_inference_mode(tmp_path):
    from PIL import Image
    from gan_amd import pix2pix
    from gan_amd.checkpoint import Checkpoint, latest_checkpoint
    from gan_amd.runner import save_panels
    rng = np.random.default_rng(0)
    data = str(tmp_path / 'data')
    os.makedirs(data)
    for i in range(7):
        Image.fromarray(rng.integers(0, 256, (64, 128), dtype=np.uint8), 'L').save(os.path.join(data, f"p{i}.png"))
    out = str(tmp_path / 'out')
    pix2pix.main(pix2pix.parse_opt(['--data', data, '--output', out, '--train', '--epochs', '1', '--batch-size', '2', '--test-img', '1',
                                    '--validation-size', '0.2', '--logging', 'false', '--dtype', 'f32']))
    ck = os.path.join(out, sorted(os.listdir(out))[0], 'training_checkpoints')
    args = ['--data', data, '--predict', '--weights', ck, '--logging', 'false', '--predict-training', 'false', '--batch-size', '3',
            '--dtype', 'f32']
    pix2pix.main(pix2pix.parse_opt(args + ['--output', str(tmp_path / 'p1')]))
    pix2pix.main(pix2pix.parse_opt(args + ['--output', str(tmp_path / 'p2')]))
    a, b = _pngs(_predict_dir(str(tmp_path / 'p1'))), _pngs(_predict_dir(str(tmp_path / 'p2')))
    assert sorted(a) == [f"img{k}.png" for k in range(7)] and sorted(a) == sorted(b)
    assert all(np.array_equal(a[f], b[f]) for f in a)             # deterministic: identical on a rerun
    # the first prediction = generator(x, training=False) of that input at batch 1, rendered the same way
    p = pix2pix.Pix2Pix(vars(pix2pix.parse_opt(args + ['--output', str(tmp_path / 'p3')])))
    Checkpoint(generator=p.generator, discriminator=p.discriminator, generator_optimizer=p.generator_optimizer,
               discriminator_optimizer=p.discriminator_optimizer).restore(latest_checkpoint(ck))
    ds = p.image_pipeline(predict=True)[0]
    inp, tar = next(iter(ds.unbatch()))
    pred = p.generator(inp[None], training=False).cpu().numpy()[0]
    save_panels(str(tmp_path / 'one.png'), [('Input Image', inp), ('Ground Truth', tar), ('Predicted Image', pred)], gray=True)
    one = np.asarray(Image.open(str(tmp_path / 'one.png'))).astype(np.int16)
    diff = np.abs(one - a['img0.png'].astype(np.int16))
    assert one.shape == a['img0.png'].shape and diff.max() <= 2 and (diff > 0).mean() < 1e-3


def test_cyclegan_cli_predict_in_inference_mode(tmp_path):
    from PIL import Image
    from gan_amd import cycle_gan
    from gan_amd.runner import save_panels
    rng = np.random.default_rng(1)
    dx, dy = str(tmp_path / 'X'), str(tmp_path / 'Y')
    for d in (dx, dy):
        os.makedirs(d)
        for i in range(7):
            Image.fromarray(rng.integers(0, 256, (80, 96), dtype=np.uint8), 'L').save(os.path.join(d, f"s{i}.png"))
    out = str(tmp_path / 'out')
    cycle_gan.main(cycle_gan.parse_opt(['--input-images', dx, '--target-images', dy, '--output', out, '--train', '--epochs', '1',
                                        '--test-img', '1', '--validation-size', '0.2', '--logging', 'false', '--dtype', 'f32']))
    ck = os.path.join(out, sorted(os.listdir(out))[0], 'training_checkpoints')
    args = ['--input-images', dx, '--predict', '--weights', ck, '--logging', 'false', '--predict-training', 'false', '--batch-size', '3',
            '--dtype', 'f32']
    cycle_gan.main(cycle_gan.parse_opt(args + ['--output', str(tmp_path / 'p1')]))
    cycle_gan.main(cycle_gan.parse_opt(args + ['--output', str(tmp_path / 'p2')]))
    a, b = _pngs(_predict_dir(str(tmp_path / 'p1'))), _pngs(_predict_dir(str(tmp_path / 'p2')))
    assert sorted(a) == [f"img{k}.png" for k in range(7)] and all(np.array_equal(a[f], b[f]) for f in a)
    from gan_amd.checkpoint import Checkpoint, latest_checkpoint
    c = cycle_gan.CycleGAN(vars(cycle_gan.parse_opt(args + ['--output', str(tmp_path / 'p3')])))
    names = ('generator_g', 'generator_f', 'discriminator_x', 'discriminator_y')
    objects = {n: getattr(c, n) for n in names}
    objects.update({n + '_optimizer': getattr(c, n + '_optimizer') for n in names})
    Checkpoint(**objects).restore(latest_checkpoint(ck))
    (img,) = next(iter(c.image_pipeline(predict=True)[0].unbatch()))
    pred = c.generator_g(img[None], training=False).cpu().numpy()[0]
    save_panels(str(tmp_path / 'one.png'), [('Input Image', img), ('Predicted Image', pred)], gray=True)
    one = np.asarray(Image.open(str(tmp_path / 'one.png'))).astype(np.int16)
    diff = np.abs(one - a['img0.png'].astype(np.int16))
    assert one.shape == a['img0.png'].shape and diff.max() <= 2 and (diff > 0).mean() < 1e-3
