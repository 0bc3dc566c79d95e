"""The Pix2Pix step with a DiffAugment object: 256^2, one channel, batch 2 (the smallest the U-Net admits).
What D sees is the reference transform of the staged raw images with the table the step drew, the generator's adversarial gradient
is the reference transpose of D's input gradient, the secondary loss is the one of the un-augmented target; without the object (and
in validation passes with it) the step is the parent's, launch for launch and bit for bit; the captured step replays the eager one
and draws anew on every replay; the CLI trains with the flag."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import gan_oracle as O
from tests import diffaug_ref as R

pytestmark = pytest.mark.gpu

B, S, CH, LAM = 2, 256, 1, 100.0
ALL = 'translation,cutout,brightness,saturation'


def _pair(ctx, seed):
    a, b = O.synthetic_pair(B, S, CH, seed=seed)
    return torch.from_numpy(a).to(ctx.device), torch.from_numpy(b).to(ctx.device)


def test_fp32_eager_step_augments_what_the_discriminator_sees():
    from gan_amd.diffaug import DiffAugment
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    ctx = Ctx('cuda:0', 'f32')
    aug = DiffAugment(ctx, ALL, seed=123)
    st = Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=123, diffaug=aug)
    plain = Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=123, nets=st.nets())
    x, y = _pair(ctx, 123)
    w0 = [n.params.master.clone() for n in st.nets()]
    losses = st._run(x, y, True).clone()
    torch.cuda.synchronize()
    g, d = st.g, st.d
    assert int(aug.launches.item()) == 1
    assert all(int(n.params.step.item()) == 1 and not torch.equal(n.params.master, w) for n, w in zip(st.nets(), w0))     # both networks moved
    recs = aug.records(2 * B)
    assert recs == R.draw(aug.seed, 0, aug.stream_id, 2 * B, S, S, R.POLICIES)          # the table the step drew: launch 0
    assert any(p['tx'] or p['ty'] for p in recs) and all(p['cut_w'] > 0 for p in recs)
    # D's input = the reference transform of the staged raw images: [input | target] of the real samples (two one-channel images per
    # sample, one record), and [input | generated] of the generated ones with records B ..
    raw = st.aug_raw.t.double().cpu()
    gen = g.output_f32().double().cpu()
    assert torch.equal(raw[:B, ..., 0:1], x.double().cpu()) and torch.equal(raw[:B, ..., 1:2], y.double().cpu())
    fake_raw = torch.cat([raw[B:, ..., 0:1], gen], dim=3)
    want = torch.cat([R.forward(raw[:B, ..., :2], recs, 1, 0), R.forward(fake_raw, recs, 1, B)]).numpy()
    got = d.xin.t[..., :2].double().cpu().numpy()
    # one-channel images: x + brightness, one fp32 add rounded once: half an ulp of the result; 4 ulps of the largest term is the
    # gate of tests/test_gpu_diffaug.py
    term = np.concatenate([R.forward_terms(raw[:B, ..., :2].numpy(), recs, 1, 0), R.forward_terms(fake_raw.numpy(), recs, 1, B)])
    err = np.abs(got - want)
    print(f"diffaug step f32: D input against the reference: worst {float((err / (4 * R.ulp(term, 'f32'))).max()):.3f} of the gate")
    assert (err <= 4 * R.ulp(term, 'f32')).all()
    assert (d.xin.t[..., 2:] == 0).all()                                                # the pad channels stay what they were
    # the generator's adversarial gradient = the reference transpose of D's input gradient (one-channel images: bits move)
    tmp = st.aug_dgen.t[..., :CH].double().cpu().numpy()
    assert np.abs(tmp).max() > 0
    want = R.transpose(tmp, recs, 1, B)
    assert (g.dgen2.t[..., :CH].double().cpu().numpy() == want).all()
    # the secondary loss is the L1 term of the un-augmented target
    l1 = float((y.double().cpu() - gen).abs().mean())
    print(f"diffaug step f32: losses {losses[:4].tolist()} reference l1 {l1:.9f}")
    assert abs(float(losses[2]) - l1) <= 1e-5 * l1
    # the same weights, the same inputs, no augmentation: the same generator output and secondary loss, another discriminator loss
    for n_, w_ in zip(st.nets(), w0):
        n_.params.master.copy_(w_)
        n_.params.prepare()
        n_.params.m.zero_(); n_.params.v.zero_(); n_.params.step.zero_()
    st.g.mask_draws.zero_()
    base = plain._run(x, y, True).clone()
    torch.cuda.synchronize()
    assert torch.equal(base[2], losses[2]) and not torch.equal(base[3], losses[3])


def _logged(fn):
    from gan_amd import _lib as L
    L.set_option('diag.launch_log', 1)
    try:
        fn()
        return L.launch_log()
    finally:
        L.set_option('diag.launch_log', 0)


def _fresh(dtype, seed, **kw):
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    ctx = Ctx('cuda:0', dtype)
    return ctx, Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=seed, **kw)


def test_default_path_and_validation_are_the_step_without_the_argument():
    from gan_amd.diffaug import DiffAugment
    ctx, a = _fresh('bf16', 7)                                   # built without the argument
    _, b = _fresh('bf16', 7, diffaug=None)
    x, y = _pair(ctx, 43)
    la, lb = [], []
    loga = _logged(lambda: la.extend(a.train_step(x, y, True).clone() for _ in range(3)))
    logb = _logged(lambda: lb.extend(b.train_step(x, y, True).clone() for _ in range(3)))
    torch.cuda.synchronize()
    assert len(loga) > 300 and loga == logb
    assert not any('diffaug' in k for k in loga)
    assert all(torch.equal(p, q) for p, q in zip(la, lb))
    # training=False with the object given: the launches and the losses of the default step, bit for bit
    _, c = _fresh('bf16', 7, diffaug=DiffAugment(ctx, ALL, seed=7))
    _, e = _fresh('bf16', 7)
    lc, le = [], []
    logc = _logged(lambda: lc.append(c.train_step(x, y, False).clone()))
    loge = _logged(lambda: le.append(e.train_step(x, y, False).clone()))
    torch.cuda.synchronize()
    assert logc == loge and torch.equal(lc[0], le[0]) and torch.isfinite(lc[0]).all()
    assert int(c.diffaug.launches.item()) == 0
    # ... and a training step with it adds exactly the draw and the four apply launches in place of the copy
    logt = _logged(lambda: c.train_step(x, y, True))
    torch.cuda.synchronize()
    assert sum('diffaug_draw' in k for k in logt) == 1 and sum('diffaug_apply' in k for k in logt) == 4
    logd = _logged(lambda: e.train_step(x, y, True))              # the default object's training step, at the same point of its life
    torch.cuda.synchronize()
    rest = [k for k in logt if 'diffaug' not in k]
    copies = [i for i, k in enumerate(logd) if 'copy_view' in k]
    print(f"diffaug step bf16: {len(logd)} launches per default training step, {len(logt)} with the augmentation")
    assert len(logt) == len(logd) + 4 and any(rest == logd[:i] + logd[i + 1:] for i in copies)


def test_bf16_captured_step_replays_the_eager_one_and_draws_anew():
    from gan_amd.diffaug import DiffAugment
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    ctx = Ctx('cuda:0', 'bf16')
    aug = DiffAugment(ctx, ALL, seed=7)
    st = Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=7, diffaug=aug)
    w0 = [n.params.master.clone() for n in st.nets()]
    x, y = _pair(ctx, 43)
    eager = st.train_step(x, y, True).clone()
    xin_eager = st.d.xin.t.clone()
    replay = st.capture(training=True)           # (capture runs warm-up steps: back to the initial state)
    for n_, w_ in zip(st.nets(), w0):
        n_.params.master.copy_(w_)
        n_.params.prepare()
        n_.params.m.zero_(); n_.params.v.zero_(); n_.params.step.zero_()
    st.g.mask_draws.zero_()
    for t in aug.tensors():
        t.zero_()
    first = replay(x, y)[:4].clone()
    torch.cuda.synchronize()
    print(f"diffaug step bf16: eager {eager.tolist()} replayed {first.tolist()}")
    assert torch.isfinite(first).all() and torch.equal(first, eager)
    assert torch.equal(st.d.xin.t.view(torch.int16), xin_eager.view(torch.int16)) and int(aug.launches.item()) == 1
    seen = [st.d.xin.t[:B].clone()]              # the real half: the same raw images in every replay, another table
    tot = []
    for k in range(19):
        tot.append(replay(x, y)[:4].clone())
        if k == 0:
            seen.append(st.d.xin.t[:B].clone())
    torch.cuda.synchronize()
    assert int(aug.launches.item()) == 20
    assert not torch.equal(seen[0], seen[1])
    assert aug.records(2 * B) == R.draw(aug.seed, 19, aug.stream_id, 2 * B, S, S, R.POLICIES)
    tot = torch.stack(tot)
    print(f"diffaug step bf16: losses of replay 20 {tot[-1].tolist()}")
    assert torch.isfinite(tot).all()


def test_cli_trains_with_diffaugment(tmp_path):
    from PIL import Image
    from gan_amd import pix2pix
    rng = np.random.default_rng(0)
    data, out = str(tmp_path / 'data'), str(tmp_path / 'out')
    os.makedirs(data)
    for i in range(10):
        Image.fromarray(rng.integers(0, 256, (256, 512), dtype=np.uint8), 'L').save(os.path.join(data, f"p{i}.png"))
    pix2pix.main(pix2pix.parse_opt(['--data', data, '--output', out, '--train', '--epochs', '1', '--batch-size', '2', '--logging', 'false',
                                    '--seed', '7', '--diffaugment', 'cutout,translation', '--save-weights', 'false']))
    logs = os.path.join(out, sorted(os.listdir(out))[0], 'logs')
    strict = lambda p: json.loads(open(p).read(), parse_constant=lambda s: pytest.fail(f"not strict JSON: {s} in {p}"))
    assert strict(os.path.join(logs, 'config.json'))['diffaugment'] == 'translation,cutout'
    for name in ('train_metrics.json', 'val_metrics.json'):
        for key, vals in strict(os.path.join(logs, name)).items():
            assert len(vals) == 1 and all(np.isfinite(v) for v in vals), (name, key, vals)
