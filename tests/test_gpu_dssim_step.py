"""The Pix2Pix step with generator_loss='dssim' (DESIGN.md section 14): 256^2, one channel, batch 2 (the smallest the U-Net admits).
The secondary term of the step is the stand-alone gan_dssim on the step's own operands - value against the fp64 reference, gradient
bit for bit - the captured step replays the eager one and descends, and the CLI trains with the flag."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import gan_oracle as O
from tests import dssim_ref as R

pytestmark = pytest.mark.gpu

B, S, CH, LAM = 2, 256, 1, 100.0


def _pair(ctx, seed):
    a, b = O.synthetic_pair(B, S, CH, seed=seed)
    return torch.from_numpy(a).to(ctx.device), torch.from_numpy(b).to(ctx.device)


def test_fp32_eager_step_takes_its_secondary_term_from_gan_dssim():
    from gan_amd import _lib as L
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    ctx = Ctx('cuda:0', 'f32')
    st = Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=123, generator_loss='dssim')
    x, y = _pair(ctx, 123)
    losses = st._run(x, y, True).clone()
    torch.cuda.synchronize()
    g, d = st.g, st.d
    gen = g.output_f32()
    want = R.loss(gen.double().cpu().numpy(), y.double().cpu().numpy())
    l = losses.double().cpu().numpy()
    print(f"dssim step f32: losses {l[:4].tolist()} reference dssim {want:.9f} err {abs(l[2] - want):.3e}")
    assert np.isfinite(l[:4]).all() and 0.0 < l[2] < 2.0
    assert abs(l[2] - want) <= 1e-5
    # gen_total = gan_loss + lambda * dssim in fp32: one product and one sum, each rounded (or one fused rounding)
    assert abs(l[0] - (l[1] + LAM * l[2])) <= 2.0 ** -22 * (abs(l[1]) + LAM * abs(l[2]))
    # the gradient the backward pass started from = the stand-alone op on the step's own operands, grad_scale = lambda
    da = torch.full((B, S, S, CH), float('nan'), device=ctx.device)
    out = torch.zeros(1, device=ctx.device)
    ws = torch.zeros(ctx.lib.gan_dssim_workspace_bytes(B, S, S, CH) // 4, device=ctx.device)
    desc = L.GanDssimDesc(L.F32, L.F32, g.out_view(), d.xin.view(CH, CH, 0, B), 1.0, 0, out.data_ptr(), LAM, L.F32,
                          L.GanTensor(da.data_ptr(), B, S, S, CH, CH), ws.data_ptr(), ws.numel() * 4, None)
    L.check(ctx.lib.gan_dssim(C.byref(desc), ctx.stream()), "dssim")
    torch.cuda.synchronize()
    assert torch.equal(g.dgen.t[..., :CH].contiguous().view(torch.int32), da.view(torch.int32))
    assert torch.equal(out[0], losses[2])
    _, ref_grad = R.loss_and_grad(gen.double().cpu().numpy(), y.double().cpu().numpy())
    e = float((da.double().cpu() - LAM * ref_grad).abs().max() / (LAM * ref_grad).abs().max())
    print(f"dssim step f32: gradient against the fp64 reference {e:.3e}")
    assert e <= 1e-3
    # the default step is untouched by the option
    assert Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=123, nets=st.nets()).generator_loss == 'l1'


def _reset(st, w0):
    for n_, w_ in zip(st.nets(), w0):
        n_.params.master.copy_(w_)
        n_.params.prepare()
        n_.params.m.zero_(); n_.params.v.zero_(); n_.params.step.zero_()
    for call in vars(st).values():
        if hasattr(call, 'mask_draws'):
            call.mask_draws.zero_()


def test_bf16_captured_step_replays_the_eager_one_and_descends():
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    ctx = Ctx('cuda:0', 'bf16')
    st = Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=7, generator_loss='dssim')
    w0 = [n.params.master.clone() for n in st.nets()]
    x, y = _pair(ctx, 43)
    eager = st.train_step(x, y, True).clone()
    replay = st.capture(training=True)           # (capture runs warm-up steps: back to the initial state)
    _reset(st, w0)
    first = replay(x, y)[:4].clone()
    torch.cuda.synchronize()
    print(f"dssim step bf16: eager {eager.tolist()} replayed {first.tolist()}")
    assert torch.isfinite(first).all() and torch.equal(first, eager)
    sec = [float(first[2])]
    for _ in range(29):
        sec.append(replay(x, y)[2:3].clone())
    torch.cuda.synchronize()
    sec = [float(v) for v in sec]
    print(f"dssim step bf16: secondary loss over 30 replays: first {sec[0]:.5f} last five {[round(v, 5) for v in sec[-5:]]}")
    assert np.isfinite(sec).all() and np.mean(sec[-5:]) < sec[0]


def test_cli_trains_with_generator_loss_dssim(tmp_path):
    from PIL import Image
    from gan_amd import pix2pix
    rng = np.random.default_rng(0)
    data, out = str(tmp_path / 'data'), str(tmp_path / 'out')
    os.makedirs(data)
    for i in range(10):
        Image.fromarray(rng.integers(0, 256, (256, 512), dtype=np.uint8), 'L').save(os.path.join(data, f"p{i}.png"))
    pix2pix.main(pix2pix.parse_opt(['--data', data, '--output', out, '--train', '--epochs', '1', '--batch-size', '2', '--logging', 'false',
                                    '--seed', '7', '--generator-loss', 'dssim', '--save-weights', 'false']))
    logs = os.path.join(out, sorted(os.listdir(out))[0], 'logs')
    strict = lambda p: json.loads(open(p).read(), parse_constant=lambda s: pytest.fail(f"not strict JSON: {s} in {p}"))
    assert strict(os.path.join(logs, 'config.json'))['generator_loss'] == 'dssim'
    for name in ('train_metrics.json', 'val_metrics.json'):
        m = strict(os.path.join(logs, name))
        assert 'Generator Loss (Secondary)' in m
        for key, vals in m.items():
            assert len(vals) == 1 and all(np.isfinite(v) for v in vals), (name, key, vals)
        assert 0.0 < m['Generator Loss (Secondary)'][0] < 2.0           # 1 - SSIM lies in [0, 2]
