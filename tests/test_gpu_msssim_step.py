"""The Pix2Pix step with generator_loss='msssim' and 'msssim_l1' (DESIGN.md section 24): 256^2, one channel, batch 2 (the smallest
the U-Net admits).  The secondary term of the step is the stand-alone gan_msssim (behind gan_l1 for the mix) on the step's own
operands - value against the fp64 reference within the kernel test's loss gate, gradient bit for bit - the captured step replays the
eager one, the other losses enqueue what they did, and the edge term follows the MS-SSIM call."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gan_oracle as O
from tests import msssim_ref as R

pytestmark = pytest.mark.gpu

B, S, CH, LAM, ALPHA, M = 2, 256, 1, 100.0, 0.84, 5
LOSS_GATE = 2.5e-5          # tests/test_gpu_msssim.py: 2.5 x the SSIM gate of an image that is not flat


def _pair(ctx, seed):
    a, b = O.synthetic_pair(B, S, CH, seed=seed)
    return torch.from_numpy(a).to(ctx.device), torch.from_numpy(b).to(ctx.device)


def _standalone(ctx, st, kind):
    """The stand-alone call(s) on the step's own operands -> (losses[2], da)."""
    from gan_amd import _lib as L
    g, d = st.g, st.d
    da = torch.full((B, S, S, CH), float('nan'), device=ctx.device)
    out = torch.zeros(1, device=ctx.device)
    tda = L.GanTensor(da.data_ptr(), B, S, S, CH, CH)
    a, b = g.out_view(), d.xin.view(CH, CH, 0, B)
    al = ALPHA if kind == 'msssim_l1' else 1.0
    if kind == 'msssim_l1':
        ws = torch.zeros(4096, device=ctx.device)
        L.check(ctx.lib.gan_l1(L.F32, C.byref(a), C.byref(b), 1.0 * (1.0 - al), 0, out.data_ptr(), LAM * (1.0 - al), C.byref(tda), ws.data_ptr(),
                               None, ctx.stream()), "l1")
    ws2 = torch.full((ctx.lib.gan_msssim_workspace_bytes(B, S, S, CH, M) // 4,), float('nan'), device=ctx.device)
    acc = int(kind == 'msssim_l1')
    desc = L.GanMsssimDesc(L.F32, L.F32, a, b, 1.0 * al, acc, out.data_ptr(), LAM * al, L.F32, tda, ws2.data_ptr(), ws2.numel() * 4, None, M,
                           L.msssim_power(M), None, acc)
    L.check(ctx.lib.gan_msssim(C.byref(desc), ctx.stream()), "msssim")
    torch.cuda.synchronize()
    return out, da


@pytest.mark.parametrize('kind', ['msssim', 'msssim_l1'])
def test_fp32_eager_step_takes_its_secondary_term_from_gan_msssim(kind):
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    ctx = Ctx('cuda:0', 'f32')
    st = Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=123, generator_loss=kind, msssim_alpha=ALPHA)
    x, y = _pair(ctx, 123)
    losses = st._run(x, y, True).clone()
    torch.cuda.synchronize()
    gen = st.g.output_f32().double().cpu().numpy()
    tar = y.double().cpu().numpy()
    ms = R.loss(gen, tar, M)
    want = ms if kind == 'msssim' else (1.0 - ALPHA) * float(np.abs(tar - gen).mean()) + ALPHA * ms
    l = losses.double().cpu().numpy()
    print(f"{kind} step f32: losses {l[:4].tolist()} reference 1 - MS-SSIM {ms:.9f} secondary {want:.9f} err {abs(l[2] - want):.3e} "
          f"smallest factor {R.min_factor(gen, tar, M):.3f}")
    assert np.isfinite(l[:4]).all() and 0.0 < l[2] < 2.0
    assert abs(l[2] - want) <= LOSS_GATE
    # gen_total = gan_loss + lambda * losses[2] in fp32: one product and one sum, each rounded (or one fused rounding)
    assert abs(l[0] - (l[1] + LAM * l[2])) <= 2.0 ** -22 * (abs(l[1]) + LAM * abs(l[2]))
    # the gradient the backward pass started from = the stand-alone call(s) on the step's own operands, grad_scale = lambda
    out, da = _standalone(ctx, st, kind)
    assert torch.equal(st.g.dgen.t[..., :CH].contiguous().view(torch.int32), da.view(torch.int32))
    assert torch.equal(out[0], losses[2])
    # the default step is untouched by the option
    assert Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=123, nets=st.nets()).generator_loss == 'l1'
    with pytest.raises(ValueError):
        Pix2PixStep(ctx, B, 128, CH, lam=LAM, seed=123, generator_loss=kind)           # 128 < 11 * 16: refused in __init__


def _reset(st, w0):
    for n_, w_ in zip(st.nets(), w0):
        n_.params.master.copy_(w_)
        n_.params.prepare()
        n_.params.m.zero_(); n_.params.v.zero_(); n_.params.step.zero_()
    for call in vars(st).values():
        if hasattr(call, 'mask_draws'):
            call.mask_draws.zero_()


@pytest.mark.parametrize('kind', ['msssim', 'msssim_l1'])
def test_bf16_captured_step_replays_the_eager_one(kind):
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    ctx = Ctx('cuda:0', 'bf16')
    st = Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=7, generator_loss=kind)
    w0 = [n.params.master.clone() for n in st.nets()]
    x, y = _pair(ctx, 43)
    eager = st.train_step(x, y, True).clone()
    replay = st.capture(training=True)           # (capture runs warm-up steps: back to the initial state)
    _reset(st, w0)
    first = replay(x, y)[:4].clone()
    torch.cuda.synchronize()
    print(f"{kind} step bf16: eager {eager.tolist()} replayed {first.tolist()}")
    assert torch.isfinite(first).all() and torch.equal(first, eager)


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


@pytest.mark.parametrize('kind', ['l1', 'dssim'])
def test_the_other_losses_enqueue_what_they_did(kind):
    """'l1' and 'dssim' do not see the new argument: launch for launch and bit for bit the step built without it; and 'msssim' is
    that step with the secondary call swapped - 2 M + 1 launches in place of gan_l1's."""
    ctx, a = _fresh('bf16', 7, **({} if kind == 'l1' else dict(generator_loss=kind)))            # built without the arguments
    _, b = _fresh('bf16', 7, generator_loss=kind, msssim_alpha=0.5)
    x, y = _pair(ctx, 43)
    la, lb = [], []
    loga = _logged(lambda: la.extend(a.train_step(x, y, True).clone() for _ in range(2)))
    logb = _logged(lambda: lb.extend(b.train_step(x, y, True).clone() for _ in range(2)))
    torch.cuda.synchronize()
    assert len(loga) > 200 and loga == logb
    assert not any('msssim' in k for k in loga) and not hasattr(b, 'msssim_ws')
    assert all(torch.equal(p, q) for p, q in zip(la, lb))
    if kind == 'l1':
        _, c = _fresh('bf16', 7, generator_loss='msssim')
        logc = _logged(lambda: c.train_step(x, y, True))
        logd = _logged(lambda: a.train_step(x, y, True))
        torch.cuda.synchronize()
        ms = [k for k in logc if 'msssim' in k]
        assert len(ms) == 2 * M + 1 and sum('pool' in k for k in ms) == M - 1 and sum('finalize' in k for k in ms) == 1
        l1 = [k for k in logd if 'l1_kernel' in k or 'l1_finalize' in k]
        assert len(l1) == 2 and [k for k in logc if 'msssim' not in k] == [k for k in logd if k not in l1]       # gan_l1's two launches are gone


def test_the_edge_launches_follow_the_msssim_call():
    ctx, st = _fresh('bf16', 7, generator_loss='msssim_l1', edge_weight=0.25)
    x, y = _pair(ctx, 43)
    log = _logged(lambda: st.train_step(x, y, True))
    torch.cuda.synchronize()
    ms = [i for i, k in enumerate(log) if 'msssim' in k]
    edge = [i for i, k in enumerate(log) if 'edge' in k]
    assert len(ms) == 2 * M + 1 and ms == list(range(ms[0], ms[0] + len(ms))) and edge == [ms[-1] + 1, ms[-1] + 2]
    assert 'l1_kernel' in log[ms[0] - 2] and 'l1_finalize' in log[ms[0] - 1]            # gan_l1 directly in front of it


def test_train_state_carries_the_loss_and_its_weight():
    from gan_amd import pix2pix
    from gan_amd import train_state as T
    from gan_amd.runner import config_of
    opt = pix2pix.parse_opt(['--data', 'd', '--output', 'o', '--train', '--epochs', '1', '--generator-loss', 'msssim-l1', '--msssim-alpha', '0.5'])
    stored = T._from_json_array(T._json_array(T.run_config(config_of(opt))))
    assert stored['generator_loss'] == 'msssim-l1' and stored['msssim_alpha'] == 0.5
