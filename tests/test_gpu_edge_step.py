"""The Pix2Pix step with edge_weight: 256^2, one channel, batch 2 (the smallest the U-Net admits).  The
secondary slot of the step holds the secondary loss plus the weighted Sobel edge term - value against the fp64 references, gradient
bit for bit the stand-alone gan_l1 (or gan_dssim) followed by gan_edge_l1 on the step's own operands - the captured step replays the
eager one and descends, weight 0 is the step without the argument launch for launch, DiffAugment leaves the term on the un-augmented
target, and the CLI trains with the flag."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import gan_oracle as O
from tests import dssim_ref
from tests import edge_ref as R

pytestmark = pytest.mark.gpu

B, S, CH, LAM, W = 2, 256, 1, 100.0, 0.25
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(ctx, seed):
    a, b = O.synthetic_pair(B, S, CH, seed=seed)
    return torch.from_numpy(a).to(ctx.device), torch.from_numpy(b).to(ctx.device)


def _standalone(ctx, st, kind):
    """The stand-alone secondary op, then gan_edge_l1 accumulating, on the step's own operands -> (losses[2], da)."""
    from gan_amd import _lib as L
    g, d = st.g, st.d
    da = torch.full((B, S, S, CH), float('nan'), device=ctx.device)
    out = torch.zeros(1, device=ctx.device)
    tda = L.GanTensor(da.data_ptr(), B, S, S, CH, CH)
    a, b = g.out_view(), d.xin.view(CH, CH, 0, B)
    if kind == 'dssim':
        ws = torch.zeros(ctx.lib.gan_dssim_workspace_bytes(B, S, S, CH) // 4, device=ctx.device)
        desc = L.GanDssimDesc(L.F32, L.F32, a, b, 1.0, 0, out.data_ptr(), LAM, L.F32, tda, ws.data_ptr(), ws.numel() * 4, None)
        L.check(ctx.lib.gan_dssim(C.byref(desc), ctx.stream()), "dssim")
    else:
        ws = torch.zeros(4096, device=ctx.device)
        L.check(ctx.lib.gan_l1(L.F32, C.byref(a), C.byref(b), 1.0, 0, out.data_ptr(), LAM, C.byref(tda), ws.data_ptr(), None, ctx.stream()), "l1")
    ws2 = torch.zeros(ctx.lib.gan_edge_workspace_bytes(B, S, S, CH) // 4, device=ctx.device)
    desc = L.GanEdgeDesc(L.F32, L.F32, a, b, W, 1, out.data_ptr(), LAM * W, L.F32, tda, ws2.data_ptr(), ws2.numel() * 4, None, 1)
    L.check(ctx.lib.gan_edge_l1(C.byref(desc), ctx.stream()), "edge_l1")
    torch.cuda.synchronize()
    return out, da


@pytest.mark.parametrize('kind', ['l1', 'dssim'])
def test_fp32_eager_step_adds_the_edge_term_to_its_secondary_slot(kind):
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    ctx = Ctx('cuda:0', 'f32')
    st = Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=123, generator_loss=kind, edge_weight=W)
    x, y = _pair(ctx, 123)
    losses = st._run(x, y, True).clone()
    torch.cuda.synchronize()
    gen = st.g.output_f32().double().cpu().numpy()
    tar = y.double().cpu().numpy()
    first = dssim_ref.loss(gen, tar) if kind == 'dssim' else float(np.abs(tar - gen).mean())
    edge = R.loss(gen, tar)
    want = first + W * edge
    l = losses.double().cpu().numpy()
    print(f"edge step f32 {kind}: losses {l[:4].tolist()} reference {first:.9f} + {W} * {edge:.9f} = {want:.9f} err {abs(l[2] - want):.3e}")
    assert np.isfinite(l[:4]).all() and edge > 0
    assert abs(l[2] - want) <= 1e-5
    # gen_total = gan_loss + lambda * losses[2] in fp32: one product and one sum, each rounded (or one fused rounding)
    assert abs(l[0] - (l[1] + LAM * l[2])) <= 2.0 ** -22 * (abs(l[1]) + LAM * abs(l[2]))
    # the gradient the backward pass started from = the two stand-alone ops on the step's own operands
    out, da = _standalone(ctx, st, kind)
    assert torch.equal(st.g.dgen.t[..., :CH].contiguous().view(torch.int32), da.view(torch.int32))
    assert torch.equal(out[0], losses[2])
    # the default step is untouched by the option
    assert Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=123, nets=st.nets()).edge_weight == 0.0


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
    st = Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=7, edge_weight=W)
    w0 = [n.params.master.clone() for n in st.nets()]
    x, y = _pair(ctx, 43)
    eager = [st.train_step(x, y, True).clone() for _ in range(3)]
    replay = st.capture(training=True)           # (capture runs warm-up steps: back to the initial state)
    _reset(st, w0)
    again = [replay(x, y)[:4].clone() for _ in range(3)]
    torch.cuda.synchronize()
    print(f"edge step bf16: eager {[e.tolist() for e in eager]} replayed {[e.tolist() for e in again]}")
    for e, r in zip(eager, again):
        assert torch.isfinite(r).all() and torch.equal(r, e)
    sec = [float(again[0][2])]
    for _ in range(27):
        sec.append(replay(x, y)[2:3].clone())
    torch.cuda.synchronize()
    sec = [float(v) for v in sec]
    print(f"edge step bf16: secondary loss over 30 replays: first {sec[0]:.5f} last five {[round(v, 5) for v in sec[-5:]]}")
    assert np.isfinite(sec).all() and np.mean(sec[-5:]) < sec[0]


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


def test_weight_zero_is_the_step_without_the_argument():
    ctx, a = _fresh('bf16', 7)                                   # built without the argument
    _, b = _fresh('bf16', 7, edge_weight=0.0)
    x, y = _pair(ctx, 43)
    la, lb = [], []
    loga = _logged(lambda: la.extend(a.train_step(x, y, True).clone() for _ in range(3)))
    logb = _logged(lambda: lb.extend(b.train_step(x, y, True).clone() for _ in range(3)))
    torch.cuda.synchronize()
    assert len(loga) > 300 and loga == logb
    assert not any('edge' in k for k in loga) and not hasattr(b, 'edge_ws')
    assert all(torch.equal(p, q) for p, q in zip(la, lb))
    # ... and with a weight the step adds exactly the two launches of gan_edge_l1, training and validation alike
    _, c = _fresh('bf16', 7, edge_weight=W)
    _, e = _fresh('bf16', 7)
    for training in (True, False):
        logt = _logged(lambda: c.train_step(x, y, training))
        logd = _logged(lambda: e.train_step(x, y, training))
        torch.cuda.synchronize()
        assert sum('edge_tile' in k for k in logt) == 1 and sum('edge_finalize' in k for k in logt) == 1
        assert [k for k in logt if 'edge' not in k] == logd
        print(f"edge step bf16 training={training}: {len(logd)} launches per default step, {len(logt)} with the edge term")


def test_diffaugment_leaves_the_edge_term_on_the_unaugmented_target():
    from gan_amd.diffaug import DiffAugment
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    ctx = Ctx('cuda:0', 'f32')
    aug = DiffAugment(ctx, 'translation,cutout,brightness,saturation', seed=123)
    st = Pix2PixStep(ctx, B, S, CH, lam=LAM, seed=123, diffaug=aug, edge_weight=W)
    x, y = _pair(ctx, 123)
    losses = st._run(x, y, True).clone()
    torch.cuda.synchronize()
    assert int(aug.launches.item()) == 1 and any(p['tx'] or p['ty'] for p in aug.records(2 * B))
    gen = st.g.output_f32().double().cpu().numpy()
    tar = y.double().cpu().numpy()
    l1, edge = float(np.abs(tar - gen).mean()), R.loss(gen, tar)
    seen = st.d.xin.t[:B, ..., CH:2 * CH].double().cpu().numpy()          # the target as D saw it: augmented
    assert not np.array_equal(seen, tar)
    print(f"edge step f32 diffaug: losses[2] {float(losses[2]):.9f} reference {l1:.9f} + {W} * {edge:.9f}; on the augmented target "
          f"the edge term would be {R.loss(gen, seen):.9f}")
    assert abs(float(losses[2]) - (l1 + W * edge)) <= 1e-5
    assert abs(R.loss(gen, seen) - edge) > 1e-4                            # (the check above tells the two targets apart)


def test_cli_trains_with_edge_weight(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    data, out = str(tmp_path / 'data'), str(tmp_path / 'out')
    os.makedirs(data)
    for i in range(10):
        Image.fromarray(rng.integers(0, 256, (256, 512), dtype=np.uint8), 'L').save(os.path.join(data, f"p{i}.png"))
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'pix2pix.py'), '--data', data, '--output', out, '--train', '--epochs', '1',
                          '--batch-size', '2', '--logging', 'false', '--seed', '7', '--edge-weight', '0.25', '--save-weights', 'false'],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    logs = os.path.join(out, sorted(os.listdir(out))[0], 'logs')
    strict = lambda p: json.loads(open(p).read(), parse_constant=lambda s: pytest.fail(f"not strict JSON: {s} in {p}"))
    assert strict(os.path.join(logs, 'config.json'))['edge_weight'] == 0.25
    for name in ('train_metrics.json', 'val_metrics.json'):
        m = strict(os.path.join(logs, name))
        assert 'Generator Loss (Secondary)' in m
        for key, vals in m.items():
            assert len(vals) == 1 and all(np.isfinite(v) for v in vals), (name, key, vals)
