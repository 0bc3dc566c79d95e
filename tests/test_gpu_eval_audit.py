"""Every library call of the inference forward (`model(x, training=False)`, `--predict-training false`, tiled prediction), at the
shapes and with the descriptors the product code builds itself, checked on its own against an fp64 reference of the values it read
(tests/launch_audit.py), as tests/test_gpu_launch_audit.py does for the training step.  In inference mode every BatchNorm layer is
one convolution on folded weights with bias + activation in its epilogue: the bias row of the GEMM tile epilogues (plain and
parity form), the bias load of the split-K slab reduce and bias + activation on the 256-row and 1024-row tile classes are reached
by no launch of the training step.  The end-to-end gates of tests/test_gpu_inference.py (5e-2 after a saturating tanh in bf16)
cannot see a bias taken from the neighbouring channel; the per-call gate here is one output ulp plus the accumulation bound.

BatchNorm state: the calibrated parameters of tests/inference_ref.py (random gamma, a fifth negative, random beta, moving
statistics near the layer's real ones), so every folded bias is non-zero and differs from channel to channel.  Inputs on the
normalize() lattice.  EVAL_AUDITED (tests/test_cpu_launch_audit.py) is the bf16 batch list; that file asserts on the host planners
alone that it reaches every plan class of B = 1..64 at 256x256 and 1..16 at 512x512, and each case here fails if the launches it
recorded are not the ones that table lists for its batch."""
import ctypes as C
import gc
import time

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from tests import launch_audit as A
from tests.inference_ref import disc_params, gen_params
from tests.test_cpu_launch_audit import EVAL_AUDITED, eval_plan_strings

pytestmark = pytest.mark.gpu

DT = {'f32': L.F32, 'bf16': L.BF16, 'f16': L.F16}
# (network, dtype, size, batch): the bf16 batches of EVAL_AUDITED; f16 at the smallest batches with an unsplit 256-row tile with
# bias (generator 8, discriminator 11); f32 (exact-MFMA kernels) at batch 2
CASES = [(n, 'bf16', s, b) for (n, s), bs in EVAL_AUDITED.items() for b in bs] + [
    ('generator', 'f16', 256, 8), ('discriminator', 'f16', 256, 11), ('generator', 'f32', 256, 2), ('discriminator', 'f32', 256, 2)]


def lattice(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, shape, generator=g).float() / 127.5 - 1.0).cuda()


def start(monkeypatch):
    # graphs and events of earlier tests must be gone before anything is built (see test_gpu_launch_audit.py)
    gc.collect()
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return A.Recorder(monkeypatch)            # before the call object: its op lists hold the bound entry points


def conv_rows(calls, rows):
    return [(c, r) for c, r in zip(calls, rows) if c.name in A.OPS]


def seen_plans(calls, rows):
    """check_conv's plan string + bias + activation of every recorded convolution (eval_plan_strings' form)."""
    return {f"{r[2]} bias {int(bool(c.args[0]._obj.bias))} act {c.args[0]._obj.act}" for c, r in conv_rows(calls, rows)}


def report(title, calls, rows, t0, t1, t2):
    print('\n' + A.table(rows, title))
    worst = A.worst_per_entry(rows)
    print(f"[{title}] worst error/gate per entry point: " + ', '.join(f"{k[4:]} {v:.3f}" for k, v in sorted(worst.items())))
    biased = [max(r[4].values()) for c, r in conv_rows(calls, rows) if c.args[0]._obj.bias and r[4]]
    print(f"[{title}] {len(rows)} calls ({sum(r[4] is not None for r in rows)} checked, {len(biased)} convolutions with bias: "
          f"worst {max(biased, default=0.0):.3f}); build + record {t1 - t0:.1f} s, audit {t2 - t1:.1f} s")
    bad = A.failures(rows)
    assert not bad, "calls outside their gates:\n" + '\n'.join(f"  {b}" for b in bad[:40])
    assert biased, "no checked convolution with a bias"


def assert_fold_checked(rows, net):
    fold = [r for r in rows if r[1] == 'gan_bn_fold_multi']
    assert len(fold) == 1 and fold[0][4] is not None
    assert {'bias', 'nk', 'inputs unchanged', 'master / nat / tr / state unchanged'} <= set(fold[0][4])
    for name, b in net.folded().bias.items():          # every folded bias non-zero, different from channel to channel
        b = b.cpu()
        assert bool((b != 0).all()) and b.unique().numel() > 0.9 * b.numel(), name


@pytest.mark.parametrize("net,dtype,size,batch", CASES, ids=[f"{n}-{d}-{s}-B{b}" for n, d, s, b in CASES])
def test_every_launch_of_the_eval_forward_against_fp64(net, dtype, size, batch, monkeypatch):
    from gan_amd.nets import Ctx, DiscriminatorNet, GeneratorNet, workspace_mb_for
    t0 = time.time()
    rec = start(monkeypatch)
    ctx = Ctx('cuda:0', dtype, workspace_mb=workspace_mb_for(batch, size))
    if net == 'generator':
        nn = GeneratorNet(ctx, 1, 'batchnorm', seed=5)
        nn.params.load_numpy(gen_params(S=size))
        call = nn.new_eval_call(batch, size)
        call.set_input(lattice((batch, size, size, 1), 7 + batch))
    else:
        nn = DiscriminatorNet(ctx, 1, True, 'batchnorm', seed=2)
        nn.params.load_numpy(disc_params())
        call = nn.new_eval_call(batch, size)
        x = lattice((batch, size, size, 2), 7 + batch)            # concatenate([inp, tar]) as the two leading channels
        v = call.xin.view(0, 2)
        L.check(ctx.lib.gan_pack(ctx.dt, x.data_ptr(), C.byref(v), ctx.stream()), "pack")
    torch.cuda.synchronize()
    with rec.recording():
        call.infer(fold=True)
    torch.cuda.synchronize()
    calls = rec.calls
    assert [c.name for c in calls][0] == 'gan_bn_fold_multi' and len(calls) == 1 + len(call.fwd_ops)
    A.label_calls(calls, call)
    t1 = time.time()
    rows = A.replay(calls)
    t2 = time.time()
    title = f"eval {net} {dtype} {size}x{size} B={batch}"
    report(title, calls, rows, t0, t1, t2)
    assert_fold_checked(rows, nn)
    want = eval_plan_strings(net, batch, size, DT[dtype])
    got = seen_plans(calls, rows)
    assert got == want, f"recorded launches differ from eval_launches() of tests/test_cpu_launch_audit.py: only recorded " \
                        f"{sorted(got - want)}, only in the table {sorted(want - got)}"
    out = call.output_f32() if net == 'generator' else call.logits.t
    assert bool(torch.isfinite(out).all())


def test_every_launch_of_a_tiled_prediction_against_fp64(monkeypatch):
    """320 x 384 uint8 image, tile 256, overlap 64, batch 3: four tiles, run as one call of 3 and one call of 1."""
    from gan_amd.base_gan import GeneratorModel
    from gan_amd.nets import Ctx, GeneratorNet, workspace_mb_for
    from gan_amd.tiling import tile_grid
    t0 = time.time()
    rec = start(monkeypatch)
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=workspace_mb_for(3, 256))
    nn = GeneratorNet(ctx, 1, 'batchnorm', seed=5)
    nn.params.load_numpy(gen_params(S=256))
    model = GeneratorModel(nn)
    assert tile_grid(320, 384, 256, 64) == (2, 2)
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 256, (320, 384, 1), generator=g, dtype=torch.uint8).cuda()
    with rec.recording():
        img = model.infer_tiled(src, tile=256, overlap=64, batch=3)
    torch.cuda.synchronize()
    first = img.clone()
    calls = rec.calls
    names = [c.name for c in calls]
    assert names[0] == 'gan_bn_fold_multi' and names.count('gan_bn_fold_multi') == 1
    assert names.count('gan_tile_gather_u8') == 2 and names.count('gan_tile_blend') == 2
    assert sorted(model._eval_calls) == [(1, 256), (3, 256)] and len(calls) == 5 + 2 * 16
    A.label_calls(calls, model)
    t1 = time.time()
    rows = A.replay(calls)                    # (a recorded entry point with neither a checker nor an ALLOWLIST entry fails here)
    t2 = time.time()
    report("eval tiled generator bf16 320x384 tile 256 overlap 64 batch 3", calls, rows, t0, t1, t2)
    assert_fold_checked(rows, nn)
    want = eval_plan_strings('generator', 3, 256) | eval_plan_strings('generator', 1, 256)
    assert seen_plans(calls, rows) == want
    torch.cuda.synchronize()
    assert bool(torch.isfinite(img).all()) and torch.equal(img, first)          # the replay blended the same image again


@pytest.mark.parametrize("batch", [1, 4])
def test_every_launch_of_the_instancenorm_eval_forward_against_fp64(batch, monkeypatch):
    """new_eval_call of an InstanceNorm generator: the training forward without dropout.  In training up0-2 always carry a mask, so
    the mask-less ReLU forms of norm_act_fwd and of the finishing slab reduce (GanNormFuse) at those shapes run only here.  Nothing to
    fold; the one launch with a bias is the head."""
    from gan_amd.nets import Ctx, GeneratorNet, workspace_mb_for
    t0 = time.time()
    rec = start(monkeypatch)
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=workspace_mb_for(batch, 256))
    nn = GeneratorNet(ctx, 1, 'instancenorm', seed=5)
    call = nn.new_eval_call(batch, 256)
    call.set_input(lattice((batch, 256, 256, 1), 17 + batch))
    torch.cuda.synchronize()
    with rec.recording():
        call.infer(fold=True)
    torch.cuda.synchronize()
    calls = rec.calls
    assert len(calls) == len(call.fwd_ops) and not any('dropout' in c.name or 'fold' in c.name for c in calls)
    A.label_calls(calls, call)
    t1 = time.time()
    rows = A.replay(calls)
    t2 = time.time()
    report(f"eval instancenorm generator bf16 256x256 B={batch}", calls, rows, t0, t1, t2)
    assert all(r[4] is not None for r in rows)                                   # convolutions and norm launches only: all checked
    # up0-2 without a mask: each finished either by the slab reduce of its convolution (norm_fuse) or by norm_act_fwd
    ups = [(c, r) for c, r in zip(calls, rows) if any(f"G.up{j}." in r[0] for j in range(3))]
    done = [r for c, r in ups if 'norm_fuse out' in r[4] or c.name == 'gan_norm_act_fwd']
    assert len(done) == 3 and not any('dropout' in r[2] for c, r in ups)
    assert bool(torch.isfinite(call.output_f32()).all())
