"""The RGB (channels = 3) training steps and inference forwards, per launch against fp64 (tests/launch_audit.py).  Every other
audit builds its steps at channels = 1, where the tanh head and the discriminator's gradient into the image run on the one-kernel
thin-N form; at 3 channels they take conv_thin_n_kernel + conv_thin_col2im_kernel (Z through the workspace), D's dx dgrad reads
weight rows [3, 6) of 6, CycleGAN's generators write their own input gradient into 3 channels, the first / last layers' wgrad
launches have sides of 3 and 6 channels, and pad channels [3, 8) ([6, 8) in D's input) sit next to every image-side store.

Cases (RGB_AUDITED / RGB_EVAL_AUDITED of tests/test_cpu_launch_audit.py, which asserts on the host planners that they reach every
class with a thin operand of B = 1..16 at 256x256 and 1..8 at 512x512 - the sweep named no class that needs another batch):
  Pix2Pix bf16 256 B = 1   the captured one-GPU step; also: its first replay equals the eager step bit for bit
  Pix2Pix f16 256 B = 1    the f16 stores of col2im, unfused Adam + loss scale
  Pix2Pix bf16 256 B = 9   conv_thin_n_kernel's grid cap (2,048 workgroups x 4 waves x 16 pixels = 8 images of 128 x 128): the
                           smallest batch with a ragged second grid-stride trip; D's parameter pass over 18 images
  Pix2Pix bf16 512 B = 1   256-row head input, 512-wide col2im rows
  CycleGAN bf16 256 B = 1  the generators' down0 dx dgrad into 3 channels, D with cin = 3, accumulate-mode wgrads over 3B
  Pix2Pix bf16 256 B = 1   data-parallel, bucketed with direct wire writes (launch_audit.identity_sync / WireAudit / AdamEnd)
  eval forwards            infer(fold=True) of the BatchNorm generator and PatchGAN at B = 1, 9; one tiled prediction of a 3-channel
                           uint8 image

Checked: every call with an operand of <= 8 channels (launch_audit.thin_call); the rest is issued unchecked, and each such
convolution / wgrad must be of a plan class the channels = 1 table holds at the same model, batch and size - the class
tests/test_gpu_launch_audit.py audits.  REQUIRED names the calls the checked set must hold; the kernels the streaming launches ran
are asserted by name, so a planner change that moves these layers to the tiled GEMM fails here instead of emptying the test.  The
pad channels of every image-side buffer must be bit-zero before the first and after the last call."""
import gc
import time

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from tests import launch_audit as A
from tests.inference_ref import disc_params, gen_params
from tests.test_cpu_launch_audit import RGB, RGB_AUDITED, RGB_EVAL_AUDITED, eval_plan_strings, plan_classes
from tests.test_gpu_launch_audit import _reset

pytestmark = pytest.mark.gpu

DT = {'bf16': L.BF16, 'f16': L.F16}
# (model, dtype, size, batch, data-parallel table or None)
CASES = [(m, 'bf16', s, b, None) for (m, s), bs in RGB_AUDITED.items() for b in bs] + [
    ('pix2pix', 'f16', 256, 1, None), ('pix2pix', 'bf16', 256, 1, 'direct')]
assert ('pix2pix', 'bf16', 256, 9, None) in CASES and ('cyclegan', 'bf16', 256, 1, None) in CASES

# (title, entry point, label fragment, distinct checked calls at least)
G_REQUIRED = [("{g}.down0 fwd", 'gan_conv2d_fwd', "{g}.down0.kernel", 1), ("{g}.down0 wgrad", 'gan_conv_wgrad', "{g}.down0.kernel", 1),
              ("{g}.last fwd", 'gan_convT2d_fwd', "{g}.last.kernel", 1), ("{g}.last dgrad", 'gan_convT2d_dgrad', "{g}.last.kernel", 1),
              ("{g}.last wgrad", 'gan_conv_wgrad', "{g}.last.kernel", 1), ("{g}.last bias gradient", 'gan_bias_grad', "{g}.last.bias", 1)]
D_REQUIRED = [("{d}.down0 fwd, both invocations", 'gan_conv2d_fwd', "{d}.down0.kernel", 2), ("{d}.down0 wgrad", 'gan_conv_wgrad', "{d}.down0.kernel", 1),
              ("{d}.down0 dx dgrad", 'gan_conv2d_dgrad', "{d}.down0.kernel", 1), ("{d}.last fwd", 'gan_conv2d_fwd', "{d}.last.kernel", 2),
              ("{d}.last dgrad", 'gan_conv2d_dgrad', "{d}.last.kernel", 2), ("{d}.last wgrad", 'gan_conv_wgrad', "{d}.last.kernel", 1),
              ("{d}.last bias gradient", 'gan_bias_grad', "{d}.last.bias", 1)]


def required(model):
    """Pix2Pix: G, D.  CycleGAN: both generators (each also with its down0 dx dgrad, gan_conv2d_dgrad labelled down0) and both
    discriminators.  D.down0 fwd / D.last fwd: Pix2Pix runs the two invocations (real, fake) as separate launches on separate
    samples, both required; D.last dgrad: once in the parameter pass (2B), once in the input pass (B)."""
    fill = lambda spec, **k: [(t.format(**k), e, f.format(**k), n) for t, e, f, n in spec]
    if model == 'pix2pix':
        return fill(G_REQUIRED, g='G') + fill(D_REQUIRED, d='D')
    out = []
    for g in ('Gg', 'Gf'):
        out += fill(G_REQUIRED, g=g) + [(f"{g}.down0 dx dgrad", 'gan_conv2d_dgrad', f"{g}.down0.kernel", 1)]
    for d in ('Dx', 'Dy'):                          # (the merged schedule runs D(real) ++ D(fake) as ONE forward over 2B)
        out += [(t, e, f, 1 if e == 'gan_conv2d_fwd' else n) for t, e, f, n in fill(D_REQUIRED, d=d)]
    return out


def lattice(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, shape, generator=g).float() / 127.5 - 1.0).cuda()


def image_buffers(obj):
    """[(name, tensor, real channels)] of the image-side buffers of every call object of a step / model / call: the generators'
    xin, out, dgen, dgen2 (their own channels), D's xin and dxin (its input channels)."""
    from gan_amd.nets import DiscCall, DiscEvalCall, GenCall, GenEvalCall
    out, seen = [], set()

    def walk(o, name, depth=0):
        if id(o) in seen or depth > 3:
            return
        seen.add(id(o))
        if isinstance(o, (GenCall, GenEvalCall)):
            for k in ('xin', 'out', 'dgen', 'dgen2'):
                if hasattr(o, k):
                    out.append((f"{name}.{k}", getattr(o, k).t, o.C))
        elif isinstance(o, (DiscCall, DiscEvalCall)):
            for k in ('xin', 'dxin'):
                if hasattr(o, k):
                    out.append((f"{name}.{k}", getattr(o, k).t, o.net.cin))
        elif isinstance(o, (list, tuple)):
            for i, e in enumerate(o):
                walk(e, f"{name}[{i}]", depth + 1)
        elif isinstance(o, dict):
            for k, e in o.items():
                walk(e, f"{name}[{k}]", depth + 1)
        elif hasattr(o, '__dict__') and type(o).__module__.startswith('gan_amd'):
            for k, e in vars(o).items():
                walk(e, f"{name}.{k}" if name else k, depth + 1)
    walk(obj, '')
    return out


def kernel_name_failures(calls, rows):
    """Checked streaming launches whose launch log does not name the kernels expected of them."""
    bad = []
    for c, r in zip(calls, rows):
        if c.name not in A.OPS or r[4] is None:
            continue
        d, ks = c.args[0]._obj, r[3]
        if d.dtype != L.F32 and d.y.c in (3, 6) and d.x.c in (64, 128, 512):
            if 'conv_thin_n_kernel' not in ks or 'conv_thin_col2im_kernel' not in ks:
                bad.append(f"{r[0]}: y.c = {d.y.c}, launched {ks or 'nothing'}")
        if d.dtype != L.F32 and d.x.c == 8 and d.y.c % 64 == 0 and c.name in ('gan_conv2d_fwd', 'gan_convT2d_dgrad'):
            if 'conv_thin_k_kernel' not in ks:
                bad.append(f"{r[0]}: 8-channel input, launched {ks or 'nothing'}")
    return bad


def class_failures(calls, rows, table3, table1):
    """Recorded conv / wgrad calls whose plan class the channels = 3 table does not hold (the table no longer mirrors the step), and
    unchecked ones whose class the channels = 1 table - what tests/test_gpu_launch_audit.py audits - does not hold.
    Left out: the launches that finish their layer in the slab reduce (GanNormFuse honoured, statistics 'full', conv_own among
    them).  The host tables request the fusion with an empty GanNormFuse, which the planner does not honour, so they hold no 'full'
    class at any channel count (measured: 28 such launches in the Pix2Pix B = 1 step).  None of them has an operand of <= 8
    channels - asserted - so their descriptors are those of the channels = 1 step."""
    t3, t1 = {A.same_class(k) for k in table3}, {A.same_class(k) for k in table1}
    bad = []
    for c, r in zip(calls, rows):
        k = A.call_class(c)
        if k is None:
            continue
        if 'full' in k:
            if A.thin_call(c):
                bad.append(f"{r[0]} ({c.name}): a launch with a thin operand finishes its layer (class {k}): not in any table")
            continue
        if k not in t3:
            bad.append(f"{r[0]} ({c.name}): class {k} is not in the channels = 3 table")
        if r[4] is None and k not in t1:
            bad.append(f"{r[0]} ({c.name}): issued unchecked, but class {k} is not in the channels = 1 table")
    return bad


def summary(title, calls, rows, secs):
    print('\n' + A.table(rows, title))
    worst = A.worst_per_entry(rows)
    print(f"[{title}] worst error/gate per entry point: " + ', '.join(f"{k[4:]} {v:.3f}" for k, v in sorted(worst.items())))
    checked = sum(r[4] is not None for r in rows)
    same = sum(r[2] == A.AS_ONE_GPU for r in rows)
    ks = sorted({k for r in rows if r[4] is not None for k in r[3].split(',') if k.startswith('conv_thin')})
    print(f"[{title}] {len(rows)} calls issued, {checked} checked (thin operand), {same} as at channels = 1, {len(rows) - checked - same} "
          f"allowlisted; streaming kernels in the checked rows: {ks}; " + ', '.join(f"{k} {v:.1f} s" for k, v in secs.items()))
    print(f"[{title}] slowest calls: " + ', '.join(f"{lab} {sec:.2f} s" for sec, lab, _ in sorted(A.TIMES, reverse=True)[:3]))


@pytest.mark.parametrize("model,dtype,size,batch,ddp", CASES,
                         ids=[f"{m}-{d}-{s}-B{b}" + ("-ddp-wire-direct" if t else "") for m, d, s, b, t in CASES])
def test_every_thin_launch_of_the_rgb_step_against_fp64(model, dtype, size, batch, ddp, monkeypatch):
    from gan_amd.nets import Ctx, workspace_mb_for
    from gan_amd.steps import CycleGANStep, Pix2PixStep
    gc.collect()                                  # (graphs of the previous case: see test_gpu_launch_audit.py)
    torch.cuda.synchronize()
    t0 = time.time()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    rec = A.Recorder(monkeypatch)
    rec.hook_capture(monkeypatch)
    ctx = Ctx('cuda:0', dtype, workspace_mb=workspace_mb_for(batch, size, RGB))
    if model == 'pix2pix':
        st = Pix2PixStep(ctx, batch, size, RGB, lam=100.0, seed=123)
    else:
        st = CycleGANStep(ctx, batch, size, RGB, lam=10.0, seed=123)
    bufs = image_buffers(st)
    assert len(bufs) >= (6 if model == 'pix2pix' else 12), [b[0] for b in bufs]
    assert not A.pad_channels(bufs)
    saved = [(n.params.master.clone(), {k: t.clone() for k, t in n.params.state.items()}) for n in st.nets()]
    g = torch.Generator().manual_seed(7 + batch)
    inputs = [(torch.randint(0, 256, (batch, size, size, RGB), generator=g).float() / 127.5 - 1.0).cuda() for _ in range(2)]
    first_case = (model, dtype, size, batch, ddp) == ('pix2pix', 'bf16', 256, 1, None)
    if first_case:                                # the eager step from the initial state, before anything is captured
        eager = st.train_step(*inputs, True).clone()
        eager_out = st.g.out.t.clone()
    sync = wa = None
    if ddp:
        sync = st.sync = A.identity_sync(st, True)
        assert sync.world == 2 and sync.active
    replay = st.capture(training=True)
    torch.cuda.synchronize()
    if ddp:                                       # G1..G4 | A0..A3 (tests/test_gpu_ddp_audit.py)
        starts = rec.graph_starts + [len(rec.calls)]
        graphs = [rec.calls[a:b] for a, b in zip(starts[:-1], starts[1:])]
        assert hasattr(st, 'buckets') and len(graphs) == 8
        compute, adam = sum(graphs[:4], []), sum(graphs[4:], [])
        assert not any(c.name.startswith('gan_adam') for c in compute) and not any(c.name in ('gan_conv_wgrad', 'gan_grad_pack') for c in adam)
    else:
        compute, adam = list(rec.calls), []
    calls = compute + adam
    assert calls, "nothing recorded inside the capture body"
    A.label_calls(calls, st)

    def reset():
        _reset(st, saved)                         # initial weights, step 0, small non-zero moments
        for call in vars(st).values():
            if hasattr(call, 'mask_draws'):
                call.mask_draws.zero_()
        for t, src in zip(replay.inputs, inputs):
            t.copy_(src)
        torch.cuda.synchronize()
    reset()
    if first_case:                                # the first replay of the captured step = the eager step, bit for bit
        first = replay(*replay.inputs)[:4].clone()
        torch.cuda.synchronize()
        print(f"\npix2pix bf16 channels 3: eager {eager.tolist()} replayed {first.tolist()}")
        assert torch.isfinite(first).all() and torch.equal(first, eager)
        assert A.bit_equal(st.g.out.t, eager_out) == 0.0, "generator output of the first replay differs from the eager step's"
        reset()
    if ddp:
        wa = A.WireAudit(st, sync)
        wa.fill()
    before = A.pad_channels(bufs)
    t1 = time.time()
    del A.TIMES[:]
    # (data-parallel: every wgrad / bias gradient is checked, as in tests/test_gpu_ddp_audit.py - WireAudit counts the writers of a
    # wire element inside the checks)
    check = (lambda c: A.thin_call(c) or c.name in ('gan_conv_wgrad', 'gan_bias_grad')) if ddp else A.thin_call
    rows = A.replay(compute, check=check, wire=wa)
    t2 = time.time()
    cover = end_rows = []
    if ddp:
        cover = wa.coverage()
        end = A.AdamEnd(st, sync)
        end.snapshot()
        rows += A.replay(adam, check=check)
        end_rows = end.check()
    torch.cuda.synchronize()
    after = A.pad_channels(bufs)
    t3 = time.time()
    title = f"rgb {model} {dtype} {size}x{size} B={batch}" + (" data-parallel, wire direct" if ddp else "")
    summary(title, calls, rows + end_rows, {'build + capture': t1 - t0, 'compute calls': t2 - t1, 'rest': t3 - t2})
    # every required call was checked; no unchecked call is of a class the channels = 1 audit does not hold
    miss = A.missing_required(calls, rows, required(model))
    assert not miss, "required calls that were not checked:\n" + '\n'.join(miss)
    strings = set()
    table3 = plan_classes(model, batch, size, DT[dtype], ddp=ddp, channels=RGB, strings=strings)
    table1 = plan_classes(model, batch, size, DT[dtype], ddp=ddp)
    bad = class_failures(calls, rows, table3, table1)
    assert not bad, "plan classes:\n" + '\n'.join(bad)
    wg = [r for r in rows if r[1] == 'gan_conv_wgrad']
    assert any(r[4] is not None for r in wg)
    if ddp:                                       # the plan strings of EVERY wgrad launch (checked or not) are the table's
        seen = {A.plan_of(c) for c in calls if c.name == 'gan_conv_wgrad'}
        assert seen == strings, f"wgrad plans differ from the table: only recorded {sorted(seen - strings)}, only in the table {sorted(strings - seen)}"
        assert any(s.endswith(' wire') for s in seen) and all(r[4] is not None for r in wg if r[2] != A.AS_ONE_GPU)
        packs = [r for r in rows if r[1] == 'gan_grad_pack']
        assert packs and all(r[4] is not None for r in packs)
        assert not cover, "wire coverage:\n" + '\n'.join(cover)
        assert end_rows and all(r[4] for r in end_rows)
    names = kernel_name_failures(calls, rows)
    assert not names, "kernels:\n" + '\n'.join(names)
    two = [r for c, r in zip(calls, rows) if r[4] is not None and 'conv_thin_col2im_kernel' in r[3]]
    assert len(two) >= (2 if model == 'pix2pix' else 6), [r[0] for r in two]
    assert not before and not after, f"pad channels: before the first call {before}, after the last {after}"
    bad = A.failures(rows + end_rows)
    assert not bad, "calls outside their gates:\n" + '\n'.join(f"  {b}" for b in bad[:40])
    assert np.isfinite(st.losses.cpu().numpy()).all()


def eval_checks(title, owner, calls, rows, t0, t1, t2):
    print('\n' + A.table(rows, title))
    worst = A.worst_per_entry(rows)
    print(f"[{title}] worst error/gate per entry point: " + ', '.join(f"{k[4:]} {v:.3f}" for k, v in sorted(worst.items())))
    print(f"[{title}] {len(rows)} calls ({sum(r[4] is not None for r in rows)} checked); build + record {t1 - t0:.1f} s, audit {t2 - t1:.1f} s")
    names = kernel_name_failures(calls, rows)
    assert not names, "kernels:\n" + '\n'.join(names)
    pads = A.pad_channels(image_buffers(owner))
    assert not pads, f"pad channels after the last call: {pads}"
    bad = A.failures(rows)
    assert not bad, "calls outside their gates:\n" + '\n'.join(f"  {b}" for b in bad[:40])


def eval_seen(calls):
    return {f"{A.plan_of(c)} bias {int(bool(c.args[0]._obj.bias))} act {c.args[0]._obj.act}" for c in calls if c.name in A.OPS}


EVAL_CASES = [(n, b) for (n, s), bs in RGB_EVAL_AUDITED.items() for b in bs]


@pytest.mark.parametrize("net,batch", EVAL_CASES, ids=[f"{n}-B{b}" for n, b in EVAL_CASES])
def test_every_thin_launch_of_the_rgb_eval_forward_against_fp64(net, batch, monkeypatch):
    import ctypes as C
    from gan_amd.nets import Ctx, DiscriminatorNet, GeneratorNet, workspace_mb_for
    gc.collect()
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0 = time.time()
    rec = A.Recorder(monkeypatch)
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=workspace_mb_for(batch, 256, RGB))
    if net == 'generator':
        nn = GeneratorNet(ctx, RGB, 'batchnorm', seed=5)
        P = gen_params(S=256)
    else:
        nn = DiscriminatorNet(ctx, RGB, True, 'batchnorm', seed=2)
        P = disc_params()
    # the calibrated BatchNorm state of tests/inference_ref.py (every folded bias non-zero); its channels = 1 first / last kernels
    # do not fit: those keep this network's own initial values, and the head's bias is set apart from channel to channel
    own = nn.params.to_numpy()
    P = {k: (v if np.shape(v) == np.shape(own[k]) else own[k]) for k, v in P.items() if k in own}
    if net == 'generator':
        P['last.bias'] = np.array([0.31, -0.17, 0.05], np.float32)
    nn.params.load_numpy(P)
    call = nn.new_eval_call(batch, 256)
    assert not A.pad_channels(image_buffers(call))
    if net == 'generator':
        call.set_input(lattice((batch, 256, 256, RGB), 7 + batch))
    else:
        x = lattice((batch, 256, 256, 2 * RGB), 7 + batch)        # concatenate([inp, tar]): the six leading channels
        v = call.xin.view(0, 2 * RGB)
        L.check(ctx.lib.gan_pack(ctx.dt, x.data_ptr(), C.byref(v), ctx.stream()), "pack")
    torch.cuda.synchronize()
    with rec.recording():
        call.infer(fold=True)
    torch.cuda.synchronize()
    calls = rec.calls
    assert calls[0].name == 'gan_bn_fold_multi' and len(calls) == 1 + len(call.fwd_ops)
    A.label_calls(calls, call)
    t1 = time.time()
    rows = A.replay(calls, check=lambda c: c.name == 'gan_bn_fold_multi' or A.thin_call(c))
    t2 = time.time()
    eval_checks(f"rgb eval {net} bf16 256x256 B={batch}", call, calls, rows, t0, t1, t2)
    want = eval_plan_strings(net, batch, 256, channels=RGB)
    assert eval_seen(calls) == want, f"only recorded {sorted(eval_seen(calls) - want)}, only in the table {sorted(want - eval_seen(calls))}"
    # unchecked: the inner layers, whose launches are those of the channels = 1 forward at this batch (tests/test_gpu_eval_audit.py's class)
    inner1 = eval_plan_strings(net, batch, 256)
    for c, r in zip(calls, rows):
        if c.name in A.OPS and r[4] is None:
            s = f"{A.plan_of(c)} bias {int(bool(c.args[0]._obj.bias))} act {c.args[0]._obj.act}"
            assert s in inner1, (r[0], s)
    tag = 'G' if net == 'generator' else 'D'
    miss = A.missing_required(calls, rows, [(f"{tag}.down0 fwd", 'gan_conv2d_fwd', f"{tag}.down0.kernel", 1),
                                            (f"{tag}.last fwd", 'gan_convT2d_fwd' if net == 'generator' else 'gan_conv2d_fwd', f"{tag}.last.kernel", 1)])
    assert not miss, '\n'.join(miss)
    if net == 'generator':
        head = [r for c, r in zip(calls, rows) if c.name == 'gan_convT2d_fwd' and r[4] is not None]
        assert len(head) == 1 and 'conv_thin_col2im_kernel' in head[0][3] and calls[-1].args[0]._obj.bias
        out = call.output_f32()
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
    else:
        assert bool(torch.isfinite(call.logits.t).all())


def test_every_thin_launch_of_a_tiled_rgb_prediction_against_fp64(monkeypatch):
    """320 x 384 x 3 uint8 image, tile 256, overlap 64, batch 3: four tiles, one call of 3 and one of 1 (as the eval audit's)."""
    from gan_amd.base_gan import GeneratorModel
    from gan_amd.nets import Ctx, GeneratorNet, workspace_mb_for
    from gan_amd.tiling import tile_grid
    gc.collect()
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0 = time.time()
    rec = A.Recorder(monkeypatch)
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=workspace_mb_for(3, 256, RGB))
    nn = GeneratorNet(ctx, RGB, 'batchnorm', seed=5)
    own = nn.params.to_numpy()
    P = {k: (v if np.shape(v) == np.shape(own[k]) else own[k]) for k, v in gen_params(S=256).items() if k in own}
    P['last.bias'] = np.array([0.31, -0.17, 0.05], np.float32)
    nn.params.load_numpy(P)
    model = GeneratorModel(nn)
    assert tile_grid(320, 384, 256, 64) == (2, 2)
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 256, (320, 384, RGB), generator=g, dtype=torch.uint8).cuda()
    with rec.recording():
        img = model.infer_tiled(src, tile=256, overlap=64, batch=3)
    torch.cuda.synchronize()
    first = img.clone()
    calls = rec.calls
    names = [c.name for c in calls]
    assert names.count('gan_bn_fold_multi') == 1 and names.count('gan_tile_gather_u8') == 2 and names.count('gan_tile_blend') == 2
    assert sorted(model._eval_calls) == [(1, 256), (3, 256)]
    A.label_calls(calls, model)
    t1 = time.time()
    rows = A.replay(calls, check=lambda c: c.name == 'gan_bn_fold_multi' or A.thin_call(c))
    t2 = time.time()
    eval_checks("rgb eval tiled generator bf16 320x384x3 tile 256 overlap 64 batch 3", model, calls, rows, t0, t1, t2)
    assert eval_seen(calls) == eval_plan_strings('generator', 3, 256, channels=RGB) | eval_plan_strings('generator', 1, 256, channels=RGB)
    heads = [r for c, r in zip(calls, rows) if c.name == 'gan_convT2d_fwd' and r[4] is not None]
    assert len(heads) == 2 and all('conv_thin_n_kernel' in r[3] and 'conv_thin_col2im_kernel' in r[3] for r in heads)
    torch.cuda.synchronize()
    assert tuple(img.shape)[-1] == RGB and bool(torch.isfinite(img).all()) and torch.equal(img, first)
