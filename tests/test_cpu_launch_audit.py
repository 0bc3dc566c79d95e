"""CPU side of the launch audit (tests/launch_audit.py, tests/test_gpu_launch_audit.py, tests/test_gpu_wide_audit.py):
  - the audit's fp64 references of the four conv entry points and of wgrad, decoded from the device weight layout, against the
    oracle's Keras-layout convolutions;
  - plan coverage: the plan class of every convolution / wgrad launch in the table of plan_classes() (the captured one-GPU Pix2Pix
    and CycleGAN steps at channels = 1, see there) at B = 1..16 (256x256) and B = 1..8 (512x512, BASELINE config 4's per-GPU batch),
    from the host-side planners, must be reached by a batch the GPU audit runs.  A planner change that creates a class no audited
    batch reaches fails here and names the batch sizes that reach it;
  - the wide sweeps (tests/test_gpu_wide_audit.py): the classes keyed by (dtype family, class) - 16-bit and fp32 - over Pix2Pix and
    CycleGAN at B = 1..64 / 1..32 (256x256) and 1..16 (512x512) at 16-bit storage, 1..16 / 1..8 at fp32, from tables that file a
    launch which finishes its layer under its own class and hold the captured schedule's discriminator forward alone; every class
    must be reached by a case of tests/test_gpu_launch_audit.py of the same family or by one of WIDE_FULL / WIDE_CLASS;
  - the same for the inference forward (eval_plan_classes(): the BatchNorm generator and PatchGAN in eval mode, every BatchNorm
    layer one convolution with bias + activation; tests/test_gpu_eval_audit.py) at B = 1..64 (256x256) and B = 1..16 (512x512);
  - the gate of check_conv and the bit-equality of check_fold must be able to fail: a float32 model of convolution + bias +
    activation + rounding to storage sits inside the gate, the wrong variants a kernel could plausibly compute (a bias from the
    neighbouring channel / channel group / parity column, dropped on the second half of the columns, activation before the bias,
    the wrong activation or slope; in the fold eps outside the root, an unscaled moving mean, the other layout) land >= 2x outside;
  - the RGB steps (channels = 3, tests/test_gpu_rgb_audit.py): the tables take a `channels` parameter, the class of a streaming
    launch carries its sub-form (one kernel, or Z through the workspace in two launches), RGB_AUDITED must reach every class with a
    thin operand, and a float32 model of the two-launch thin-N convolution sits inside the gate while its wrong variants (swapped
    taps, the other parity's tap table at the border, a neighbouring channel's Z or bias, a dropped channel, a 3-pitch store, the
    wrong weight rows, dw rows at stride 8) do not."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from oracle import torch_ref as R
from tests import launch_audit as A

HAVE_LIB = os.path.exists(L.LIB_PATH)

# the GPU audit's cases (tests/test_gpu_launch_audit.py::AUDIT_CASES), 16-bit storage: (model, size) -> batches
AUDITED = {('pix2pix', 256): (1, 3, 5, 8, 9, 16), ('pix2pix', 512): (1, 3, 5, 6), ('cyclegan', 256): (1, 4, 9, 15)}
SWEEP = {('pix2pix', 256): range(1, 17), ('pix2pix', 512): range(1, 9), ('cyclegan', 256): range(1, 17)}


def _nat(w_hwio):
    """device NK copies of a Keras kernel [4,4,A,B]: native [16][A][B], transposed [16][B][A]"""
    k = torch.as_tensor(w_hwio, dtype=torch.float64).reshape(16, w_hwio.shape[2], w_hwio.shape[3])
    return k, k.transpose(1, 2).contiguous()


def test_audit_conv_references_match_the_oracle_layouts():
    g = np.random.default_rng(3)
    x = torch.as_tensor(g.standard_normal((2, 8, 8, 8)))
    w = g.standard_normal((4, 4, 8, 16))             # Conv2D HWIO (cin 8, cout 16)
    nat, tr = _nat(w)
    y = R.conv(x, torch.as_tensor(w), 2)
    assert torch.allclose(A.conv_ref(0, x, tr, 2), y)                    # conv_fwd: transposed copy, rows = cout
    dy = torch.as_tensor(g.standard_normal(tuple(y.shape)))
    xr = x.clone().requires_grad_(True)
    wr = torch.as_tensor(w).requires_grad_(True)
    (R.conv(xr, wr, 2) * dy).sum().backward()
    assert torch.allclose(A.conv_ref(1, dy, nat, 2), xr.grad)           # conv_dgrad: native copy, rows = cin
    assert torch.allclose(A.wgrad_ref(x, dy, 2, 8, 16), wr.grad.reshape(16, 8, 16))
    # stride 1 (ZeroPadding2D + 'valid': 8 -> 7)
    y1 = R.nhwc(torch.nn.functional.conv2d(R.nchw(x), torch.as_tensor(w).permute(3, 2, 0, 1), stride=1, padding=1))
    assert torch.allclose(A.conv_ref(0, x, tr, 1), y1)
    assert tuple(A.conv_ref(1, y1, nat, 1).shape) == tuple(x.shape)
    # Conv2DTranspose (kh,kw,cout,cin) = (.., 16, 8)
    wt = g.standard_normal((4, 4, 16, 8))
    natT, trT = _nat(wt)
    yt = R.convT(x, torch.as_tensor(wt))
    assert torch.allclose(A.conv_ref(2, x, natT, 2), yt)                 # convT_fwd: native copy, rows = cout
    dyt = torch.as_tensor(g.standard_normal(tuple(yt.shape)))
    xr = x.clone().requires_grad_(True)
    wr = torch.as_tensor(wt).requires_grad_(True)
    (R.convT(xr, wr) * dyt).sum().backward()
    assert torch.allclose(A.conv_ref(3, dyt, trT, 2), xr.grad)          # convT_dgrad: transposed copy, rows = cin
    assert torch.allclose(A.wgrad_ref(dyt, x, 2, 16, 8), wr.grad.reshape(16, 16, 8))


def test_audit_ulp_gate():
    v = torch.tensor([1.0, 1.5, -3.0, 0.0, 1e-9], dtype=torch.float64)
    assert A.ulp(v, L.BF16).tolist()[:3] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    assert A.ulp(v, L.F16)[3] == 2.0 ** -24 and A.ulp(v, L.F16)[4] == 2.0 ** -24
    assert A.ulp(v, L.F32)[0] == 2.0 ** -23


# ---- plan coverage ---------------------------------------------------------------------------------------------------------
# The step objects need a device to be built, so the launches are listed here, one table per network, with the shapes, channel
# counts, request flags (fused statistics, GanBwdFuse with its cols / skip input, GanNormFuse, bias / activation / fp32 logits) and
# wgrad scheduling hints that gan_amd/nets.py and gan_amd/steps.py give them in the captured one-GPU step at `channels` image channels
# (1: the steps the GPU audit builds; 3: those of tests/test_gpu_rgb_audit.py).
G_DOWN = [64, 128, 256, 512, 512, 512, 512, 512]
G_UP = [512, 512, 512, 512, 256, 128, 64]


def T(n, h, c):
    return L.GanTensor(16, n, h, h, c, c)


def IMG(n, h, c):
    """c real channels of an 8-channel image-side pixel (out, dxin, dgen2: the views nets.py makes with Buf.view(0, c))."""
    return L.GanTensor(16, n, h, h, c, 8)


def plan_classes(model, B, S, dt=L.BF16, ddp=None, strings=None, channels=1, thin=None, fused=False, captured=False):
    """{class: label} of every conv / wgrad launch of one captured step at `channels` image channels (1: the steps of
    tests/test_gpu_launch_audit.py; 3: tests/test_gpu_rgb_audit.py).  thin: a set that receives the classes of the launches with an
    operand of <= 8 channels (launch_audit.THIN_C: the launches whose code path depends on `channels`).
    fused: the GanNormFuse requests are complete (an output tensor, and in the forward form gamma / beta / mean / rstd, as
    nets._Builder.fwd_norm_fuse / bwd_norm_fuse fill them), so the planner honours them where the step's launches have them honoured
    and the class of such a launch reads 'full', as launch_audit.call_class reads it from a recorded descriptor.  Off (the tables
    before the wide sweeps): the request is an empty struct, which the planner never honours - such a launch is filed under the class
    it would have with its own statistics epilogue, and a recorded 'full' class is in no table.
    captured: only the discriminator forward of the captured schedule (Pix2Pix: per invocation, B images; CycleGAN: D(real) ++ D(fake)
    as one forward over 2B).  Off: both forms, of which a captured step launches one - the other's classes are then in the table of a
    batch whose step does not launch them.  With fused and captured the table holds exactly the classes the captured step launches
    (tests/test_gpu_wide_audit.py asserts it for every case it builds).
    ddp: None - the one-GPU step; 'direct' - the data-parallel Pix2Pix step on its bucketed schedule with the bf16 wire
    (Pix2PixStep._capture_bucketed): every wgrad launch is given its place in the wire buffer and writes it where
    gan_wgrad_wire_direct says it can; 'plain' - every other data-parallel schedule (fp32 wire, ddp_wire_direct = False, the phased
    schedules of Pix2Pix and CycleGAN): plain-write wgrad launches.  The data-parallel launches carry neither GanAdamFuse nor
    accumulate (CycleGAN's wide wgrads write), the convolutions, `concurrent` and the wide 3B operands are those of the one-GPU step.
    strings: a set that receives the wgrad plan strings as launch_audit.check_wgrad writes them (the GPU cases compare).
    Pix2Pix: G at B images (wgrads on a side lane: concurrent 1); D forward per invocation (B images, the captured schedule) and
    batched (2B, two BatchNorm groups); D's parameter pass over 2B, its input pass (dgrads + the dx dgrad into the generator's
    gradient) over B; D wgrads concurrent 0.
    CycleGAN (merged two-chain schedule): each generator at 2B ([fake; same]) and B (the cycle call, with its dx dgrad), its wgrads
    over both calls at once (3B, concurrent 2); D as for Pix2Pix with InstanceNorm groups = images, wgrads concurrent 2."""
    lib = L.load()
    info, winfo = (C.c_int32 * 5)(), (C.c_int32 * 4)()
    out = {}
    inorm = model == 'cyclegan'
    ng = (lambda n, calls: n) if inorm else (lambda n, calls: calls)     # statistics groups of n images in `calls` invocations

    def conv(tag, op, x, y, stride=2, groups=0, norm_fuse=False, bwd=None, w_rows=None, act=0, bias=False, y_f32=0):
        """bwd: None, or (cols, normalised, skip) of the GanBwdFuse request (the layer below)."""
        nf = L.GanNormFuse() if norm_fuse else None
        bf = None
        if bwd is not None:
            cols, normed, skip = bwd
            bf = L.GanBwdFuse()
            bf.ref, bf.act, bf.slope, bf.cols = y, L.ACT_LRELU, 0.3, cols
            if normed:
                bf.mean = bf.rstd = bf.gamma = bf.beta = 16
            else:
                groups = 0                           # activation-only backward: no statistics partials
            if skip:
                bf.add = L.GanTensor(16, y.n, y.h, y.w, cols, cols)
        if fused and nf is not None:
            oc = bwd[0] if bwd is not None else y.c
            nf.out = L.GanTensor(16, y.n, y.h, y.w, oc, oc)
            if bwd is None:
                nf.gamma = nf.beta = nf.mean = nf.rstd = 16
        d = L.GanConvDesc(dt, stride, x, y, 16, w_rows or y.c, 16 if bias else None, act, 0.3, y_f32, 16, 1 << 40,
                          16 if groups else None, groups, 1 << 30, C.addressof(bf) if bf is not None else None,
                          C.addressof(nf) if nf is not None else None)
        assert lib.gan_conv_plan_info(C.byref(d), op, info) == 0, tag
        key = A.conv_class(d, op, requested=groups)      # (streaming kernels: + the one-kernel / two-launch sub-form)
        out.setdefault(key, tag)
        if thin is not None and min(x.c, y.c, d.w_rows) <= A.THIN_C:
            thin.add(key)

    def wgrad(tag, big, small, big_c, small_c, stride, conc):
        d = L.GanWgradDesc(dt, stride, big, small, 16, big_c, small_c, 0, 16, 1 << 40, conc, None, 64 if ddp == 'direct' else None)
        wire = 0
        if d.dw_wire:
            wire = lib.gan_wgrad_wire_direct(C.byref(d))
            assert wire in (0, 1), tag
            if not wire:
                d.dw_wire = None                     # (as nets._Builder.wgrad does)
        assert lib.gan_wgrad_plan_info(C.byref(d), winfo) == 0, tag
        key = ('wgrad', winfo[0], winfo[1], winfo[2] > 1, winfo[3], wire)
        assert key == A.wgrad_class(d, wire)
        out.setdefault(key, tag)
        if thin is not None and min(big_c, small_c) <= A.THIN_C:
            thin.add(key)
        if strings is not None:
            strings.add(A.wgrad_plan(d))

    hs = [S >> (i + 1) for i in range(8)]
    cin_up = [512] + [G_UP[j - 1] + G_DOWN[7 - j] for j in range(1, 7)]          # channels of up j's input (a7 / cat[j-1])

    def generator(n, need_dx):
        g = ng(n, 1)
        cin = 8
        for i, co in enumerate(G_DOWN):
            h_in = S >> i
            if i == 0:
                conv("G.down0 fwd", 0, T(n, h_in, cin), T(n, hs[0], co), act=L.ACT_LRELU)
            else:
                conv(f"G.down{i} fwd", 0, T(n, h_in, cin), T(n, hs[i], co), groups=g, norm_fuse=True)
                below = G_DOWN[i - 1]
                conv(f"G.down{i} dgrad", 1, T(n, hs[i], co), T(n, h_in, below), groups=g, norm_fuse=i > 1, bwd=(below, i > 1, True))
            cin = co
        if need_dx:
            conv("G.down0 dx dgrad", 1, T(n, hs[0], 64), IMG(n, S, channels))
        for j, co in enumerate(G_UP):
            h_in = hs[7 - j]
            conv(f"G.up{j} fwd", 2, T(n, h_in, cin_up[j]), T(n, 2 * h_in, co), groups=g, norm_fuse=True)
            cols = G_UP[j - 1] if j > 0 else 512
            conv(f"G.up{j} dgrad", 3, T(n, 2 * h_in, co), T(n, h_in, cin_up[j]), groups=g, norm_fuse=True, bwd=(cols, True, False))
        conv("G.last fwd", 2, T(n, hs[0], 128), IMG(n, S, channels), act=L.ACT_TANH, bias=True)
        conv("G.last dgrad", 3, T(n, S, 8), T(n, hs[0], 128), groups=g, bwd=(G_UP[6], True, False))

    def generator_wgrads(n, conc):
        cin = 8
        for i, co in enumerate(G_DOWN):
            big_c = channels if i == 0 else G_DOWN[i - 1]
            wgrad(f"G.down{i} wgrad", T(n, S >> i, cin), T(n, hs[i], co), big_c, co, 2, conc)
            cin = co
        for j, co in enumerate(G_UP):
            h_in = hs[7 - j]
            wgrad(f"G.up{j} wgrad", T(n, 2 * h_in, co), T(n, h_in, cin_up[j]), co, cin_up[j], 2, conc)
        wgrad("G.last wgrad", T(n, S, 8), T(n, hs[0], 128), channels, 128, 2, conc)

    s1, s2, s3 = S // 2, S // 4, S // 8
    s4, s5 = s3 - 1, s3 - 2
    d_cin = 2 * channels if model == 'pix2pix' else channels
    layers = [('down1', 64, 128, s1, s2, 2), ('down2', 128, 256, s2, s3, 2), ('conv', 256, 512, s3, s4, 1)]

    def disc_forward(n, calls):
        g = ng(n, calls)
        conv("D.down0 fwd", 0, T(n, S, 8), T(n, s1, 64), act=L.ACT_LRELU)
        for name, ci, co, hi, ho, st in layers:
            conv(f"D.{name} fwd", 0, T(n, hi, ci), T(n, ho, co), st, groups=g, norm_fuse=True)
        conv("D.last fwd", 0, T(n, s4, 512), T(n, s5, 1), 1, bias=True, y_f32=1)

    def disc_chain(n, calls, params, conc):
        g = ng(n, calls)
        conv("D.last dgrad", 1, T(n, s5, 8), T(n, s4, 512), 1, groups=g, bwd=(512, True, False))
        for name, ci, co, hi, ho, st in reversed(layers):
            conv(f"D.{name} dgrad", 1, T(n, ho, co), T(n, hi, ci), st, groups=g, norm_fuse=name != 'down1',
                 bwd=(ci, name != 'down1', False))
        if params:
            wgrad("D.last wgrad", T(n, s4, 512), T(n, s5, 8), 512, 1, 1, conc)
            for name, ci, co, hi, ho, st in layers:
                wgrad(f"D.{name} wgrad", T(n, hi, ci), T(n, ho, co), ci, co, st, conc)
            wgrad("D.down0 wgrad", T(n, S, 8), T(n, s1, 64), d_cin, 64, 2, conc)
        else:
            conv("D.down0 dx dgrad", 1, T(n, s1, 64), IMG(n, S, channels), w_rows=d_cin)

    if model == 'pix2pix':
        generator(B, False)
        generator_wgrads(B, 1)
        d_conc = 0
    else:
        for _ in range(2):                       # G_g and G_f: the same launches
            generator(2 * B, False)
            generator(B, True)
            generator_wgrads(3 * B, 2)
        d_conc = 2
    if not captured or model == 'pix2pix':
        disc_forward(B, 1)
    if not captured or model == 'cyclegan':
        disc_forward(2 * B, 2)
    disc_chain(2 * B, 2, True, d_conc)
    disc_chain(B, 1, False, d_conc)
    return out


@pytest.mark.skipif(not HAVE_LIB, reason="library not built")
def test_audited_batches_reach_every_plan_class():
    missing = []
    for key, batches in SWEEP.items():
        model, S = key
        reach = {}
        for B in batches:
            for cls, tag in plan_classes(model, B, S).items():
                reach.setdefault(cls, []).append((B, tag))
        audited = set()
        for B in AUDITED[key]:
            audited |= set(plan_classes(model, B, S))
        for cls, where in reach.items():
            if cls not in audited:
                missing.append(f"{model} {S}x{S}: class {cls} ({where[0][1]}) reached at B = {[b for b, _ in where]}, audited {AUDITED[key]}")
    assert not missing, "plan classes no audited batch reaches:\n" + "\n".join(missing)


# ---- wide sweeps: fp32, CycleGAN 512x512 and the batches above SWEEP (tests/test_gpu_wide_audit.py) ---------------------------------
# SWEEP above is 16-bit storage only and ends at the batches of BASELINE's configurations.  The command lines accept any
# --batch-size (the inference sweep already goes to 64 / 16), BASELINE config 5 is CycleGAN at 512x512, and fp32 - the exact-MFMA
# path every oracle-parity gate rests on - had one audited case.  conv_class() carries no dtype, so a class is keyed here by
# (dtype family, class): the planner tells 16-bit storage from fp32 and nothing else (asserted below for F16 / BF16 over the whole
# 16-bit sweeps).  A family's classes are pooled over models and sizes: a class is a kernel, tile, split and epilogue form, whichever
# network launches it.  The tables are plan_classes(fused=True, captured=True): a launch that finishes its layer (GanNormFuse
# honoured) has a class of its own ('full'), as launch_audit.call_class gives a recorded one, and the discriminator forward is the
# captured schedule's alone, so a batch is not credited with a class its step never launches.
FAMILY = {'bf16': '16-bit', 'f16': '16-bit', 'f32': 'fp32'}
DTYPE = {'bf16': L.BF16, 'f16': L.F16, 'f32': L.F32}
WIDE_SWEEP = {
    '16-bit': {('pix2pix', 256): range(1, 65), ('cyclegan', 256): range(1, 33), ('pix2pix', 512): range(1, 17), ('cyclegan', 512): range(1, 17)},
    'fp32': {('pix2pix', 256): range(1, 17), ('cyclegan', 256): range(1, 17), ('pix2pix', 512): range(1, 9), ('cyclegan', 512): range(1, 9)},
}
# tests/test_gpu_wide_audit.py's cases, in the order it runs them.  WIDE_FULL: every launch checked (the cheapest CycleGAN shape: the
# f16 loss-scaled InstanceNorm chain, the fp32 CycleGAN launches).  WIDE_CLASS: (model, dtype, size) -> batches whose launches of a
# class no earlier case of the family has audited are checked; earlier = tests/test_gpu_launch_audit.py::AUDIT_CASES, WIDE_FULL and
# the entries before it here.  Per key the smallest set that covers, the smaller of two batches that reach the same classes.
WIDE_FULL = (('cyclegan', 'f16', 256, 1), ('cyclegan', 'f32', 256, 1))
WIDE_CLASS = {
    ('pix2pix', 'f32', 256): (3, 5),
    ('pix2pix', 'f32', 512): (5,),
    ('cyclegan', 'f32', 256): (9,),
    ('cyclegan', 'f32', 512): (5, 7),
    ('pix2pix', 'bf16', 256): (49,),
    ('cyclegan', 'bf16', 256): (25,),
    ('cyclegan', 'bf16', 512): (9,),
}
_WIDE = {}


def wide_classes(model, dtype, S, B):
    """{class: tag} of one step in the wide tables (same_class keys, as a recorded call has them)."""
    key = (model, dtype, S, B)
    if key not in _WIDE:
        _WIDE[key] = {A.same_class(k): tag for k, tag in plan_classes(model, B, S, DTYPE[dtype], fused=True, captured=True).items()}
    return _WIDE[key]


def wide_earlier():
    """The cases that ran before WIDE_CLASS: (model, dtype, size, batch) of the one-GPU audit and the full audits."""
    from tests.test_gpu_launch_audit import AUDIT_CASES
    return list(AUDIT_CASES) + list(WIDE_FULL)


def wide_class_cases(table=None):
    return [(m, d, s, b) for (m, d, s), bs in (WIDE_CLASS if table is None else table).items() for b in bs]


def wide_audited(cases, family):
    """The classes of a dtype family that the cases' steps launch."""
    out = set()
    for m, d, s, b in cases:
        if FAMILY[d] == family:
            out |= set(wide_classes(m, d, s, b))
    return out


def wide_new_classes(case, table=None):
    """{class: tag}: the classes `case` (one of wide_class_cases) is the first of its family to audit - what it was added for."""
    cases = wide_class_cases(table)
    before = wide_audited(wide_earlier() + cases[:cases.index(case)], FAMILY[case[1]])
    m, d, s, b = case
    return {k: tag for k, tag in wide_classes(m, d, s, b).items() if k not in before}


def wide_reach(family):
    """{class: [(model, size, batch, tag)]} over the family's wide sweep."""
    dtype = 'f32' if family == 'fp32' else 'bf16'
    reach = {}
    for (m, s), batches in WIDE_SWEEP[family].items():
        for B in batches:
            for cls, tag in wide_classes(m, dtype, s, B).items():
                reach.setdefault(cls, []).append((m, s, B, tag))
    return reach


def wide_missing(table=None):
    missing = []
    cases = wide_earlier() + wide_class_cases(table)
    for family in WIDE_SWEEP:
        seen = wide_audited(cases, family)
        for cls, where in wide_reach(family).items():
            if cls not in seen:
                at = {}
                for m, s, B, tag in where:
                    at.setdefault(f"{m} {s}x{s}", []).append(B)
                missing.append(f"{family} class {cls} ({where[0][3]}) reached at " + ', '.join(f"{k} B = {v}" for k, v in at.items()))
    return missing


@pytest.mark.skipif(not HAVE_LIB, reason="library not built")
def test_f16_and_bf16_plan_alike_over_the_wide_sweeps():
    """One 16-bit dtype per case suffices: the class sets are equal at every point of the 16-bit sweeps, CycleGAN included."""
    for (m, s), batches in WIDE_SWEEP['16-bit'].items():
        for B in batches:
            assert set(wide_classes(m, 'f16', s, B)) == set(wide_classes(m, 'bf16', s, B)), (m, s, B)
            assert set(plan_classes(m, B, s, L.F16)) == set(plan_classes(m, B, s, L.BF16)), (m, s, B)


@pytest.mark.skipif(not HAVE_LIB, reason="library not built")
def test_wide_cases_reach_every_plan_class_of_the_wide_sweeps():
    for family, sweep in WIDE_SWEEP.items():
        reach = wide_reach(family)
        old = wide_audited(wide_earlier()[:-len(WIDE_FULL)], family)
        print(f"{family}: {len(reach)} classes, {len(set(reach) - old)} of them launched by no case of tests/test_gpu_launch_audit.py")
        for (m, s), batches in sweep.items():
            own = {c for c, where in reach.items() if any(w[:2] == (m, s) for w in where)}
            print(f"  {m} {s}x{s} B = {batches[0]}..{batches[-1]}: {len(own)} classes, {len(own - old)} not launched")
    missing = wide_missing()
    assert not missing, "plan classes of the wide sweeps that no audit case reaches:\n" + "\n".join(missing)
    # the wide sweeps contain the narrow one, and every case lies inside its sweep
    for (m, s), batches in SWEEP.items():
        assert set(batches) <= set(WIDE_SWEEP['16-bit'][(m, s)])
    for m, d, s, b in wide_class_cases() + list(WIDE_FULL):
        assert b in WIDE_SWEEP[FAMILY[d]][(m, s)], (m, d, s, b)
    for case in wide_class_cases():
        new = wide_new_classes(case)
        print(f"  {case}: added for {sorted(new.items(), key=str)}")
        assert new, f"{case} audits no class that an earlier case has not audited"
    # the test can fail: without the largest batch of a key a class is left out, and the message names the batches that reach it
    for key, batches in WIDE_CLASS.items():
        less = wide_missing({**WIDE_CLASS, key: batches[:-1]})
        assert less and all(f"{FAMILY[key[1]]} class" in msg and f"{key[0]} {key[2]}x{key[2]} B = " in msg for msg in less), (key, less)
        assert all(batches[-1] in [int(v) for v in msg.split(f"{key[0]} {key[2]}x{key[2]} B = [")[1].split(']')[0].split(',')] for msg in less), (key, less)
        # and no smaller batch of that key does what its largest one does
        for b in range(WIDE_SWEEP[FAMILY[key[1]]][key[0], key[2]][0], batches[-1]):
            assert wide_missing({**WIDE_CLASS, key: batches[:-1] + (b,)}), (key, b)


# ---- plan coverage of the inference forward ------------------------------------------------------------------------------------
# tests/test_gpu_eval_audit.py's bf16 cases: (network, size) -> batches.  The smallest sets that reach every class of the sweep
# below (the batches people use: tools/bench_infer.py reports 16 and 64, --batch-size sets the predict batch, infer_tiled runs one
# call per tile count and one for the last chunk).
EVAL_AUDITED = {('generator', 256): (1, 8, 33, 49), ('generator', 512): (2, 9, 11),
                ('discriminator', 256): (4, 11, 18, 33), ('discriminator', 512): (1, 5, 6, 9)}
EVAL_SWEEP = {('generator', 256): range(1, 65), ('generator', 512): range(1, 17),
              ('discriminator', 256): range(1, 65), ('discriminator', 512): range(1, 17)}


def eval_launches(net, B, S, dt=L.BF16, channels=1):
    """[(tag, op, plan info, tap-shared, bias present, activation, sub-form)] of the convolution launches of one eval forward, with
    the views (channel slices of the concat buffers, their real pitches), bias and activation that nets.GenEvalCall /
    nets.DiscEvalCall give them at `channels` image channels: no statistics, no fused epilogue requests.  sub-form: () for the tiled
    GEMM, ('one-kernel',) or ('two-launch',) for the streaming kernels (launch_audit.conv_class)."""
    lib = L.load()
    out = []

    def V(n, h, c, pitch=None):
        return L.GanTensor(16, n, h, h, c, pitch or c)

    def conv(tag, op, x, y, stride=2, bias=True, act=L.ACT_NONE, y_f32=0):
        d = L.GanConvDesc(dt, stride, x, y, 16, y.c, 16 if bias else None, act, 0.3, y_f32, 16, 1 << 40, None, 0, 0, None, None)
        info = (C.c_int32 * 5)()
        assert lib.gan_conv_plan_info(C.byref(d), op, info) == 0, tag
        out.append((tag, op, list(info), lib.gan_conv_tap_shared(C.byref(d), op), bool(bias), act, A.conv_class(d, op)[8:]))

    if net == 'generator':
        hs = [S >> (i + 1) for i in range(8)]
        pitch = [G_UP[j] + G_DOWN[6 - j] for j in range(7)]                  # concat buffer j: [up j | down 6-j]

        def a_down(i):
            return V(B, hs[i], 512) if i == 7 else V(B, hs[i], G_DOWN[i], pitch[6 - i])
        conv("G.down0", 0, V(B, S, 8), a_down(0), bias=False, act=L.ACT_LRELU)
        for i in range(1, 8):
            conv(f"G.down{i}", 0, a_down(i - 1), a_down(i), act=L.ACT_LRELU)
        for j in range(7):
            x = V(B, hs[7], 512) if j == 0 else V(B, hs[7 - j], pitch[j - 1])
            conv(f"G.up{j}", 2, x, V(B, hs[6 - j], G_UP[j], pitch[j]), act=L.ACT_RELU)
        conv("G.last", 2, V(B, hs[0], pitch[6]), V(B, S, channels, 8), act=L.ACT_TANH)
    else:
        s1, s2, s3 = S // 2, S // 4, S // 8
        s4, s5 = s3 - 1, s3 - 2
        conv("D.down0", 0, V(B, S, 8), V(B, s1, 64), bias=False, act=L.ACT_LRELU)
        conv("D.down1", 0, V(B, s1, 64), V(B, s2, 128), act=L.ACT_LRELU)
        conv("D.down2", 0, V(B, s2, 128), V(B, s3, 256), act=L.ACT_LRELU)
        conv("D.conv", 0, V(B, s3, 256), V(B, s4, 512), 1, act=L.ACT_LRELU)
        conv("D.last", 0, V(B, s4, 512), V(B, s5, 1), 1, y_f32=1)
    return out


def eval_plan_classes(net, B, S, dt=L.BF16, channels=1):
    """{class: tag}: the class key of plan_classes (op, tile, split or not, parity form, statistics, tap sharing) plus (bias
    present, activation) and, for the streaming kernels, their sub-form."""
    return {('conv', op, info[0], info[1], info[2] > 1, info[3], '-', ts, bias, act) + sub: tag
            for tag, op, info, ts, bias, act, sub in reversed(eval_launches(net, B, S, dt, channels))}


def eval_plan_strings(net, B, S, dt=L.BF16, channels=1):
    """The launches as tests/test_gpu_eval_audit.py names what it recorded: check_conv's plan string + bias + activation.  The GPU
    test fails if the set it saw differs from this one, so a change in nets.py cannot leave the table above behind."""
    return {f"op{op} tile {info[0]}x{info[1]} split {info[2]} par {info[3]} stats {info[4]} ts {ts} bias {int(bias)} act {act}"
            for tag, op, info, ts, bias, act, sub in eval_launches(net, B, S, dt, channels)}


def eval_missing(audited):
    missing = []
    for key, batches in EVAL_SWEEP.items():
        net, S = key
        reach = {}
        for B in batches:
            for cls, tag in eval_plan_classes(net, B, S).items():
                reach.setdefault(cls, []).append((B, tag))
        seen = set()
        for B in audited[key]:
            seen |= set(eval_plan_classes(net, B, S))
        for cls, where in reach.items():
            if cls not in seen:
                missing.append(f"{net} {S}x{S}: class {cls} ({where[0][1]}) reached at B = {[b for b, _ in where]}, audited {audited[key]}")
    return missing


@pytest.mark.skipif(not HAVE_LIB, reason="library not built")
def test_eval_audited_batches_reach_every_plan_class():
    missing = eval_missing(EVAL_AUDITED)
    assert not missing, "plan classes of the eval forward no audited batch reaches:\n" + "\n".join(missing)
    # the test can fail: without its largest batch a set leaves a class out, and the message names the batches that reach it
    for key, batches in EVAL_AUDITED.items():
        less = eval_missing({**EVAL_AUDITED, key: batches[:-1]})
        assert less and all(f"{key[0]} {key[1]}x" in m and str(batches[-1]) in m for m in less), (key, less)


# ---- the gates must be able to fail ----------------------------------------------------------------------------------------------
ROUND = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16}
PCOLS = 64            # channels per parity block of columns of a parity-form tile (conv_gemm.hip: BN / 4 of the 128x256 family)


def _case(op, dt, seed=5):
    """2 x 8 x 8 input, 64 -> 256 channels, stored operands (values of the storage type), calibrated-style bias (non-zero,
    different from channel to channel, both signs) -> x, w [16][256][64], bias, all fp64."""
    g = torch.Generator().manual_seed(seed + op)
    x = (torch.randint(0, 256, (2, 8, 8, 64), generator=g).float() / 127.5 - 1.0).to(ROUND[dt]).double()
    w = (0.03 * torch.randn((16, 256, 64), generator=g)).to(ROUND[dt]).double()
    bias = (0.2 * torch.randn(256, generator=g) + 0.3 * (torch.rand(256, generator=g) - 0.5)).float().double()
    return x, w, bias


def _model(op, x, w, bias, act, slope, dt, variant=None):
    """float32 model of one launch: fp32 accumulation of the products of the stored operands, + bias, activation, one rounding to
    storage.  variant: what a wrong kernel would compute instead."""
    f = torch.float32
    acc = A.conv_ref(op, x.to(f), w.to(f), 2)                        # [n, h, w, 256], fp32 sums
    b = bias.to(f)
    bb = b.expand_as(acc)
    if variant == 'bias rotated by one channel':
        bb = torch.roll(b, 1).expand_as(acc)
    elif variant == 'bias rotated by one 4-channel group':
        bb = torch.roll(b, 4).expand_as(acc)
    elif variant == 'bias dropped on columns >= 128':
        bb = torch.where(torch.arange(256) < 128, b, torch.zeros_like(b)).expand_as(acc)
    elif variant == "bias of the other parity's column":             # the column index taken without % PCOLS (transposed form)
        bb = torch.empty_like(acc)
        for par in range(4):
            idx = torch.arange(256) + par * PCOLS
            bp = torch.where(idx < 256, b[idx.clamp(max=255)], torch.zeros_like(b))
            bb[:, par >> 1::2, par & 1::2, :] = bp
    a_, sl = act, slope
    if variant == 'ReLU for LeakyReLU':
        a_ = L.ACT_RELU
    elif variant == 'slope 0.2 for 0.3':
        sl = 0.2
    if variant == 'activation before the bias':
        out = A.act_f(acc, a_, sl) + bb
    else:
        out = A.act_f(acc + bb, a_, sl)
    return out.to(f).to(ROUND[dt])


CONV_VARIANTS = ['bias rotated by one channel', 'bias rotated by one 4-channel group', 'bias dropped on columns >= 128',
                 'activation before the bias', 'ReLU for LeakyReLU', 'slope 0.2 for 0.3']


@pytest.mark.parametrize('dt', [L.BF16, L.F16, L.F32], ids=['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('op', [0, 2], ids=['conv_fwd', 'convT_fwd'])
def test_conv_gate_passes_the_float32_model_and_rejects_wrong_epilogues(op, dt):
    x, w, bias = _case(op, dt)
    ref, eacc = A.conv_pre(op, x, w, bias, 2)
    out, gate = A.y_gate(ref, eacc, L.ACT_LRELU, 0.3, dt)
    assert tuple(out.shape) == ((2, 4, 4, 256) if op == 0 else (2, 16, 16, 256))
    assert float((ref < 0).double().mean()) > 0.2 and float((ref > 0).double().mean()) > 0.2       # both sides of the kink in use
    good = A.ratio(_model(op, x, w, bias, L.ACT_LRELU, 0.3, dt), out, gate)
    print(f"conv op{op} dtype {dt}: float32 model worst error / gate {good:.3f}")
    assert good <= 1.0
    if dt != L.F32:
        assert good <= 0.55                      # half an ulp of the rounding to storage against a gate of one
    variants = CONV_VARIANTS + (["bias of the other parity's column"] if op == 2 else [])
    for v in variants:
        r = A.ratio(_model(op, x, w, bias, L.ACT_LRELU, 0.3, dt, v), out, gate)
        print(f"  {v}: {r:.1f}")
        assert r >= 2.0, (v, r)
    # ReLU layers (up0-6): LeakyReLU in their place, and the bias variants again
    out, gate = A.y_gate(ref, eacc, L.ACT_RELU, 0.3, dt)
    assert A.ratio(_model(op, x, w, bias, L.ACT_RELU, 0.3, dt), out, gate) <= 1.0
    assert A.ratio(_model(op, x, w, bias, L.ACT_LRELU, 0.3, dt), out, gate) >= 2.0
    for v in variants[:4] + variants[6:]:
        assert A.ratio(_model(op, x, w, bias, L.ACT_RELU, 0.3, dt, v), out, gate) >= 2.0, v


def _fold_inputs(A_, B_, transposed, seed):
    rng = np.random.default_rng(seed)
    co = B_ if transposed else A_
    master = (0.05 * rng.standard_normal((16, A_, B_))).astype(np.float32)
    gamma = (rng.uniform(0.6, 1.4, co) * rng.choice([-1.0, 1.0], co, p=[0.2, 0.8])).astype(np.float32)
    beta = rng.normal(0.0, 0.2, co).astype(np.float32)
    mean = rng.normal(0.0, 0.5, co).astype(np.float32)
    var = rng.uniform(0.01, 3.0, co).astype(np.float32)
    return master, gamma, beta, mean, var


@pytest.mark.parametrize('dt', [L.BF16, L.F16, L.F32], ids=['bf16', 'f16', 'f32'])
def test_fold_reference_is_the_numpy_fold_and_rejects_wrong_folds(dt):
    from oracle import gan_oracle as O
    from tests.inference_ref import _np_fold
    tdt = ROUND[dt]
    for k, (A_, B_, tr) in enumerate([(64, 256, 1), (256, 64, 0), (12, 70, 1), (96, 20, 0), (64, 64, 1)]):
        master, gamma, beta, mean, var = _fold_inputs(A_, B_, tr, 20 + k)
        t = [torch.from_numpy(a) for a in (master, gamma, beta, mean, var)]
        bias, nk = A.fold_ref(*t, O.BN_EPS, tr, tdt)
        co, ci = (B_, A_) if tr else (A_, B_)
        assert tuple(nk.shape) == (16, co, (ci + 7) // 8 * 8) and not nk[..., ci:].any()
        s_np, b_np, w_np = _np_fold(master, gamma, beta, mean, var, tr)          # tests/inference_ref.py: numpy, one operation at a time
        assert A.bit_equal(bias, torch.from_numpy(b_np)) == 0.0
        assert A.bit_equal(nk[..., :ci], torch.from_numpy(w_np).to(tdt)) == 0.0
        # wrong folds: each must differ in at least one bit (check_fold's items are bit equality: any difference is outside)
        eps = np.float32(O.BN_EPS)
        s_eps = gamma * (np.float32(1.0) / (np.sqrt(var) + eps))                                 # eps outside the root
        w3 = master.transpose(0, 2, 1) if tr else master
        assert A.bit_equal(bias, torch.from_numpy(beta - mean * s_eps)) == math.inf
        assert A.bit_equal(nk[..., :ci], torch.from_numpy(w3 * s_eps[None, :, None]).to(tdt)) == math.inf
        assert A.bit_equal(bias, torch.from_numpy(beta - mean)) == math.inf                      # the moving mean left unscaled by s
        swapped = master if tr else master.transpose(0, 2, 1)                                    # the other layout, same bytes count
        if A_ == B_:
            wrong = torch.from_numpy(swapped * s_np[None, :, None]).to(tdt)
            assert A.bit_equal(nk[..., :ci], wrong) == math.inf
        elif ci % 8 == 0:
            wrong = torch.from_numpy(np.ascontiguousarray(swapped)).to(tdt).reshape(-1)          # what the buffer would hold, read flat
            assert A.bit_equal(nk.reshape(-1), wrong) == math.inf


# ---- plan coverage of the data-parallel step ---------------------------------------------------------------------------------------
# tests/test_gpu_ddp_audit.py's cases: name -> (model, dtype, wgrad table of plan_classes, per-rank batches), all 256x256 (the
# smallest size the 8-level generator accepts).  A case's wgrad launches are the table's at its batch; the batches of all cases that
# share a table must together reach every wgrad class of per-rank batches 1..8 (DDP_SWEEP).  The sweep's answer: batches 1..3 reach
# five of the six classes of every table, and the sixth - the 256 x 256 ping-pong kernel, which only D's stride-1 layer at 2B >= 8
# images takes - needs B >= 4; B = 4 alone reaches all six.  So one case per table runs B = 4 (no 512x512 case: nothing is left for
# it) and every other case, which adds no class, the cheapest batch, 1.
DDP_CASES = {
    'pix2pix-bf16-bucketed-wire-direct': ('pix2pix', 'bf16', 'direct', (4,)),
    'pix2pix-bf16-bucketed-wire-pack': ('pix2pix', 'bf16', 'plain', (1,)),
    'pix2pix-bf16-bucketed-fp32-wire': ('pix2pix', 'bf16', 'plain', (4,)),
    'pix2pix-f16-phased': ('pix2pix', 'f16', 'plain', (1,)),
    'cyclegan-bf16-phased-wire': ('cyclegan', 'bf16', 'plain', (4,)),
    'pix2pix-bf16-phased-wire': ('pix2pix', 'bf16', 'plain', (1,)),
}
DDP_SWEEP = range(1, 9)
DDP_DT = {'bf16': L.BF16, 'f16': L.F16}


def ddp_audited(cases=None):
    """(model, table) -> the batches of the 16-bit cases that run it."""
    out = {}
    for model, dtype, tab, batches in (cases or DDP_CASES).values():
        out[(model, tab)] = tuple(sorted(set(out.get((model, tab), ()) + tuple(batches))))
    return out


DDP_AUDITED = ddp_audited()


def ddp_wgrad_classes(model, tab, B, dt=L.BF16):
    return {k: v for k, v in plan_classes(model, B, 256, dt, ddp=tab).items() if k[0] == 'wgrad'}


def ddp_wgrad_plan_strings(model, dtype, tab, B):
    """The wgrad launches of a data-parallel capture as launch_audit.check_wgrad names them (the GPU cases compare)."""
    s = set()
    plan_classes(model, B, 256, DDP_DT[dtype], ddp=tab, strings=s)
    return s


def ddp_missing(audited):
    missing = []
    for (model, tab), batches in audited.items():
        reach = {}
        for B in DDP_SWEEP:
            for cls, tag in ddp_wgrad_classes(model, tab, B).items():
                reach.setdefault(cls, []).append((B, tag))
        seen = set()
        for B in batches:
            seen |= set(ddp_wgrad_classes(model, tab, B))
        for cls, where in reach.items():
            if cls not in seen:
                missing.append(f"{model} {tab} 256x256: class {cls} ({where[0][1]}) reached at B = {[b for b, _ in where]}, audited {batches}")
    return missing


@pytest.mark.skipif(not HAVE_LIB, reason="library not built")
def test_ddp_audited_batches_reach_every_plan_class():
    assert {(m, t) for m, _, t, _ in DDP_CASES.values()} == set(DDP_AUDITED)
    missing = ddp_missing(DDP_AUDITED)
    assert not missing, "wgrad classes of the data-parallel step no audited batch reaches:\n" + "\n".join(missing)
    # f16 plans its wgrads as bf16 does (the planner only tells 16-bit from fp32): the f16 case adds no class of its own
    for B in DDP_SWEEP:
        assert set(ddp_wgrad_classes('pix2pix', 'plain', B, L.F16)) == set(ddp_wgrad_classes('pix2pix', 'plain', B, L.BF16)), B
    # the direct table has launches that write the wire format and launches that cannot (tap-folded first / last layers, the logits)
    wires = {k[5] for B in DDP_AUDITED[('pix2pix', 'direct')] for k in ddp_wgrad_classes('pix2pix', 'direct', B)}
    assert wires == {0, 1}
    # the test can fail: without its largest batch a set leaves a class out, and the message names the batches that reach it; and
    # no smaller batch than that one would do
    for key, batches in DDP_AUDITED.items():
        less = ddp_missing({key: batches[:-1]})
        assert less and all(f"{key[0]} {key[1]} 256x" in m and str(batches[-1]) in m for m in less), (key, less)
        assert all(ddp_missing({key: (b,)}) for b in range(1, batches[-1])), key


# ---- the data-parallel gates must be able to fail ------------------------------------------------------------------------------------
# A numpy float32 model of what the bucketed step does to ONE flat buffer: two kernels (64 -> 128 channels, small tensor 2 x 8 x 8)
# whose wgrad launches write the bf16 wire format themselves (split-K in 4 slabs, fp32 sums, round to nearest even), a vector of 100
# elements (padded to ALIGN) that gan_grad_pack casts, then Adam from the wire with grad_scale = 1/2 - put through the very objects
# the GPU audit uses (launch_audit.WireAudit, wire_gate, rounding_bias, adam_end_ratios).
ALIGN = 64
KN = 16 * 64 * 128
VEC, VEC_PAD = 100, 128
LAYOUT = {'k0.kernel': (0, (4, 4, 64, 128)), 'k1.kernel': (KN, (4, 4, 64, 128)), 'v.gamma': (2 * KN, (VEC,))}
TOTAL = 2 * KN + VEC_PAD
DDP_VARIANTS = ['truncation instead of RNE', 'wire written one 4-element group late', "wire written at the neighbouring kernel's offset",
                'one split-K slab dropped', 'grad_scale 1', 'grad_scale 1/4', 'Adam reads the stale fp32 buffer for one kernel',
                'a kernel missing from its segment', 'a kernel updated twice', 'pack range stops ALIGN short',
                'pack range overlaps a direct kernel']


class _FlatSet:
    ALIGN = ALIGN
    entries, total, vec_start = LAYOUT, TOTAL, 2 * KN

    def __init__(self, grad):
        self.grad = grad


class _FlatNet:
    def __init__(self, grad):
        self.params = _FlatSet(grad)


class _FlatStep:
    def __init__(self, grad):
        self._nets = (_FlatNet(grad),)

    def nets(self):
        return self._nets


class _FlatSync:
    def __init__(self):
        self.wire = [torch.zeros(TOTAL, dtype=torch.bfloat16)]


def _bf16_trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _ddp_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    big = (torch.randint(0, 256, (2, 16, 16, 64), generator=g).float() / 127.5 - 1.0).to(torch.bfloat16)
    small = (0.05 * torch.randn((2, 8, 8, 128), generator=g)).to(torch.bfloat16)
    return big, small


def _wgrad_f32(big, small, drop_slab=False):
    """fp32 model of a split launch: 4 slabs over the 128 output positions, each an fp32 GEMM, summed in fp32."""
    cols = F_unfold(big.float())                                     # [M = 128, 16 * 64]
    sm = small.float().reshape(-1, 128)
    out = torch.zeros((16 * 64, 128), dtype=torch.float32)
    for k in range(1 if drop_slab else 0, 4):
        sl = slice(32 * k, 32 * k + 32)
        out = out + cols[sl].t() @ sm[sl]
    return out.reshape(-1)


def F_unfold(big):
    """[n, 16, 16, c] -> [n * 8 * 8, 16 taps * c]: the stride-2, pad-1, 4 x 4 patches, tap-major as dw[tap][big channel]."""
    n, h, w, c = big.shape
    p = torch.nn.functional.unfold(A.nchw(big), kernel_size=4, stride=2, padding=1)          # [n, c * 16, 64]
    return p.reshape(n, c, 16, 64).permute(0, 3, 2, 1).reshape(n * 64, 16 * c)


def _ddp_model(variant=None):
    """Run the model (or a wrong variant) through the audit's objects -> {item: worst error / gate}."""
    from tests import elementwise_ref as E
    g = torch.Generator().manual_seed(23)
    grad = torch.zeros(TOTAL)                                        # fp32 gradient buffer: the direct kernels leave it at zero
    grad[2 * KN:2 * KN + VEC] = 0.3 * torch.randn(VEC, generator=g)
    sync = _FlatSync()
    wa = A.WireAudit(_FlatStep(grad), sync)
    wa.fill()
    wire = sync.wire[0]
    res = {}

    def note(d):
        for k, v in d.items():
            res[k] = max(res.get(k, 0.0), v)
    ops = [_ddp_inputs(31), _ddp_inputs(32)]
    for k, (big, small) in enumerate(ops):                           # the two direct wgrad launches
        acc = _wgrad_f32(big, small, drop_slab=(variant == 'one split-K slab dropped' and k == 0))
        out = _bf16_trunc(acc) if variant == 'truncation instead of RNE' else acc.to(torch.bfloat16)
        lo = k * KN
        at = lo
        if k == 0 and variant == 'wire written one 4-element group late':
            at = lo + 4
        if k == 0 and variant == "wire written at the neighbouring kernel's offset":
            at = KN
        w0 = wa.snapshot()
        wire[at:at + KN] = out
        note(wa.written(w0, 0, lo, lo + KN))
        ref = A.wgrad_ref(big.double(), small.double(), 2, 64, 128).reshape(-1)
        eg = A.wgrad_acc_bound(big.double(), small.double(), 64, 128)
        got = wire[lo:lo + KN].clone()
        note({'wire': A.ratio(got, ref, A.wire_gate(ref, eg)), 'wire rounding bias': A.rounding_bias(got, ref)})
    lo, hi = 2 * KN, TOTAL                                           # gan_grad_pack: the rest of the bucket
    if variant == 'pack range stops ALIGN short':
        hi -= ALIGN
    if variant == 'pack range overlaps a direct kernel':
        lo -= ALIGN
    w0 = wa.snapshot()
    wire[lo:hi] = grad[lo:hi].to(torch.bfloat16)
    note(wa.written(w0, 0, lo, hi))
    res['coverage'] = math.inf if wa.coverage() else 0.0
    # Adam of the whole buffer from the wire, grad_scale = 1 / world
    p0 = 0.02 * torch.randn(TOTAL, generator=g)
    m0 = 1e-4 * torch.randn(TOTAL, generator=g)
    v0 = 1e-8 * torch.rand(TOTAL, generator=g) + 1e-10
    lr_t = float(E.lr_t_model(2e-4, 0.5, 0.999, 1))
    gs = {'grad_scale 1': 1.0, 'grad_scale 1/4': 0.25}.get(variant, 0.5)
    src = wire.float().numpy()
    if variant == 'Adam reads the stale fp32 buffer for one kernel':
        src = src.copy()
        src[KN:2 * KN] = grad[KN:2 * KN].numpy()
    with np.errstate(invalid='ignore'):          # (a sentinel left in the wire is a NaN: the variant is meant to show it)
        p1, m1, v1 = E.adam_model(p0.numpy(), m0.numpy(), v0.numpy(), src, lr_t, gs)
    if variant == 'a kernel missing from its segment':
        for a, b in ((p1, p0), (m1, m0), (v1, v0)):
            a[KN:2 * KN] = b.numpy()[KN:2 * KN]
    if variant == 'a kernel updated twice':
        q = E.adam_model(p1[:KN], m1[:KN], v1[:KN], src[:KN], lr_t, gs)
        for a, b in zip((p1, m1, v1), q):
            a[:KN] = b
    real = torch.zeros(TOTAL, dtype=torch.bool)
    for o, shape in LAYOUT.values():
        real[o:o + int(np.prod(shape))] = True
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a))[real]
    note(A.adam_end_ratios(p0[real], m0[real], v0[real], wire.float()[real], 0.5, lr_t, f(p1), f(m1), f(v1)))
    return res


def test_ddp_gates_pass_the_float32_model_and_reject_wrong_variants():
    good = _ddp_model()
    print("data-parallel float32 model, worst error / gate: " + ', '.join(f"{k} {v:.3f}" for k, v in good.items()))
    assert all(v <= 0.5 for v in good.values()), good
    smallest = {}
    for v in DDP_VARIANTS:
        r = _ddp_model(v)
        out = {k: x for k, x in r.items() if x >= 2.0}
        print(f"  {v}: " + (', '.join(f"{k} {x:.1f}" for k, x in out.items()) or f"NOT SEEN ({r})"))
        assert out, (v, r)
        smallest[v] = max(out.values())
    worst = min(smallest, key=smallest.get)
    print(f"smallest ratio of a wrong variant: {smallest[worst]:.1f} ({worst})")
    # truncation: the per-element gate of a stored 16-bit value is one ulp and passes it - only the rounding-bias item (and, for
    # gan_grad_pack, the bit equality of check_pack_range) sees it
    t = _ddp_model('truncation instead of RNE')
    assert t['wire'] <= 1.0 and t['wire rounding bias'] >= 2.0


# ---- RGB steps (channels = 3): plan coverage --------------------------------------------------------------------------------------
# tests/test_gpu_rgb_audit.py's cases: (model, size) -> batches of the one-GPU training steps, (network, size) -> batches of the eval
# forwards.  At channels = 3 the image-side launches leave the one-kernel thin-N form (thin.hip: y.c <= 2) for conv_thin_n_kernel +
# conv_thin_col2im_kernel; the sweep below (the one of SWEEP: B = 1..16 at 256x256, 1..8 at 512x512) asks which batches the classes
# WITH A THIN OPERAND need - every other class is one the channels = 1 audit covers at the same batch (asserted below).
RGB = 3
RGB_AUDITED = {('pix2pix', 256): (1, 9), ('pix2pix', 512): (1,), ('cyclegan', 256): (1,)}
RGB_SWEEP = SWEEP
RGB_EVAL_AUDITED = {('generator', 256): (1, 9), ('discriminator', 256): (1, 9)}
RGB_EVAL_SWEEP = {('generator', 256): range(1, 17), ('discriminator', 256): range(1, 17)}


def rgb_thin_classes(model, B, S):
    thin = set()
    plan_classes(model, B, S, channels=RGB, thin=thin)
    return thin


def rgb_missing(audited):
    missing = []
    for key, batches in RGB_SWEEP.items():
        model, S = key
        reach = {}
        for B in batches:
            for cls in rgb_thin_classes(model, B, S):
                reach.setdefault(cls, []).append(B)
        seen = set()
        for B in audited[key]:
            seen |= rgb_thin_classes(model, B, S)
        for cls, where in reach.items():
            if cls not in seen:
                missing.append(f"{model} {S}x{S} channels 3: thin class {cls} reached at B = {where}, audited {audited[key]}")
    return missing


@pytest.mark.skipif(not HAVE_LIB, reason="library not built")
def test_rgb_audited_batches_reach_every_thin_plan_class():
    missing = rgb_missing(RGB_AUDITED)
    assert not missing, "thin plan classes at channels = 3 that no RGB case reaches:\n" + "\n".join(missing)
    for key, sweep in RGB_SWEEP.items():
        model, S = key
        for B in sweep:
            thin3, thin1 = set(), set()
            c3 = plan_classes(model, B, S, channels=RGB, thin=thin3)
            c1 = plan_classes(model, B, S, thin=thin1)
            # the launches without a thin operand do not know the image's channel count: same classes as at channels = 1
            assert set(c3) - thin3 == set(c1) - thin1, (key, B)
            # every thin-N launch at channels = 1 is the one-kernel form (no existing class splits); at 3 the image-side ones are not
            assert not any(k[-1] == 'two-launch' for k in c1), (key, B)
            # (a class carries the tag of its first launch: CycleGAN's G.down0 dx dgrad and D.down0 dx dgrad are one class)
            two = {(k[1], c3[k]) for k in c3 if k[-1] == 'two-launch'}
            assert two == {(2, "G.last fwd"), (1, "G.down0 dx dgrad" if model == 'cyclegan' else "D.down0 dx dgrad")}, (key, B, two)
    # the eval forwards: the head is the only launch that changes (two-launch form with bias + tanh)
    for key, sweep in RGB_EVAL_SWEEP.items():
        net, S = key
        reach = {}
        for B in sweep:
            for cls, tag in eval_plan_classes(net, B, S, channels=RGB).items():
                if cls[2] == 0:
                    reach.setdefault(cls, []).append(B)
        seen = set()
        for B in RGB_EVAL_AUDITED[key]:
            seen |= set(eval_plan_classes(net, B, S, channels=RGB))
        gone = {cls: bs for cls, bs in reach.items() if cls not in seen}
        assert not gone, f"eval {net} channels 3: streaming-kernel classes {gone} not reached by {RGB_EVAL_AUDITED[key]}"
    assert any(k[-1] == 'two-launch' and k[8:10] == (True, L.ACT_TANH) for k in eval_plan_classes('generator', 1, 256, channels=RGB))
    # the test can fail: a case list without a model's batches names them
    less = rgb_missing({**RGB_AUDITED, ('cyclegan', 256): ()})
    assert less and all('cyclegan 256x256' in m for m in less)


def test_thin_n_grid_cap_is_first_exceeded_at_batch_9():
    """conv_thin_n_kernel: tiles of 16 pixels, 4 per workgroup, grid capped at 2,048 workgroups (thin.hip, thin_launch).  The head
    reads 128 x 128 pixels per image at 256 x 256: tiles = 1024 B, workgroups 256 B > 2048 iff B > 8.  At B = 9 the second grid-stride
    trip is ragged: 9,216 tiles over 8,192 waves."""
    def groups(B, h):
        return (B * h * h + 15) // 16 // 4
    assert [B for B in range(1, 17) if groups(B, 128) > 2048][0] == 9
    assert groups(9, 128) * 4 - 2048 * 4 == 1024                     # 1,024 of 8,192 waves take a second tile
    assert groups(1, 256) == 1024                                    # 512 x 512, B = 1: within one trip
    assert 9 in RGB_AUDITED[('pix2pix', 256)] and 9 in RGB_EVAL_AUDITED[('generator', 256)]


# ---- the RGB gates must be able to fail -----------------------------------------------------------------------------------------
# A numpy float32 model of the two-launch thin-N convolution (thin.hip): Z[pixel][c][tap] = x[pixel, :] . W[tap][c][:] in fp32, then
# per output pixel the col2im gather of the valid taps (the parity table y[2g + p] = sum_a x[g + p - a] w[1 - p + 2a], or the stride
# table y[g] = sum_a x[g S - 1 + a] w[a]), bias, activation and ONE rounding, stored at channel c of the view's 8-channel pixel.
# Smallest shape with all four borders and both parities: 1 x 8 x 8 source pixels, 64 -> 3 channels.
RGB_CO, RGB_CI, RGB_H = 3, 64, 8
RGB_CONV_VARIANTS = ['ky / kx swapped', 'tap table of the other parity on the last row / column', 'channel c gathers Z of c + 1',
                     'bias rotated by one channel', 'last real channel dropped', 'stored at c of a 3-pitch',
                     'weight rows [0, 3) for [3, 6)']
SENT = {L.BF16: 0x7FA5, L.F16: 0x7E55}        # NaN patterns no kernel produces: what the pad channels / unwritten outputs would keep


def _rgb_case(dt, seed, rows=RGB_CO):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(0, 256, (1, RGB_H, RGB_H, RGB_CI), generator=g).float() / 127.5 - 1.0).to(ROUND[dt]).double()
    w = (0.03 * torch.randn((16, rows, RGB_CI), generator=g)).to(ROUND[dt]).double()
    bias = (0.2 * torch.randn(RGB_CO, generator=g) + 0.1).float().double()
    return x, w, bias


def _thin_n_model(x, w, bias, parity, act, dt, variant=None, row0=0):
    """-> raw int16 span of the [1, Ho, Wo] x 8-channel output buffer (pad channels and unwritten elements keep SENT).
    w: [16][w_rows][64], the launch reads rows [row0, row0 + 3) (D's dx dgrad: the pointer advanced by row0 rows)."""
    f = np.float32
    if variant == 'weight rows [0, 3) for [3, 6)':
        row0 = 0
    xs = x.numpy().astype(f).reshape(RGB_H * RGB_H, RGB_CI)
    ws = w.numpy().astype(f)[:, row0:row0 + RGB_CO]                           # [tap][c][ci]
    Z = np.einsum('pi,tci->pct', xs, ws).astype(f).reshape(RGB_H, RGB_H, RGB_CO, 16)
    Ho = 2 * RGB_H if parity else RGB_H - 1
    b = bias.numpy().astype(f)
    if variant == 'bias rotated by one channel':
        b = np.roll(b, 1)
    pitch = 3 if variant == 'stored at c of a 3-pitch' else 8
    raw = np.full(Ho * Ho * 8, SENT[dt], dtype=np.uint16)
    nco = RGB_CO - 1 if variant == 'last real channel dropped' else RGB_CO
    for Y in range(Ho):
        for X in range(Ho):
            if parity:
                py, gy, px, gx = Y & 1, Y >> 1, X & 1, X >> 1
                if variant == 'tap table of the other parity on the last row / column':
                    py, px = (py ^ 1 if Y == Ho - 1 else py), (px ^ 1 if X == Ho - 1 else px)
                ty = [(gy + py - a, 1 - py + 2 * a) for a in range(2)]
                tx = [(gx + px - a, 1 - px + 2 * a) for a in range(2)]
            else:
                ty = [(Y - 1 + a, a) for a in range(4)]
                tx = [(X - 1 + a, a) for a in range(4)]
            acc = np.zeros(RGB_CO, dtype=f)
            for iy, ky in ty:
                if not 0 <= iy < RGB_H:
                    continue
                for ix, kx in tx:
                    if not 0 <= ix < RGB_H:
                        continue
                    tap = kx * 4 + ky if variant == 'ky / kx swapped' else ky * 4 + kx
                    z = Z[iy, ix, :, tap]
                    acc = (acc + (np.roll(z, -1) if variant == 'channel c gathers Z of c + 1' else z)).astype(f)
            v = torch.from_numpy((acc + b).astype(f))
            v = A.act_f(v, act, 0.3).to(ROUND[dt]).view(torch.int16).numpy().view(np.uint16)
            o = (Y * Ho + X) * pitch
            raw[o:o + nco] = v[:nco]
    return torch.from_numpy(raw.view(np.int16).copy()), Ho


def _thin_n_ratios(op, stride, act, dt, use_bias, variant=None, row0=0):
    """The model's output through check_conv's own items: 'y' (y_gate of conv_pre) and 'y untouched outside y.c'."""
    x, w, bias = _rgb_case(dt, 40 + op + stride, rows=RGB_CO + row0)
    parity = stride == 2
    raw, Ho = _thin_n_model(x, w, bias if use_bias else torch.zeros(RGB_CO).double(), parity, act, dt, variant, row0)
    t = L.GanTensor(16, 1, Ho, Ho, RGB_CO, 8)
    span = (Ho * Ho - 1) * 8 + RGB_CO
    y0 = A.View.of_host(torch.full((span,), SENT[dt], dtype=torch.int16).view(ROUND[dt]), t, dt)
    y1 = A.View.of_host(raw[:span].view(ROUND[dt]), t, dt)
    ref, eacc = A.conv_pre(op, x, w[:, row0:row0 + RGB_CO], bias if use_bias else None, stride)
    assert tuple(ref.shape) == (1, Ho, Ho, RGB_CO)
    out, gate = A.y_gate(ref, eacc, act, 0.3, dt)
    return {'y': A.ratio(y1.dense(), out, gate), 'y untouched outside y.c': A.untouched(y0, y1, 0, RGB_CO)}


def _thin_wgrad_ratios(dt, big_c, variant=None):
    """float32 model of a wgrad launch with a thin big side (G.down0 / G.last: 3 of 8 channels, D.down0: 6 of 8): dw[tap][big_c][64]
    through check_wgrad's plain-write item."""
    g = torch.Generator().manual_seed(50 + big_c)
    big = torch.zeros((1, 16, 16, 8))
    big[..., :big_c] = torch.randint(0, 256, (1, 16, 16, big_c), generator=g).float() / 127.5 - 1.0
    big = big.to(ROUND[dt])
    small = (0.05 * torch.randn((1, 8, 8, 64), generator=g)).to(ROUND[dt])
    dw = (F_unfold(big[..., :big_c].float()).t() @ small.float().reshape(-1, 64)).reshape(16, big_c, 64)
    got = torch.zeros(16 * big_c * 64)
    if variant == 'dw rows written with row stride 8':
        rows = (torch.arange(16)[:, None] * 8 + torch.arange(big_c)[None, :]).reshape(-1)
        keep = rows < 16 * big_c                                            # (a kernel would write the rest behind the tensor)
        got.view(16 * big_c, 64)[rows[keep]] = dw.reshape(-1, 64)[keep]
    else:
        got.copy_(dw.reshape(-1))
    ref = A.wgrad_ref(big.double(), small.double(), 2, big_c, 64).reshape(-1)
    eg = A.wgrad_acc_bound(big.double(), small.double(), big_c, 64)
    return {'dw': A.ratio(got, ref, eg + A.ulp(ref, L.F32))}


# (entry point, stride, activation, bias, first weight row): the head, a stride-1 / pad-1 layer of 3 outputs, D's dx dgrad
RGB_FORMS = {'convT_fwd parity + bias + tanh (G.last)': (2, 2, L.ACT_TANH, True, 0),
             'conv_fwd stride 1 pad 1 + bias': (0, 1, L.ACT_NONE, True, 0),
             'conv_dgrad parity, rows [3, 6) of 6 (D.down0 dx dgrad)': (1, 2, L.ACT_NONE, False, 3)}


@pytest.mark.parametrize('dt', [L.BF16, L.F16], ids=['bf16', 'f16'])
def test_rgb_gates_pass_the_float32_model_and_reject_wrong_variants(dt):
    smallest = {}
    for form, (op, stride, act, use_bias, row0) in RGB_FORMS.items():
        good = _thin_n_ratios(op, stride, act, dt, use_bias, None, row0)
        print(f"{form}, dtype {dt}: float32 model worst error / gate " + ', '.join(f"{k} {v:.3f}" for k, v in good.items()))
        assert all(v <= 0.5 for v in good.values()), (form, good)
        for v in RGB_CONV_VARIANTS:
            if v == 'tap table of the other parity on the last row / column' and stride != 2:
                continue                          # (the stride form has one tap table)
            if v == 'bias rotated by one channel' and not use_bias:
                continue
            if v == 'weight rows [0, 3) for [3, 6)' and not row0:
                continue
            r = _thin_n_ratios(op, stride, act, dt, use_bias, v, row0)
            out = {k: x for k, x in r.items() if x >= 2.0}
            print(f"  {v}: " + (', '.join(f"{k} {x:.1f}" for k, x in out.items()) or f"NOT SEEN ({r})"))
            assert out, (form, v, r)
            smallest[v] = min(smallest.get(v, math.inf), max(out.values()))
            if v == 'stored at c of a 3-pitch':
                assert r['y untouched outside y.c'] == math.inf
    assert set(smallest) == set(RGB_CONV_VARIANTS)
    for big_c in (3, 6):
        good = _thin_wgrad_ratios(dt, big_c)
        bad = _thin_wgrad_ratios(dt, big_c, 'dw rows written with row stride 8')
        print(f"wgrad big_c {big_c}, dtype {dt}: float32 model dw {good['dw']:.3f}; dw rows written with row stride 8: {bad['dw']:.1f}")
        assert good['dw'] <= 0.5 and bad['dw'] >= 2.0
        smallest['dw rows written with row stride 8'] = min(smallest.get('dw rows written with row stride 8', math.inf), bad['dw'])
    worst = min(smallest, key=smallest.get)
    print(f"smallest ratio of a wrong variant: {smallest[worst]:.1f} ({worst})")
