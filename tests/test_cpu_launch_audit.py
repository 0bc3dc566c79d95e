"""CPU side of the launch audit (tests/launch_audit.py, tests/test_gpu_launch_audit.py):
  - the audit's fp64 references of the four conv entry points and of wgrad, decoded from the device weight layout, against the
    oracle's Keras-layout convolutions;
  - plan coverage: the plan class of every convolution / wgrad launch in the table of plan_classes() (the captured one-GPU Pix2Pix
    and CycleGAN steps at channels = 1, see there) at B = 1..16 (256x256) and B = 1..8 (512x512, BASELINE config 4's per-GPU batch),
    from the host-side planners, must be reached by a batch the GPU audit runs.  A planner change that creates a class no audited
    batch reaches fails here and names the batch sizes that reach it."""
import ctypes as C
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
# wgrad scheduling hints that gan_amd/nets.py and gan_amd/steps.py give them in the captured one-GPU step at channels = 1 (the steps
# the GPU audit builds).
G_DOWN = [64, 128, 256, 512, 512, 512, 512, 512]
G_UP = [512, 512, 512, 512, 256, 128, 64]
CH = 1


def T(n, h, c):
    return L.GanTensor(16, n, h, h, c, c)


def plan_classes(model, B, S, dt=L.BF16):
    """{class: label} of every conv / wgrad launch of one captured step.
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
        d = L.GanConvDesc(dt, stride, x, y, 16, w_rows or y.c, 16 if bias else None, act, 0.3, y_f32, 16, 1 << 40,
                          16 if groups else None, groups, 1 << 30, C.addressof(bf) if bf is not None else None,
                          C.addressof(nf) if nf is not None else None)
        assert lib.gan_conv_plan_info(C.byref(d), op, info) == 0, tag
        ts = lib.gan_conv_tap_shared(C.byref(d), op)
        st = ('full' if info[4] == -1 else 'stats' if info[4] > 0 else 'none') if groups else '-'
        out.setdefault(('conv', op, info[0], info[1], info[2] > 1, info[3], st, ts), tag)

    def wgrad(tag, big, small, big_c, small_c, stride, conc):
        d = L.GanWgradDesc(dt, stride, big, small, 16, big_c, small_c, 0, 16, 1 << 40, conc, None)
        assert lib.gan_wgrad_plan_info(C.byref(d), winfo) == 0, tag
        out.setdefault(('wgrad', winfo[0], winfo[1], winfo[2] > 1, winfo[3]), tag)

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
            conv("G.down0 dx dgrad", 1, T(n, hs[0], 64), T(n, S, CH))
        for j, co in enumerate(G_UP):
            h_in = hs[7 - j]
            conv(f"G.up{j} fwd", 2, T(n, h_in, cin_up[j]), T(n, 2 * h_in, co), groups=g, norm_fuse=True)
            cols = G_UP[j - 1] if j > 0 else 512
            conv(f"G.up{j} dgrad", 3, T(n, 2 * h_in, co), T(n, h_in, cin_up[j]), groups=g, norm_fuse=True, bwd=(cols, True, False))
        conv("G.last fwd", 2, T(n, hs[0], 128), T(n, S, CH), act=L.ACT_TANH, bias=True)
        conv("G.last dgrad", 3, T(n, S, 8), T(n, hs[0], 128), groups=g, bwd=(G_UP[6], True, False))

    def generator_wgrads(n, conc):
        cin = 8
        for i, co in enumerate(G_DOWN):
            big_c = CH if i == 0 else G_DOWN[i - 1]
            wgrad(f"G.down{i} wgrad", T(n, S >> i, cin), T(n, hs[i], co), big_c, co, 2, conc)
            cin = co
        for j, co in enumerate(G_UP):
            h_in = hs[7 - j]
            wgrad(f"G.up{j} wgrad", T(n, 2 * h_in, co), T(n, h_in, cin_up[j]), co, cin_up[j], 2, conc)
        wgrad("G.last wgrad", T(n, S, 8), T(n, hs[0], 128), CH, 128, 2, conc)

    s1, s2, s3 = S // 2, S // 4, S // 8
    s4, s5 = s3 - 1, s3 - 2
    d_cin = 2 * CH if model == 'pix2pix' else CH
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
            conv("D.down0 dx dgrad", 1, T(n, s1, 64), T(n, S, CH), w_rows=d_cin)

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
    disc_forward(B, 1)
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
