"""Per-element checks of the loss, Adam, cast, wire-format, mask and weight-layout kernels of gan_amd/csrc/elementwise.hip against
the references and gates of tests/elementwise_ref.py (proven on the CPU by tests/test_cpu_elementwise.py).  Calls go through the
C ABI.  Every case is the smallest shape that reaches its edge (asserted in test_cpu_elementwise.py::test_every_shape_reaches_its_edge);
every output buffer starts as a sentinel (NaN, 0xAA bytes) between two guard regions, and every case asserts that nothing outside
the addressed view changed."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from tests import elementwise_ref as E

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64                  # elements in front of and behind every buffer
WORST = {}                  # table title -> {entry point: {item: worst error / gate}}


@pytest.fixture(scope="module", params=['f32', 'bf16', 'f16'])
def ctx(request):
    from gan_amd.nets import Ctx
    request.addfinalizer(lambda: print('\n' + E.table(WORST.get(request.param, {}), request.param)))
    return Ctx('cuda:0', request.param)


@pytest.fixture(scope="module")
def dev(request):
    """The entry points without a dtype argument: library, device, stream."""
    request.addfinalizer(lambda: print('\n' + E.table(WORST.get('no dtype argument', {}), 'no dtype argument')))
    d = torch.device('cuda:0')
    return types.SimpleNamespace(lib=L.load(), device=d, dtype='no dtype argument', stream=lambda: torch.cuda.current_stream(d).cuda_stream)


def gate(c, name, item, value):
    """Record error / gate under the context's table and assert it."""
    E.note(WORST.setdefault(c.dtype, {}), name, item, value)
    assert value <= 1.0, (name, item, value)


def _int_view(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Guarded:
    """n elements between two guards on the device, everything filled with the sentinel (NaN; 0xAA for bytes; for integers the
    given fill), then `data` copied in.  shift: extra elements in front (a deliberately misaligned start)."""

    def __init__(self, device, n, tdtype=torch.float32, data=None, shift=0, fill=None):
        self.n, self.lo = n, GUARD + shift
        if fill is None:
            fill = 0xAA if tdtype == torch.uint8 else float('nan')
        self.t = torch.full((self.lo + n + GUARD,), fill, dtype=tdtype, device=device)
        if data is not None:
            self.t[self.lo:self.lo + n] = data.reshape(-1).to(device)
        self.ptr = self.t.data_ptr() + self.lo * self.t.element_size()
        self.snap = _int_view(self.t).cpu().clone()

    def host(self):
        return self.t.cpu()[self.lo:self.lo + self.n]

    def changed(self):
        """bool [n]: elements whose bits differ from construction time; asserts the guards kept theirs."""
        ch = _int_view(self.t).cpu() != self.snap
        assert not ch[:self.lo].any() and not ch[self.lo + self.n:].any(), "a guard region was written"
        return ch[self.lo:self.lo + self.n]

    def untouched(self):
        return not self.changed().any()


class View(Guarded):
    """NHWC view of c channels at channel offset c0 of a pitch-wide guarded buffer; the other channels hold the sentinel."""

    def __init__(self, device, shape, pitch, c0, tdtype, data=None):
        n, h, w, c = shape
        self.shape, self.pitch, self.c0, self.rows = shape, pitch, c0, n * h * w
        super().__init__(device, self.rows * pitch, tdtype)
        if data is not None:
            self.t[self.lo:self.lo + self.n].view(self.rows, pitch)[:, c0:c0 + c] = data.reshape(self.rows, c).to(device)
            self.snap = _int_view(self.t).cpu().clone()
        self.tensor = L.GanTensor(self.ptr + c0 * self.t.element_size(), n, h, w, c, pitch)

    def dense(self):
        return self.host().view(self.rows, self.pitch)[:, self.c0:self.c0 + self.shape[3]].contiguous()

    def outside_untouched(self):
        ch = self.changed().view(self.rows, self.pitch).clone()
        ch[:, self.c0:self.c0 + self.shape[3]] = False
        return not ch.any()


def scale_state(c, vals):
    return Guarded(c.device, 4, data=torch.tensor(vals, dtype=torch.float32)) if vals is not None else None


def sync():
    torch.cuda.synchronize()


# ---- losses -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", E.BCE_COUNTS)
def test_bce_logits(ctx, count):
    """gan_bce_logits: gradient per element and loss scalar against their gates; dx null and non-null (pitch 8); loss_accumulate from
    a non-zero loss_out (exactly the fp32 sum of the two stored values); with a scale state the gradient is scaled, the loss not."""
    x = E.logits(count, count)
    xd = Guarded(ctx.device, count, data=torch.from_numpy(x))
    for target in (1.0, 0.0):
        ls_, gs_ = E.bce_args(target)
        for ls in (None, E.LS_ON):
            st = scale_state(ctx, ls)
            ls0 = ls[0] if ls else 1.0
            dx = View(ctx.device, (1, 1, count, 1), 8, 0, ctx.tdtype)
            loss = Guarded(ctx.device, 1, data=torch.tensor([7.25]))
            rc = ctx.lib.gan_bce_logits(xd.ptr, count, target, ls_, 0, loss.ptr, gs_, ctx.dt, dx.ptr, 8, ctx.ws_ptr, st.ptr if st else None,
                                        ctx.stream())
            assert rc == 0
            sync()
            got = float(loss.host()[0])
            for k, v in E.check_bce(x, target, gs_, ls0, ctx.dt, got, dx.dense().reshape(-1), ls_).items():
                gate(ctx, 'gan_bce_logits', f'{k} t={target:g} ls={ls0:g}', v)
            assert dx.outside_untouched() and xd.untouched() and (st is None or st.untouched())
            # dx null, accumulate onto 1.5: the same deterministic loss, added in fp32
            acc = Guarded(ctx.device, 1, data=torch.tensor([1.5]))
            rc = ctx.lib.gan_bce_logits(xd.ptr, count, target, ls_, 1, acc.ptr, gs_, ctx.dt, None, 8, ctx.ws_ptr, st.ptr if st else None,
                                        ctx.stream())
            assert rc == 0
            sync()
            assert acc.host().numpy()[0].view(np.uint32) == (F32(1.5) + F32(got)).view(np.uint32)
            acc.changed()


@pytest.mark.parametrize("count", E.PATCHGAN_COUNTS)
def test_patchgan_losses(ctx, count):
    """gan_patchgan_losses: all three gradient maps, each pointer null in turn, l1 / gen_total null and non-null, with a scale state;
    gan and disc against their gates, gen_total exactly the fp32 gan + lambda * l1 of the stored values."""
    real, fake = E.logits(count, count), E.logits(count, count + 1, -0.5)
    rd, fd = Guarded(ctx.device, count, data=torch.from_numpy(real)), Guarded(ctx.device, count, data=torch.from_numpy(fake))
    lam, l1v = 100.0, 0.37
    names = ('g_dfake', 'd_dreal', 'd_dfake')
    # (index of the null gradient or -1, scalars: both / none / gen_total without l1, scale state)
    for null, scalars, ls in ((-1, 'both', None), (0, 'none', E.LS_ON), (1, 'both', E.LS_ON), (2, 'gen', None), (-1, 'gen', E.LS_ON)):
        st = scale_state(ctx, ls)
        ls0 = ls[0] if ls else 1.0
        maps = [View(ctx.device, (1, 1, count, 1), 8, 0, ctx.tdtype) if i != null else None for i in range(3)]
        losses = Guarded(ctx.device, 4)                    # [gen_total, gan, l1, disc], NaN
        losses.t[losses.lo + 2] = l1v
        losses.snap = _int_view(losses.t).cpu().clone()
        lp = losses.ptr
        rc = ctx.lib.gan_patchgan_losses(rd.ptr, fd.ptr, count, ctx.dt, *[m.ptr if m else None for m in maps], 8, lam,
                                         lp + 8 if scalars == 'both' else None, lp if scalars != 'none' else None, lp + 4, lp + 12,
                                         ctx.ws_ptr, st.ptr if st else None, ctx.stream())
        assert rc == 0
        sync()
        out = losses.host().numpy()
        got = dict(gan=out[1], disc=out[3], gen_total=out[0] if scalars != 'none' else None)
        got.update({k: m.dense().reshape(-1) if m else None for k, m in zip(names, maps)})
        for k, v in E.check_patchgan(real, fake, ls0, ctx.dt, got, lam, l1v if scalars == 'both' else 0.0).items():
            gate(ctx, 'gan_patchgan_losses', f'{k} ls={ls0:g}', v)
        ch = losses.changed()
        assert not ch[2] and (scalars != 'none' or not ch[0])            # l1 is only read; a null gen_total is not written
        assert all(m.outside_untouched() for m in maps if m) and rd.untouched() and fd.untouched() and (st is None or st.untouched())


@pytest.mark.parametrize("shape", E.L1_SHAPES)
def test_l1(ctx, shape):
    """gan_l1 on views (a: pitch 8 offset 0, b: pitch 16 offset 3, da: pitch 8 offset 2 or null) of NaN-filled buffers: mean and
    sign gradient (exactly 0 where a == b) against their gates, with and without a scale state, loss_accumulate."""
    a, b = E.lattice(shape, shape[2])
    a_st, b_st = E.stored(a, ctx.dt), E.stored(b, ctx.dt)
    av, bv = View(ctx.device, shape, 8, 0, ctx.tdtype, a_st), View(ctx.device, shape, 16, 3, ctx.tdtype, b_st)
    gs_, ls_ = E.L1_GRAD_SCALE, E.L1_LOSS_SCALE
    for ls in (None, E.LS_ON):
        st = scale_state(ctx, ls)
        ls0 = ls[0] if ls else 1.0
        da = View(ctx.device, shape, 8, 2, ctx.tdtype)
        loss = Guarded(ctx.device, 1, data=torch.tensor([7.25]))
        rc = ctx.lib.gan_l1(ctx.dt, C.byref(av.tensor), C.byref(bv.tensor), ls_, 0, loss.ptr, gs_, C.byref(da.tensor), ctx.ws_ptr,
                            st.ptr if st else None, ctx.stream())
        assert rc == 0
        sync()
        got = float(loss.host()[0])
        res = E.check_l1(a_st, b_st, gs_, ls0, ctx.dt, got, da.dense(), ls_)
        for k, v in res.items():
            gate(ctx, 'gan_l1', f'{k} ls={ls0:g}', v)
        eq = (a_st.float() == b_st.float()).reshape(-1)
        assert (da.dense().reshape(-1)[eq].float() == 0).all() and (shape[1] == 1 or int(eq.sum()) >= shape[2] * shape[3])
        assert da.outside_untouched() and av.untouched() and bv.untouched() and (st is None or st.untouched())
        acc = Guarded(ctx.device, 1, data=torch.tensor([1.5]))
        rc = ctx.lib.gan_l1(ctx.dt, C.byref(av.tensor), C.byref(bv.tensor), ls_, 1, acc.ptr, gs_, None, ctx.ws_ptr,
                            st.ptr if st else None, ctx.stream())
        assert rc == 0
        sync()
        assert acc.host().numpy()[0].view(np.uint32) == (F32(1.5) + F32(got)).view(np.uint32)
        acc.changed()


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step0", E.ADAM_BEGIN_STEPS)
def test_adam_begin(dev, step0):
    """gan_adam_begin: step + 1 and lr_t within one ulp of fp32 of the extended-precision value; a skipped step keeps both."""
    for ls in (None, E.LS_ON, E.LS_SKIP):
        st = scale_state(dev, ls)
        step = Guarded(dev.device, 1, torch.int32, data=torch.tensor([step0], dtype=torch.int32), fill=-1)
        lr_t = Guarded(dev.device, 1, data=torch.tensor([0.125]))
        assert dev.lib.gan_adam_begin(step.ptr, lr_t.ptr, E.LR, E.BETA1, E.BETA2, st.ptr if st else None, dev.stream()) == 0
        sync()
        if ls is E.LS_SKIP:
            assert step.untouched() and lr_t.untouched()
        else:
            assert int(step.host()[0]) == step0 + 1
            got = lr_t.host().numpy()[0]
            assert np.isfinite(got) and got > 0
            gate(dev, 'gan_adam_begin', 'lr_t (ulps of fp32, gate 1)', E.ulps_apart32(got, E.lr_t_ref(E.LR, E.BETA1, E.BETA2, step0 + 1)))
            step.changed(), lr_t.changed()
        assert st is None or st.untouched()


def _adam_combos(count):
    """(grad_bf16, grad_scale, scale state): the full cross product on the small counts, every level at least once on the large."""
    full = [(w, gs, ls) for w in (0, 1) for gs in (1.0, 0.5) for ls in (None, E.LS_ON, E.LS_SKIP)]
    return full if count < 1 << 20 else [(0, 1.0, None), (1, 0.5, E.LS_ON), (0, 0.5, E.LS_SKIP), (1, 1.0, None)]


@pytest.mark.parametrize("count", E.ADAM_COUNTS)
def test_adam_tf(dev, count):
    """gan_adam_tf: m, v against fp64 of the stored inputs, p against fp64 of the stored new moments (elementwise_ref.adam_gates);
    fp32 and bf16-wire gradients, grad_scale, the 1/scale factor of a scale state, the skipped step; g = m = v = 0 leaves p as it was."""
    p, m, v, g = E.adam_inputs(count, count)
    lr_t = E.lr_t_model(E.LR, E.BETA1, E.BETA2, 1)
    lrd = torch.tensor([float(lr_t)], dtype=torch.float32, device=dev.device)
    zeros = np.concatenate([np.arange(3, count, 64), np.arange(8, count, 64)])
    for wire, gs_, ls in _adam_combos(count):
        st = scale_state(dev, ls)
        gw = E.cast_ref(g, L.BF16) if wire else torch.from_numpy(g)
        g32 = gw.float().numpy()
        bufs = [Guarded(dev.device, count, data=torch.from_numpy(t)) for t in (p, m, v)]
        gd = Guarded(dev.device, count, gw.dtype, data=gw)
        rc = dev.lib.gan_adam_tf(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, gd.ptr, count, lrd.data_ptr(), E.BETA1, E.BETA2, E.ADAM_EPS, gs_,
                                 st.ptr if st else None, wire, dev.stream())
        assert rc == 0
        sync()
        if ls is E.LS_SKIP:
            assert all(b.untouched() for b in bufs)
        else:
            p1, m1, v1 = (b.host().numpy() for b in bufs)
            for k, val in E.check_adam(p, m, v, g32, gs_ * (ls[1] if ls else 1.0), lr_t, p1, m1, v1).items():
                gate(dev, 'gan_adam_tf', f'{k} wire={wire} gs={gs_:g} ls={"on" if ls else "-"}', val)
            assert np.array_equal(p1[zeros].view(np.uint32), p[zeros].view(np.uint32))
            for b in bufs:
                b.changed()
        assert gd.untouched() and (st is None or st.untouched())
    # return codes (nothing is launched)
    bufs = [Guarded(dev.device, 8, data=torch.zeros(8)) for _ in range(4)]
    args = lambda gp, n, wire: (bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, gp, n, lrd.data_ptr(), E.BETA1, E.BETA2, E.ADAM_EPS, 1.0, None, wire,
                                dev.stream())
    assert dev.lib.gan_adam_tf(*args(bufs[3].ptr, 6, 0)) == L.E_ARG
    assert dev.lib.gan_adam_tf(*args(bufs[3].ptr + 4, 4, 0)) == L.E_ARG and dev.lib.gan_adam_tf(*args(bufs[3].ptr + 8, 4, 0)) == L.E_ARG
    assert dev.lib.gan_adam_tf(*args(bufs[3].ptr + 2, 4, 1)) == L.E_ARG and dev.lib.gan_adam_tf(*args(bufs[3].ptr + 4, 4, 1)) == L.E_ARG
    sync()
    assert all(b.untouched() for b in bufs)


@pytest.mark.parametrize("count", E.CHECK_COUNTS)
def test_grads_check(dev, count):
    """gan_grads_check: fp32 max, subnormals and -0 leave the flag at 0; one +inf, -inf or NaN at the first element, the last (second
    trip of the capped grid) or mid-buffer sets it to 1; [0..2] of the state are never touched."""
    g = E.edge_cycle(count, 5)
    g[~np.isfinite(g)] = F32(3.4e38)
    assert E.flag_ref(g) == 0.0
    assert count == 4 or ((g == F32(3.4e38)).any() and (np.abs(g[g != 0]) < 1e-38).any() and np.signbit(g[g == 0]).any())
    gd = Guarded(dev.device, count, data=torch.from_numpy(g))

    def run():
        st = scale_state(dev, (1024.0, 1.0 / 1024.0, 5.0, 0.0))
        assert dev.lib.gan_grads_check(gd.ptr, count, st.ptr, dev.stream()) == 0
        sync()
        assert not st.changed()[:3].any()
        return float(st.host()[3])
    assert run() == 0.0
    for pos in (0, count - 1, count // 2):
        for bad in (math.inf, -math.inf, math.nan):
            keep = float(gd.t[gd.lo + pos])
            gd.t[gd.lo + pos] = bad
            h = g.copy()
            h[pos] = bad
            assert run() == E.flag_ref(h) == 1.0, (pos, bad)
            gd.t[gd.lo + pos] = keep
    assert run() == 0.0 and gd.untouched()


# ---- casts, copies, wire format -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", E.PACK_VIEWS, ids=lambda v: f"pitch{v[0]}+{v[1]}")
@pytest.mark.parametrize("shape", E.PACK_SHAPES, ids=str)
def test_pack_unpack_copy_view(ctx, shape, view):
    """gan_pack / gan_unpack / gan_copy_view / gan_pack_multi on ties, overflow, subnormals, +-0, inf and NaN: bit-equal to the
    round-to-nearest-even cast, the exact widening and the copied bits."""
    pitch, c0 = view
    total = int(np.prod(shape))
    x = E.edge_cycle(total, total)
    ref = E.cast_ref(x, ctx.dt)
    xd = Guarded(ctx.device, total, data=torch.from_numpy(x))
    dst = View(ctx.device, shape, pitch, c0, ctx.tdtype)
    assert ctx.lib.gan_pack(ctx.dt, xd.ptr, C.byref(dst.tensor), ctx.stream()) == 0
    out = Guarded(ctx.device, total)
    assert ctx.lib.gan_unpack(ctx.dt, C.byref(dst.tensor), out.ptr, ctx.stream()) == 0
    other = View(ctx.device, shape, 24 - pitch, 5 - c0, ctx.tdtype)            # the other pitch, another offset
    assert ctx.lib.gan_copy_view(ctx.dt, C.byref(dst.tensor), C.byref(other.tensor), ctx.stream()) == 0
    sync()
    gate(ctx, 'gan_pack', 'bits = RNE cast', E.exact(dst.dense().reshape(-1), ref))
    gate(ctx, 'gan_unpack', 'bits = widened', E.exact(out.host(), ref.float()))
    gate(ctx, 'gan_copy_view', 'bits = source', 0.0 if torch.equal(_int_view(other.dense()), _int_view(dst.dense())) else math.inf)
    assert dst.outside_untouched() and other.outside_untouched() and xd.untouched()
    out.changed()
    for n in (1, 4):
        x2 = E.edge_cycle(total, total + 1)
        x2d = Guarded(ctx.device, total, data=torch.from_numpy(x2))
        dsts = [View(ctx.device, shape, (pitch, 24 - pitch)[k % 2], (c0, 5 - c0)[k % 2], ctx.tdtype) for k in range(n)]
        srcs = (C.c_void_p * n)(*[(xd, x2d)[k // 2 % 2].ptr for k in range(n)])
        tens = (L.GanTensor * n)(*[d.tensor for d in dsts])
        assert ctx.lib.gan_pack_multi(ctx.dt, n, srcs, tens, ctx.stream()) == 0
        sync()
        for k, d in enumerate(dsts):
            gate(ctx, 'gan_pack_multi', f'bits = RNE cast (n={n})', E.exact(d.dense().reshape(-1), (ref, E.cast_ref(x2, ctx.dt))[k // 2 % 2]))
            assert d.outside_untouched()
        assert torch.equal(_int_view(dsts[0].dense()), _int_view(dst.dense()))          # = the single call


@pytest.mark.parametrize("count", E.WIRE_COUNTS)
def test_grad_pack_unpack(dev, count):
    """gan_grad_pack: bit-equal to the bf16 round-to-nearest-even cast; gan_grad_unpack: bit-equal to ONE fp32 multiply."""
    x = E.edge_cycle(count, 9)
    ref = E.cast_ref(x, L.BF16)
    xd = Guarded(dev.device, count, data=torch.from_numpy(x))
    wire = Guarded(dev.device, count, torch.bfloat16)
    assert dev.lib.gan_grad_pack(xd.ptr, wire.ptr, count, dev.stream()) == 0
    sync()
    gate(dev, 'gan_grad_pack', 'bits = RNE cast', E.exact(wire.host(), ref))
    wire.changed()
    assert xd.untouched()
    wire.snap = _int_view(wire.t).cpu().clone()
    got = wire.host()
    for scale in (1.0, 0.5, 1.0 / 3.0):
        out = Guarded(dev.device, count)
        assert dev.lib.gan_grad_unpack(wire.ptr, out.ptr, count, scale, dev.stream()) == 0
        sync()
        gate(dev, 'gan_grad_unpack', f'bits = fp32 multiply x {scale:.3g}', E.exact(out.host(), E.wire_unpack_ref(got, float(F32(scale)))))
        out.changed()
    assert wire.untouched()
    s = dev.stream()
    assert dev.lib.gan_grad_pack(xd.ptr, wire.ptr, 12, s) == L.E_ARG and dev.lib.gan_grad_unpack(wire.ptr, xd.ptr, 12, 1.0, s) == L.E_ARG
    assert dev.lib.gan_grad_pack(xd.ptr + 4, wire.ptr, 8, s) == L.E_ARG and dev.lib.gan_grad_pack(xd.ptr, wire.ptr + 8, 8, s) == L.E_ARG
    assert dev.lib.gan_grad_unpack(wire.ptr + 2, xd.ptr, 8, 1.0, s) == L.E_ARG and dev.lib.gan_grad_unpack(wire.ptr, xd.ptr + 8, 8, 1.0, s) == L.E_ARG
    sync()
    assert wire.untouched() and xd.untouched()


# ---- dropout masks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,step", E.MASK_KEYS)
def test_dropout_masks(dev, seed, step):
    """gan_dropout_mask and gan_dropout_mask_multi: bit-equal to the SplitMix64 reference for every count, stream id and draw; the
    launch counter advances once per launch; a mask that starts at byte 3 of its allocation takes the byte path."""
    stepd = torch.tensor([step], dtype=torch.int32, device=dev.device)
    for count in E.MASK_COUNTS:
        for sid in E.MASK_SIDS:
            mk = Guarded(dev.device, count, torch.uint8)
            assert dev.lib.gan_dropout_mask(mk.ptr, count, seed, stepd.data_ptr(), sid, dev.stream()) == 0
            sync()
            gate(dev, 'gan_dropout_mask', 'bits = SplitMix64', E.exact(mk.host(), E.mask_ref(count, seed, step, sid)))
            mk.changed()
    for draws0 in (None, (0, 0), (3, 0)):
        for group, shift in ((E.MASK_COUNTS[:4], 0), (E.MASK_COUNTS[4:], 0), (E.MASK_COUNTS[3:], 3)):
            n = len(group)
            sids = [E.MASK_SIDS[k % 2] for k in range(n)]
            mks = [Guarded(dev.device, cnt, torch.uint8, shift=shift if k % 2 == 0 else 0) for k, cnt in enumerate(group)]
            assert shift == 0 or all(mk.ptr % 8 == 3 for mk in mks[0::2])
            draws = Guarded(dev.device, 2, torch.int32, data=torch.tensor(draws0, dtype=torch.int32), fill=-1) if draws0 else None
            ptrs = (C.c_void_p * n)(*[mk.ptr for mk in mks])
            cnts = (C.c_int64 * n)(*group)
            assert dev.lib.gan_dropout_mask_multi(n, ptrs, cnts, seed, stepd.data_ptr(), (C.c_uint32 * n)(*sids),
                                                  draws.ptr if draws else None, dev.stream()) == 0
            sync()
            draw = draws0[0] if draws0 else 0
            for mk, cnt, sid in zip(mks, group, sids):
                gate(dev, 'gan_dropout_mask_multi', f'bits = SplitMix64 (draw {draw}, start % 8 = {mk.ptr % 8})',
                     E.exact(mk.host(), E.mask_ref(cnt, seed, step, sid, draw)))
                mk.changed()
            if draws:
                assert draws.host().tolist() == [draw + 1, 0]
                draws.changed()


# ---- weight layouts -----------------------------------------------------------------------------------------------------------------------
def _master(A, B):
    return np.resize(E.edge_cycle(16 * A * B, A * 1000 + B), (16, A, B))


@pytest.mark.parametrize("AB", E.WPREP_SHAPES, ids=str)
def test_weights_prepare(ctx, AB):
    """gan_weights_prepare: nat [16][A][B8] and tr [16][B][A8] bit-equal to the cast master in both layouts, the padding written as
    zeros over the NaN the buffers held; nat only, tr only, both."""
    A, B = AB
    w = _master(A, B)
    nat_ref, tr_ref = E.wprep_ref(w, ctx.dt)
    md = Guarded(ctx.device, w.size, data=torch.from_numpy(w))
    for want_nat, want_tr in ((True, False), (False, True), (True, True)):
        nat, tr = Guarded(ctx.device, nat_ref.numel(), ctx.tdtype), Guarded(ctx.device, tr_ref.numel(), ctx.tdtype)
        assert ctx.lib.gan_weights_prepare(md.ptr, A, B, ctx.dt, nat.ptr if want_nat else None, tr.ptr if want_tr else None, ctx.stream()) == 0
        sync()
        if want_nat:
            gate(ctx, 'gan_weights_prepare', 'nat bits', E.exact(nat.host(), nat_ref.reshape(-1)))
            nat.changed()
        else:
            assert nat.untouched()
        if want_tr:
            gate(ctx, 'gan_weights_prepare', 'tr bits', E.exact(tr.host(), tr_ref.reshape(-1)))
            tr.changed()
        else:
            assert tr.untouched()
    assert md.untouched()


def test_weights_prepare_multi(ctx):
    """gan_weights_prepare_multi over the five tensors in one table: equal to the layout reference (and so to the single calls)."""
    offs, total = [], 0
    for A, B in E.WPREP_SHAPES:
        offs.append(total)
        total += (16 * A * B + 63) // 64 * 64
    flat = np.full(total, np.nan, dtype=F32)
    for (A, B), o in zip(E.WPREP_SHAPES, offs):
        flat[o:o + 16 * A * B] = _master(A, B).reshape(-1)
    md = Guarded(ctx.device, total, data=torch.from_numpy(flat))
    refs = [E.wprep_ref(_master(A, B), ctx.dt) for A, B in E.WPREP_SHAPES]
    nats = [Guarded(ctx.device, r[0].numel(), ctx.tdtype) for r in refs]
    trs = [Guarded(ctx.device, r[1].numel(), ctx.tdtype) for r in refs]
    ents, tiles = [], 0
    for (A, B), o, nat, tr in zip(E.WPREP_SHAPES, offs, nats, trs):
        tb = (E.pad8(B) + 63) // 64
        ents.append(L.GanPrepEntry(md.ptr + 4 * o, nat.ptr, tr.ptr, A, B, tiles, tb))
        tiles += 16 * ((E.pad8(A) + 63) // 64) * tb
    table = torch.frombuffer(bytearray(bytes((L.GanPrepEntry * len(ents))(*ents))), dtype=torch.uint8).to(ctx.device)
    assert ctx.lib.gan_weights_prepare_multi(table.data_ptr(), len(ents), tiles, ctx.dt, ctx.stream()) == 0
    sync()
    for (A, B), r, nat, tr in zip(E.WPREP_SHAPES, refs, nats, trs):
        gate(ctx, 'gan_weights_prepare_multi', f'nat bits {A}x{B}', E.exact(nat.host(), r[0].reshape(-1)))
        gate(ctx, 'gan_weights_prepare_multi', f'tr bits {A}x{B}', E.exact(tr.host(), r[1].reshape(-1)))
        nat.changed(), tr.changed()
    assert md.untouched()


# ---- sum3 -----------------------------------------------------------------------------------------------------------------------------------
def test_sum3(dev):
    """gan_sum3: (a + b) + c in fp32, bit for bit, for n = 1 and 64; n = 0 and 65 are refused."""
    a, b, c = (E.edge_cycle(64, s) for s in (1, 2, 3))
    a[np.isnan(a)], b[np.isinf(b)] = F32(0.1), F32(-7.0)           # (inf - inf and NaN stay in the mix through b and c)
    bufs = [Guarded(dev.device, 64, data=torch.from_numpy(t)) for t in (a, b, c)]
    with np.errstate(invalid='ignore', over='ignore'):
        ref = torch.from_numpy(E.sum3_ref(a, b, c))
    for n in (1, 64):
        out = Guarded(dev.device, 64)
        assert dev.lib.gan_sum3(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, out.ptr, n, dev.stream()) == 0
        sync()
        gate(dev, 'gan_sum3', f'bits = (a+b)+c, n={n}', E.exact(out.host()[:n], ref[:n]))
        assert not out.changed()[n:].any()
    out = Guarded(dev.device, 64)
    for n in (0, 65):
        assert dev.lib.gan_sum3(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, out.ptr, n, dev.stream()) == L.E_ARG
    sync()
    assert out.untouched() and all(b_.untouched() for b_ in bufs)
