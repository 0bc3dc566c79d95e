"""Image history pool of the CycleGAN step on the GPU: gan_pool_exchange bit for bit against the numpy
restatement (tests/pool_ref.py), the three-invocation discriminator call against the oracle, the step with pools against its own
pieces, the captured step against the eager one, and the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from oracle import gan_oracle as O
from tests import pool_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {'f32': (L.F32, torch.int32, np.int32), 'bf16': (L.BF16, torch.int16, np.int16), 'f16': (L.F16, torch.int16, np.int16)}
KEYS = ['fake_y', 'cycled_x', 'fake_x', 'cycled_y', 'same_x', 'same_y']


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------------
class _Rig:
    """src, dst, pool and state inside larger buffers of known bits: a guard image on either side of the views, the views at a
    channel offset of a wider pitch.  Everything is handled as integers of the element's width: the kernel only moves bits (NaN
    patterns included)."""

    def __init__(self, dtype, P, B, h, w, c, pitch, c0, seed):
        self.dt, tdt, self.ndt = DT[dtype]
        self.P, self.B, self.h, self.w, self.c, self.pitch, self.c0 = P, B, h, w, c, pitch, c0
        self.rng = np.random.default_rng(seed)
        info = np.iinfo(self.ndt)
        self.bits = lambda shape: self.rng.integers(info.min, info.max, shape, dtype=self.ndt, endpoint=True)
        dev = 'cuda:0'
        self.src = torch.from_numpy(self.bits((B + 2, h, w, pitch))).to(dev)
        self.dst = torch.from_numpy(self.bits((B + 2, h, w, pitch))).to(dev)
        self.pool = torch.from_numpy(self.bits((P + 2, h, w, c))).to(dev)
        self.state = torch.tensor([7, 7, 0, 0, 0, 7, 7, 7], dtype=torch.int32, device=dev)       # the three words at [2:5]
        es = self.src.element_size()
        view = lambda t: L.GanTensor(t.data_ptr() + (h * w * pitch + c0) * es, B, h, w, c, pitch)
        self.desc = lambda sid: L.GanPoolDesc(self.dt, view(self.src), view(self.dst), self.pool.data_ptr() + h * w * c * es, P, sid,
                                               R.GPU_SEED, self.state.data_ptr() + 8)
        self.ref_pool = self.pool[1:P + 1].cpu().numpy().copy()
        self.ref_state = (0, 0)

    def new_images(self):
        self.src.copy_(torch.from_numpy(self.bits(tuple(self.src.shape))))

    def check_launch(self, sid, launch=None):
        """One query (launch() enqueues it; default: the entry point itself) against the reference, every byte accounted for."""
        c0, c, B, P = self.c0, self.c, self.B, self.P
        src0, dst0, pool0 = self.src.cpu().numpy().copy(), self.dst.cpu().numpy().copy(), self.pool.cpu().numpy().copy()
        out, self.ref_pool, self.ref_state, trace = R.query(src0[1:B + 1, :, :, c0:c0 + c], self.ref_pool, self.ref_state, R.GPU_SEED, sid)
        if launch is None:
            d = self.desc(sid)
            L.check(L.load().gan_pool_exchange(C.byref(d), torch.cuda.current_stream().cuda_stream), "pool_exchange")
        else:
            launch()
        torch.cuda.synchronize()
        src1, dst1, pool1, state1 = self.src.cpu().numpy(), self.dst.cpu().numpy(), self.pool.cpu().numpy(), self.state.cpu().numpy()
        assert np.array_equal(src1, src0)                                                   # src is only read
        assert np.array_equal(dst1[1:B + 1, :, :, c0:c0 + c], out), trace                     # outputs
        dst0[1:B + 1, :, :, c0:c0 + c] = out
        assert np.array_equal(dst1, dst0)                                                   # pad channels and guard images
        assert np.array_equal(pool1[1:P + 1], self.ref_pool), trace                           # every slot, written or not
        assert np.array_equal(pool1[[0, P + 1]], pool0[[0, P + 1]])
        assert state1.tolist() == [7, 7, self.ref_state[0], self.ref_state[1], 0, 7, 7, 7]    # advanced once, ticket cleared
        return trace


def _six_launches(rig, sids=(R.STREAM_Y, R.STREAM_X)):
    kinds = set()
    for sid in sids:
        rig.pool[1:rig.P + 1].copy_(torch.from_numpy(rig.bits((rig.P, rig.h, rig.w, rig.c))))      # whatever an empty pool holds
        rig.ref_pool = rig.pool[1:rig.P + 1].cpu().numpy().copy()
        rig.state[2:5].zero_()
        rig.ref_state = (0, 0)
        for _ in range(R.GPU_LAUNCHES):
            rig.new_images()
            kinds |= {k for k, _ in rig.check_launch(sid)}
    return kinds


@pytest.mark.parametrize("P,B", R.GPU_CASES)
@pytest.mark.parametrize("c,c0", [(1, 5), (3, 2)])
@pytest.mark.parametrize("dtype", ['f32', 'bf16', 'f16'])
def test_exchange_matches_the_reference_bit_for_bit(dtype, c, c0, P, B):
    kinds = _six_launches(_Rig(dtype, P, B, 8, 8, c, 8, c0, seed=100 * P + B))
    assert 'fill' in kinds and 'swap' in kinds


@pytest.mark.parametrize("dtype,h,w,c,pitch,c0", [
    ('bf16', 20, 12, 3, 8, 0),        # 720 elements: no multiple of a workgroup's span, nor of 8
    ('f32', 20, 12, 1, 8, 7),
    ('f16', 40, 40, 3, 8, 1),         # 4,800 elements: five workgroups hand the state over
    ('bf16', 8, 8, 8, 8, 0),          # dense on all three sides: the 16-byte path, one workgroup
    ('f32', 48, 48, 8, 8, 0),         # ... 4,608 vectors, five workgroups
    ('bf16', 5, 3, 3, 3, 0),          # pitch == c, but 90 bytes per image: elements again
])
def test_exchange_other_shapes_and_paths(dtype, h, w, c, pitch, c0):
    kinds = _six_launches(_Rig(dtype, 3, 2, h, w, c, pitch, c0, seed=h * w + c), sids=(R.STREAM_X,))
    assert kinds == {'fill', 'swap', 'keep'}


def test_bad_arguments_launch_nothing():
    rig = _Rig('bf16', 3, 2, 8, 8, 3, 8, 2, seed=5)
    before = [t.clone() for t in (rig.src, rig.dst, rig.pool, rig.state)]
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    d = rig.desc(32); d.capacity = 0
    assert lib.gan_pool_exchange(C.byref(d), st) == L.E_ARG
    d = rig.desc(32); d.dst.h = 4
    assert lib.gan_pool_exchange(C.byref(d), st) == L.E_ARG
    d = rig.desc(32); d.src.c = 1
    assert lib.gan_pool_exchange(C.byref(d), st) == L.E_ARG
    d = rig.desc(32); d.dst.n = 1
    assert lib.gan_pool_exchange(C.byref(d), st) == L.E_ARG
    d = rig.desc(32); d.state = None
    assert lib.gan_pool_exchange(C.byref(d), st) == L.E_ARG
    torch.cuda.synchronize()
    for a, b in zip(before, (rig.src, rig.dst, rig.pool, rig.state)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("P,B,sid", [(3, 2, R.STREAM_X), (1, 4, R.STREAM_Y)])
def test_exchange_captured_once_and_replayed_six_times(P, B, sid):
    """One launch in a graph, replayed with new images each time: the decisions come from the device state, which advances under
    replay - the same bits as six eager launches (the reference is the same)."""
    rig = _Rig('bf16', P, B, 8, 8, 3, 8, 2, seed=77)
    d = rig.desc(sid)
    lib = L.load()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.check(lib.gan_pool_exchange(C.byref(d), torch.cuda.current_stream().cuda_stream), "pool_exchange")
    torch.cuda.synchronize()
    assert rig.state.tolist() == [7, 7, 0, 0, 0, 7, 7, 7]           # capturing enqueued nothing
    kinds = set()
    for _ in range(R.GPU_LAUNCHES):
        rig.new_images()
        kinds |= {k for k, _ in rig.check_launch(sid, launch=g.replay)}
    assert kinds == {'fill', 'swap', 'keep'}


# ---- the discriminator call ------------------------------------------------------------------------------------------------------------
def test_disc_call_layout():
    from gan_amd.nets import Ctx, DiscriminatorNet
    ctx = Ctx('cuda:0', 'f32')
    for norm, groups, pgroups in (('instancenorm', 6, 4), ('batchnorm', 3, 2)):
        net = DiscriminatorNet(ctx, 1, False, norm)
        dc = net.new_call(2, 32, calls=3, param_calls=2)
        assert (dc.N, dc.calls, dc.param_calls, dc.groups, dc.param_calls * dc.gper) == (6, 3, 2, groups, pgroups)
        assert dc.xin.t.shape[0] == 6 and dc.logits.t.shape[0] == 6
        assert net.new_call(2, 32, calls=2).param_calls == 2 and net.new_call(2, 32, calls=3).param_calls == 3      # default: all
        for bad in (0, 4):
            with pytest.raises(ValueError):
                net.new_call(2, 32, calls=3, param_calls=bad)


def _pools(ctx, S, Cc, capacity, seed=R.GPU_SEED):
    from gan_amd.pool import STREAM_X, STREAM_Y, ImagePool
    assert (STREAM_Y, STREAM_X) == (R.STREAM_Y, R.STREAM_X)
    return ImagePool(ctx, S, Cc, capacity, seed, STREAM_Y), ImagePool(ctx, S, Cc, capacity, seed, STREAM_X)


def _dev(ctx, *arrays):
    return [torch.from_numpy(a).to(ctx.device) for a in arrays]


@pytest.mark.parametrize("B,seeds", [(1, (21, 9, 40)), (2, (51, 13, 140))])
def test_fill_phase_against_the_oracle(B, seeds):
    """First step of an empty pool of 4: pooled == current, so the step is the reference's step - the gates of
    test_cyclegan_train_step_parity[f32] (B = 1) and test_cyclegan_batch2_f32_vs_oracle (B = 2), unchanged, on a discriminator
    call of three invocations whose parameter pass covers two."""
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep
    from tests.test_gpu_step import check_grads
    ctx = Ctx('cuda:0', 'f32')
    S, Cc = 256, 1
    pools = _pools(ctx, S, Cc, 4)
    st = CycleGANStep(ctx, B, S, Cc, lam=10.0, seed=7, dropout=True, pools=pools)
    assert st.dy.calls == 3 and st.dy.param_calls == 2 and st.dx.calls == 3
    n = 'instancenorm'
    ps, pair_seed, mask_seed = seeds
    Ps = [O.init_generator(Cc, n, seed=ps), O.init_generator(Cc, n, seed=ps + 1),
          O.init_discriminator(Cc, False, n, seed=ps + 2), O.init_discriminator(Cc, False, n, seed=ps + 3)]
    for net, P in zip(st.nets(), Ps):
        net.params.load_numpy(P)
    rx, ry = O.synthetic_pair(B, S, Cc, seed=pair_seed)
    masks = {k: O.dropout_masks(B, S, seed=mask_seed + i) for i, k in enumerate(KEYS)}
    for k, call in st.gen_calls().items():
        call.set_dropmasks(masks[k])
    Pr = [{k: v.astype(np.float64) for k, v in P.items()} for P in Ps]
    m64 = {k: [m.astype(np.float64) for m in v] for k, v in masks.items()}
    out = O.cyclegan_train_step(*Pr, [O.AdamTF() for _ in range(4)], rx.astype(np.float64), ry.astype(np.float64), 10.0, m64, True,
                                return_grads=True)
    ref_losses, fakes, grads = np.array(out[:7], np.float64), out[7], out[8:]
    losses = st.train_step(*_dev(ctx, rx, ry), True).cpu().numpy()
    err = np.abs(st.fy.output_f32().cpu().numpy() - fakes['fake_y']).max()
    print(f"[B={B}] fake_y max-abs err {err:.3e}; losses {losses} ref {ref_losses}")
    assert err < 1e-3 and np.allclose(losses, ref_losses, rtol=5e-4), (err, losses, ref_losses)
    for k, call in st.gen_calls().items():
        if k in fakes:
            assert np.abs(call.output_f32().cpu().numpy() - fakes[k]).max() < 1e-3, k
    pairs = []
    for nm, net, g in zip(('Gg', 'Gf', 'Dx', 'Dy'), st.nets(), grads):
        got = net.params.to_numpy('grad')
        pairs += [(nm + '.' + k, got[k], g[k]) for k in g]
    check_grads('f32', pairs, 1e-1)
    for p in pools:
        assert p.state.tolist() == [B, 1, 0]


# ---- the step after the fill -----------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy()


def _fakes(st):
    """Bits of the current fake_y / fake_x (the generators' output views) and of the pooled slots of dy.xin / dx.xin."""
    B, Cc = st.B, st.C
    cur = [_bits(g.out.t[:B, :, :, :Cc]) for g in (st.gA, st.gB)]
    pooled = [_bits(d.xin.t[B:2 * B, :, :, :Cc]) for d in (st.dy, st.dx)]
    current = [_bits(d.xin.t[2 * B:, :, :, :Cc]) for d in (st.dy, st.dx)]
    for a, b in zip(cur, current):
        assert np.array_equal(a, b)                  # invocation 2 holds the current fakes
    return cur, pooled


def _snapshot(st):
    return [(n.params, n.params.master.clone(), n.params.m.clone(), n.params.v.clone(), n.params.step.clone()) for n in st.nets()]


def _restore(saved):
    for ps, w, m, v, step in saved:
        ps.master.copy_(w); ps.m.copy_(m); ps.v.copy_(v); ps.step.copy_(step)
        ps.prepare()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-20))


def test_after_the_fill_the_discriminators_see_the_pool_and_the_generators_do_not():
    """Capacity 1, B = 2, fp32, three eager steps.  Tolerance of the regrouped passes: the per-tensor 1e-2 (gradients) and 1e-5
    (losses) of test_cyclegan_batched_generator_calls_equal_separate_calls - the same sums over other batch groupings."""
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep
    ctx = Ctx('cuda:0', 'f32')
    B, S, Cc = 2, 256, 1
    pools = _pools(ctx, S, Cc, 1)
    st = CycleGANStep(ctx, B, S, Cc, lam=10.0, seed=7, dropout=True, pools=pools)
    plain = CycleGANStep(ctx, B, S, Cc, lam=10.0, seed=7, dropout=True, nets=st.nets())          # pool-less, same networks
    masks = {k: O.dropout_masks(B, S, seed=60 + i) for i, k in enumerate(KEYS)}
    for s_ in (st, plain):
        for k, call in s_.gen_calls().items():
            call.set_dropmasks(masks[k])
    ref = [(np.zeros((1, S, S, Cc), np.int32), (0, 0)) for _ in pools]
    kinds = set()
    for step in range(3):
        rx, ry = O.synthetic_pair(B, S, Cc, seed=19 + step)
        x, y = _dev(ctx, rx, ry)
        saved = _snapshot(st)
        losses = st.train_step(x, y, True).cpu().numpy().copy()
        cur, pooled = _fakes(st)
        for k, (pool, sid) in enumerate(zip(pools, (R.STREAM_Y, R.STREAM_X))):
            out, new_pool, new_state, trace = R.query(cur[k], ref[k][0], ref[k][1], R.GPU_SEED, sid)
            kinds |= {kd for kd, _ in trace}
            assert np.array_equal(pooled[k], out), (step, k, trace)                            # the pooled slot, bit for bit
            assert np.array_equal(_bits(pool.storage), new_pool) and pool.state.tolist() == [new_state[0], new_state[1], 0]
            ref[k] = (new_pool, new_state)
    assert 'swap' in kinds
    assert any(not np.array_equal(p, c_) for p, c_ in zip(pooled, cur))        # step 3 really trained a discriminator on history
    grads = [n.params.to_numpy('grad') for n in st.nets()]
    # the discriminators of step 3: a stand-alone two-invocation call of the same weights on [real ; pooled]
    _restore(saved)
    for net, d3, idx, g3 in ((st.Dy, st.dy, 6, grads[3]), (st.Dx, st.dx, 5, grads[2])):
        d2 = net.new_call(B, S, calls=2)
        d2.xin.t.copy_(d3.xin.t[:2 * B])
        d2.forward()
        (rp, cnt), (pp, _) = d2.logits_view(0), d2.logits_view(1)
        st._bce(rp, cnt, 1.0, 11, 0.5, False, 0.5, d2.dlogits_ptr(0))
        st._bce(pp, cnt, 0.0, 11, 0.5, True, 0.5, d2.dlogits_ptr(1))
        d2.backward_params()
        torch.cuda.synchronize()
        alone = float(st.losses[11].item())
        print(f"disc loss [{idx}] step {losses[idx]!r} stand-alone {alone!r}")
        assert np.isclose(losses[idx], alone, rtol=1e-5)
        got = net.params.to_numpy('grad')
        for k in got:
            print(f"    {k}: rel {_rel(g3[k], got[k]):.3e}")
            assert _rel(g3[k], got[k]) < 1e-2, k
    # the generators of step 3: a pool-less step from the same weights, inputs and masks
    l0 = plain.train_step(x, y, True).cpu().numpy().copy()
    g0 = [n.params.to_numpy('grad') for n in plain.nets()]
    for i in (0, 1, 2, 3, 4):
        assert np.isclose(losses[i], l0[i], rtol=1e-5), (i, losses, l0)
    assert np.allclose(st.losses[7:9].cpu().numpy(), plain.losses[7:9].cpu().numpy(), rtol=1e-5)
    for nm, a, b in zip(('Gg', 'Gf'), grads[:2], g0[:2]):
        for k in b:
            assert _rel(a[k], b[k]) < 1e-2, (nm, k, _rel(a[k], b[k]))


def test_graph_replay_with_pools_matches_eager():
    """test_cyclegan_graph_replay_matches_eager with pools of 2: bf16, B = 1, three steps, its tolerances; capture() leaves the
    pools empty."""
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep
    rx, ry = O.synthetic_pair(1, 256, 1, seed=41)
    res = []
    for graph in (False, True):
        ctx = Ctx('cuda:0', 'bf16')
        pools = _pools(ctx, 256, 1, 2)
        st = CycleGANStep(ctx, 1, 256, 1, lam=10.0, seed=7, pools=pools)
        w0 = [n.params.master.clone() for n in st.nets()]
        x = _dev(ctx, rx, ry)
        run = st.capture(training=True) if graph else (lambda a, b: st.train_step(a, b, True))
        torch.cuda.synchronize()
        for p in pools:
            assert p.state.tolist() == [0, 0, 0] and not p.storage.any()
        for n_, w_ in zip(st.nets(), w0):          # (capture ran warm-up steps)
            n_.params.master.copy_(w_); n_.params.prepare()
            n_.params.m.zero_(); n_.params.v.zero_(); n_.params.step.zero_()
        for call in vars(st).values():
            if hasattr(call, 'mask_draws'):
                call.mask_draws.zero_()
        losses = [run(*x)[:7].cpu().numpy().copy() for _ in range(3)]
        torch.cuda.synchronize()
        res.append((losses, [n.params.master.clone() for n in st.nets()], [p.state.tolist() for p in pools]))
    (le, we, se), (lg, wg, sg) = res
    assert se == sg == [[2, 3, 0], [2, 3, 0]]
    assert np.allclose(le, lg, rtol=1e-5), (le, lg)
    for a, b in zip(we, wg):
        assert torch.allclose(a, b, atol=1e-6), float((a - b).abs().max())


def test_serial_schedule_with_pools_matches_the_two_lane_one():
    """ctx.lanes off (one chain, separate Adam passes) against the two-lane schedule, fp32, two steps.  Step 1 starts from the same
    weights: the same forward launches - losses to 1e-5, pools bit for bit - and gradients that are the same sums regrouped
    (per-tensor 1e-2, as the batched-against-separate test).  Step 2 starts from weights that differ by the two schedules' Adam
    steps on those gradients: at most 2 * lr = 4e-4 per weight and far less where the gradients agree; its losses are held to
    1e-3, the pools' decisions (state) exactly."""
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep
    B, S, Cc = 1, 256, 1
    masks = {k: O.dropout_masks(B, S, seed=80 + i) for i, k in enumerate(KEYS)}
    res = []
    for lanes in (True, False):
        ctx = Ctx('cuda:0', 'f32', lanes=lanes)
        pools = _pools(ctx, S, Cc, 1)
        st = CycleGANStep(ctx, B, S, Cc, lam=10.0, seed=7, dropout=True, pools=pools)
        for k, call in st.gen_calls().items():
            call.set_dropmasks(masks[k])
        rows = []
        for step in range(2):
            x, y = _dev(ctx, *O.synthetic_pair(B, S, Cc, seed=29 + step))
            losses = st.train_step(x, y, True)[:7].cpu().numpy().copy()
            rows.append((losses, [n.params.to_numpy('grad') for n in st.nets()], [p.state.tolist() for p in pools],
                         [_bits(p.storage) for p in pools], _fakes(st)[1]))
        res.append(rows)
    two, one = res
    print("step 1 losses", two[0][0], one[0][0], "\nstep 2 losses", two[1][0], one[1][0])
    assert np.allclose(two[0][0], one[0][0], rtol=1e-5)
    assert two[0][2] == one[0][2] == [[1, 1, 0], [1, 1, 0]] and two[1][2] == one[1][2] == [[1, 2, 0], [1, 2, 0]]
    for a, b in zip(two[0][3] + two[0][4], one[0][3] + one[0][4]):
        assert np.array_equal(a, b)
    for ga, gb in zip(two[0][1], one[0][1]):
        for k in gb:
            assert _rel(ga[k], gb[k]) < 1e-2, (k, _rel(ga[k], gb[k]))
    assert np.allclose(two[1][0], one[1][0], rtol=1e-3)


def test_steps_of_two_batch_sizes_share_one_pair_of_pools():
    """A batch of 2, then a last partial batch of 1 in a second step object: both query the model's pools."""
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep
    ctx = Ctx('cuda:0', 'bf16')
    S, Cc = 256, 1
    pools = _pools(ctx, S, Cc, 2)
    big = CycleGANStep(ctx, 2, S, Cc, lam=10.0, seed=7, pools=pools)
    small = CycleGANStep(ctx, 1, S, Cc, lam=10.0, seed=7, nets=big.nets(), pools=pools)
    ref = [(np.zeros((2, S, S, Cc), np.int16), (0, 0)) for _ in pools]
    for st, seed in ((big, 3), (small, 4), (small, 5)):
        x, y = _dev(ctx, *O.synthetic_pair(st.B, S, Cc, seed=seed))
        st.train_step(x, y, True)
        cur, pooled = _fakes(st)
        for k, sid in enumerate((R.STREAM_Y, R.STREAM_X)):
            out, new_pool, new_state, _ = R.query(cur[k], ref[k][0], ref[k][1], R.GPU_SEED, sid)
            assert np.array_equal(pooled[k], out)
            ref[k] = (new_pool, new_state)
    for k, p in enumerate(pools):
        assert p.state.tolist() == [2, 3, 0] == [ref[k][1][0], ref[k][1][1], 0]
        assert np.array_equal(_bits(p.storage), ref[k][0])


def test_refusals_of_the_step():
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep
    ctx = Ctx('cuda:0', 'bf16')
    pools = _pools(ctx, 256, 1, 2)
    with pytest.raises(ValueError):
        CycleGANStep(ctx, 1, 256, 1, merged=False, pools=pools)
    with pytest.raises(ValueError):
        CycleGANStep(ctx, 1, 256, 3, pools=pools)            # pools of another image shape
    st = CycleGANStep(ctx, 1, 256, 1, pools=pools)
    x, y = st._example_inputs()
    with pytest.raises(ValueError):
        st.train_step(x, y, training=False)                  # validation judges the current fakes: no pools
    assert pools[0].state.tolist() == [0, 0, 0]
    pools[0].state.fill_(1); pools[0].storage.fill_(1)
    pools[0].reset()
    assert pools[0].state.tolist() == [0, 0, 0] and not pools[0].storage.any()


def test_pools_none_builds_todays_step(monkeypatch):
    """The captured step with pools=None: the same library calls and the same kernel launches, one for one, as the step built
    without the argument."""
    import gc
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep
    from tests.launch_audit import Recorder
    gc.collect()
    torch.cuda.synchronize()
    rec = Recorder(monkeypatch)
    rec.hook_capture(monkeypatch)
    logs = []
    for kw in ({}, {'pools': None}):
        ctx = Ctx('cuda:0', 'bf16')
        st = CycleGANStep(ctx, 1, 256, 1, lam=10.0, seed=123, **kw)
        n0 = len(rec.calls)
        L.set_option('diag.launch_log', 1)
        try:
            replay = st.capture(training=True)
            kernels = L.launch_log()
        finally:
            L.set_option('diag.launch_log', 0)
        torch.cuda.synchronize()
        calls = [c.name for c in rec.calls[n0:]]
        assert calls and kernels and 'gan_pool_exchange' not in calls
        logs.append((calls, kernels))
        del replay, st
        gc.collect()
    assert logs[0][0] == logs[1][0]
    assert logs[0][1] == logs[1][1]


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def _strict(p):
    return json.loads(open(p).read(), parse_constant=lambda s: pytest.fail(f"not strict JSON: {s} in {p}"))


def _image_dirs(tmp_path):
    from PIL import Image
    ex = np.load(os.path.join(ROOT, 'tests', 'golden', 'example_pairs_256.npz'))
    dx, dy = str(tmp_path / 'X'), str(tmp_path / 'Y')
    for d, key in ((dx, 'input_u8'), (dy, 'target_u8')):
        os.makedirs(d)
        for i in range(6):
            a = ex[key][i % 2, :, :, 0]
            Image.fromarray(np.roll(a[:, ::-1] if (i // 2) % 2 else a, 16 * (i // 4), 0), 'L').save(os.path.join(d, f"s{i}.png"))
    return dx, dy


def _run_cli(dx, dy, out, extra=()):
    """(--data-cache device: its jitter is drawn in the consuming thread, X before Y per batch, so two runs of one command see the
    same batches; the host cache's two decode threads share one generator and race for it.)"""
    from gan_amd import cycle_gan
    cycle_gan.main(cycle_gan.parse_opt(['--input-images', dx, '--target-images', dy, '--output', out, '--train', '--epochs', '1',
                                        '--test-img', '1', '--validation-size', '0.2', '--logging', 'false', '--data-cache', 'device', *extra]))
    logs = os.path.join(out, sorted(os.listdir(out))[0], 'logs')
    return _strict(os.path.join(logs, 'config.json')), _strict(os.path.join(logs, 'train_metrics.json'))


def test_cli_trains_with_a_pool(tmp_path):
    dx, dy = _image_dirs(tmp_path)
    config, metrics = _run_cli(dx, dy, str(tmp_path / 'out'), ['--pool-size', '2'])
    assert config['pool_size'] == 2
    assert metrics and all(len(v) == 1 and np.isfinite(v[0]) for v in metrics.values())


def test_cli_without_the_flag_is_the_run_without_pools(tmp_path, monkeypatch):
    """The same command twice: as it is, and with the step built by a constructor call that names pools=None itself."""
    from gan_amd import cycle_gan
    from gan_amd.steps import CycleGANStep
    dx, dy = _image_dirs(tmp_path)
    config, metrics = _run_cli(dx, dy, str(tmp_path / 'a'))
    assert config['pool_size'] == 0

    def build(self, batch, training):
        return CycleGANStep(self.ctx, batch, self.config['img_size'], int(self.config['channels']), lam=self.config['lambda'],
                            lr=self.config['learning_rate'], beta_1=self.config['beta_1'], beta_2=self.config['beta_2'],
                            seed=int(self.config.get('seed', 123)), mask_stream=0 if training else 16,
                            nets=tuple(m.net for m in self.networks()), gan_loss=self.config.get('gan_loss', 'bce'),
                            lr_schedule=self.lr_schedule if training else None, pools=None)
    monkeypatch.setattr(cycle_gan.CycleGAN, '_build_step', build)
    _, recorded = _run_cli(dx, dy, str(tmp_path / 'b'))
    assert metrics and metrics == recorded
