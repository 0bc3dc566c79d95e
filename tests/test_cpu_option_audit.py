"""The device-free halves of the option checkers of tests/launch_audit.py (dssim_ratios, msssim_ratios, edge_ratios, diffaug_draw_ratios,
diffaug_apply_ratios, lsq_ratios, fused_lsq_ratios, pool_ratios, adam_begin_sched_ratios) on the CPU, on lattice inputs laid out as
the option-carrying steps lay them out: pitch-8 pixels, the target at channel offset C, f32 / bf16 / f16 at channels 1 and 3.

Must pass: the reference's own result rounded to the storage type (for the edge term the header's rounding order, for the least-squares
terms and the schedule the fp32 / double models of their stand-alone CPU tests) stays inside every gate, and the edge term's excluded
share on these inputs is at most 1 %.

Must fail: what a wiring or scaling bug of the step would leave in memory -
  - the edge or secondary loss taken against the augmented target instead of the raw one;
  - the edge gradient stored instead of accumulated;
  - the gradient not multiplied by the loss-scale word, and the loss multiplied by it;
  - the transpose run with sample0 = 0 instead of B;
  - one pad channel changed;
  - a 2-ulp error in one element of da (the edge gradient, held bit for bit, at every dtype; the dSSIM gradient at its largest
    element for the 16-bit types - its gate is the stand-alone test's max-norm one, 8 float32 yardsticks + one storage ulp, which at
    fp32 storage is wider than two fp32 ulps by construction);
  - a table drawn with the counter one off;
  - the pool state advanced without the swap;
  - MS-SSIM (test_msssim_compare; 45 x 47 at three scales: odd sides pooled on every level; a = clip(b + 0.1 U), the operands its loss
    gate is derived for): the above, and the gradient stored where it should accumulate and the reverse, the loss word stored where it
    should accumulate, the gradient of one level fewer, and independent operands, which must fail the premise row.
And the rule by which unchecked calls earn "as in the one-GPU step" (same_as_plain) accepts the intended sequence and rejects an extra
or a reordered launch."""
import math

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from tests import diffaug_ref as DR
from tests import dssim_ref, edge_ref, lr_schedule_ref, lsgan_ref, msssim_ref, pool_ref
from tests import elementwise_ref as E
from tests import launch_audit as A

DTS = ['f32', 'bf16', 'f16']
CODE = {'f32': L.F32, 'bf16': L.BF16, 'f16': L.F16}
B, H, W = 2, 24, 20
LS = 1024.0
ALL = DR.POLICIES


def stored(x, dt):
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).to(torch.float32).to(A.TDT[CODE[dt]])


def embed(real, c0, fill=0.0):
    """[n,h,w,c] -> whole pitch-8 pixels with the view at channel c0"""
    n, h, w, c = real.shape
    raw = torch.full((n, h, w, 8), fill, dtype=real.dtype)
    raw[..., c0:c0 + c] = real
    return raw


def failed(res):
    return [k for k, v in res.items() if not v <= 1.0]


def pair(dt, c, seed=3):
    """(generator output, target): a smooth-ish image in (-1, 1) and a lattice one, as stored."""
    a = np.tanh(1.5 * np.random.default_rng(seed).standard_normal((B, H, W, c)))
    return stored(a, dt), stored(A.lattice((B, H, W, c), seed + 1).numpy(), dt)


def fields(dt, ls, **kw):
    f = dict(loss_scale=1.0, loss_accumulate=0, grad_scale=100.0, ls=ls, dtype_da=CODE[dt], grad_accumulate=0)
    f.update(kw)
    return f


def ls_of(dt):
    return LS if dt == 'f16' else None


# ---- the two image losses -----------------------------------------------------------------------------------------------------------
def dssim_model(a, b, dt, f, ls_in_grad=True, ls_in_loss=False):
    loss, g = dssim_ref.loss_and_grad(a.double().numpy(), b.double().numpy())
    s = f['ls'] if f['ls'] is not None else 1.0
    da = stored(g.numpy() * f['grad_scale'] * (s if ls_in_grad else 1.0), dt)
    return da, float(np.float32(f['loss_scale'] * loss * (s if ls_in_loss else 1.0)))


def edge_model(a, b, dt, f, old, loss0, ls_in_grad=True, ls_in_loss=False, accumulate=True):
    from tests.test_gpu_edge import expected_grad
    a64, b64 = a.double().numpy(), b.double().numpy()
    s = f['ls'] if f['ls'] is not None else 1.0
    da = expected_grad(edge_ref.k_map(a64, b64), f['grad_scale'], tuple(a.shape), dt, ls=f['ls'] if ls_in_grad else None,
                       old=old if accumulate else None)
    term = np.float32(np.float32(edge_ref.loss(a64, b64)) * np.float32(f['loss_scale'] * (s if ls_in_loss else 1.0)))
    return da, float(np.float32(loss0) + term)


def augmented(b, dt, c):
    H, W = b.shape[1], b.shape[2]
    recs = DR.draw(123, 5, 48, 2 * B, H, W, ALL)
    return stored(DR.forward(b.double(), recs, c, 0).numpy(), dt)


def bump(t, idx, ulps):
    """t[idx] moved by `ulps` units in the last place of its storage type."""
    out = t.clone()
    bits = A._bits(out)                                   # (a view: same storage)
    flat = bits.view(-1)
    i = int(np.ravel_multi_index(idx, tuple(t.shape)))
    flat[i] += ulps if flat[i] >= 0 else -ulps
    return bits.view(t.dtype).reshape(t.shape)


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('dt', DTS)
def test_dssim_compare(dt, c):
    a, b = pair(dt, c)
    f = fields(dt, ls_of(dt))
    da0 = embed(torch.zeros_like(a), 0)
    da, loss = dssim_model(a, b, dt, f)
    res = A.dssim_ratios(a, b, da0, embed(da, 0), 0, 0.0, loss, f)
    print(f"dssim {dt} c{c}: {res}")
    assert not failed(res), res
    # the loss taken against the augmented target
    da_x, loss_x = dssim_model(a, augmented(b, dt, c), dt, f)
    assert {'da', 'loss'} <= set(failed(A.dssim_ratios(a, b, da0, embed(da_x, 0), 0, 0.0, loss_x, f)))
    if f['ls'] is not None:       # the scale word on the loss instead of the gradient
        da_x, loss_x = dssim_model(a, b, dt, f, ls_in_grad=False, ls_in_loss=True)
        assert {'da', 'loss'} <= set(failed(A.dssim_ratios(a, b, da0, embed(da_x, 0), 0, 0.0, loss_x, f)))
    pad = embed(da, 0)
    pad[1, 3, 4, c] = 1.0
    assert failed(A.dssim_ratios(a, b, da0, pad, 0, 0.0, loss, f)) == ['da untouched outside the view']
    if dt != 'f32':               # (module docstring)
        top = np.unravel_index(int(da.double().abs().argmax()), tuple(da.shape))
        assert failed(A.dssim_ratios(a, b, da0, embed(bump(da, top, 2), 0), 0, 0.0, loss, f)) == ['da']
    # loss_accumulate is honoured
    fa = dict(f, loss_accumulate=1, loss_scale=0.5)
    _, l2 = dssim_model(a, b, dt, fa)
    assert not failed(A.dssim_ratios(a, b, da0, embed(da, 0), 0, 2.0, float(np.float32(2.0) + np.float32(l2)), fa))
    assert 'loss' in failed(A.dssim_ratios(a, b, da0, embed(da, 0), 0, 2.0, l2, fa))


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('dt', DTS)
def test_edge_compare(dt, c):
    a, b = pair(dt, c)
    f = fields(dt, ls_of(dt), loss_scale=0.25, loss_accumulate=1, grad_scale=25.0, grad_accumulate=1)
    old, loss0 = dssim_model(a, b, dt, fields(dt, ls_of(dt)))              # what the secondary loss left in g.dgen and losses[2]
    da0 = embed(old, 0)
    da, loss = edge_model(a, b, dt, f, old, loss0)
    res = A.edge_ratios(a, b, da0, embed(da, 0), 0, loss0, loss, f)
    print(f"edge {dt} c{c}: {res}")
    assert not failed(res), res
    assert res['excluded share / 1 %'] <= 1.0
    run = lambda da_, loss_: failed(A.edge_ratios(a, b, da0, embed(da_, 0), 0, loss0, loss_, f))
    assert {'da (bits)', 'loss'} <= set(run(*edge_model(a, augmented(b, dt, c), dt, f, old, loss0)))
    assert run(*edge_model(a, b, dt, f, old, loss0, accumulate=False)) == ['da (bits)']              # stored, not accumulated
    if f['ls'] is not None:
        assert {'da (bits)', 'loss'} <= set(run(*edge_model(a, b, dt, f, old, loss0, ls_in_grad=False, ls_in_loss=True)))
    pad = embed(da, 0)
    pad[0, 0, 0, 7] = -1.0
    assert failed(A.edge_ratios(a, b, da0, pad, 0, loss0, loss, f)) == ['da untouched outside the view']
    mask = edge_ref.min_response(a.double().numpy(), b.double().numpy()) >= A.EDGE_MARGIN
    idx = tuple(int(v) for v in np.argwhere(mask)[len(np.argwhere(mask)) // 2])
    assert run(bump(da, idx, 2), loss) == ['da (bits)']                                              # a 2-ulp error in one element
    assert run(da, float(np.float32(loss) * np.float32(1.0 + 4096 * 2.0 ** -24))) == ['loss']


# ---- MS-SSIM ---------------------------------------------------------------------------------------------------------------------------
MH, MW, MS = 45, 47, 3               # odd sides on every level (45 x 47, 23 x 24, 12 x 12), the smallest with three
M_AMP = 0.1                          # tests/test_gpu_msssim.py::AMPS[0]


def msssim_pair(dt, c, seed=3):
    """(a, b) as stored: b a tanh-noise image, a = clip(b + 0.1 U(-1, 1)) - the generator's output near its target."""
    rng = np.random.default_rng(seed)
    b = np.tanh(1.5 * rng.standard_normal((B, MH, MW, c)))
    return stored(np.clip(b + M_AMP * rng.uniform(-1, 1, b.shape), -1, 1), dt), stored(b, dt)


def msssim_model(a, b, dt, f, old=None, loss0=None, ls_in_grad=True, ls_in_loss=False, scales=None):
    """The reference's own result as the kernel leaves it: da = round_storage([float(old) +] grad_scale * ls * g), loss word =
    fp32([loss0 +] loss_scale * loss).  old / loss0: what da / the loss word held (None: stored, not accumulated)."""
    M = f['scales']
    loss, _, _ = msssim_ref.loss_and_grad(a.double().numpy(), b.double().numpy(), M, f['power'])
    m = scales or M
    _, g, _ = msssim_ref.loss_and_grad(a.double().numpy(), b.double().numpy(), m, f['power'][:m])
    s = f['ls'] if f['ls'] is not None else 1.0
    g = g.numpy() * f['grad_scale'] * (s if ls_in_grad else 1.0)
    da = stored(g + (old.double().numpy() if old is not None else 0.0), dt)
    term = np.float32(f['loss_scale'] * loss * (s if ls_in_loss else 1.0))
    return da, float(np.float32(loss0) + term if loss0 is not None else term)


@pytest.mark.parametrize('ls', [None, LS], ids=['unscaled', 'loss-scale'])
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('dt', DTS)
def test_msssim_compare(dt, c, ls):
    a, b = msssim_pair(dt, c)
    power = tuple(float(np.float32(p)) for p in msssim_ref.POWER[:MS])
    f = dict(fields(dt, ls), scales=MS, power=power)
    fa = dict(f, loss_scale=0.84, loss_accumulate=1, grad_scale=84.0, grad_accumulate=1)         # the call of 'msssim_l1'
    # what gan_l1 left in front of the accumulating call: (1 - alpha) * lambda * ls * sign / count, and its loss word
    k1 = 16.0 * (ls or 1.0) / a.numel()
    old = stored(k1 * np.sign(b.double().numpy() - a.double().numpy()), dt)
    loss0 = float(np.float32(0.16 * np.abs(b.double().numpy() - a.double().numpy()).mean()))
    assert bool(old.double().abs().max() > 0) and loss0 > 0
    z = embed(torch.zeros_like(a), 0)
    da, loss = msssim_model(a, b, dt, f)
    res = A.msssim_ratios(a, b, z, embed(da, 0), 0, 0.0, loss, f)
    print(f"msssim {dt} c{c} ls {ls} storing: {res} (smallest factor {A.MSSSIM_PREMISE / res['premise']:.3f})")
    assert not failed(res), res
    da_a, loss_a = msssim_model(a, b, dt, fa, old, loss0)
    res = A.msssim_ratios(a, b, embed(old, 0), embed(da_a, 0), 0, loss0, loss_a, fa)
    print(f"msssim {dt} c{c} ls {ls} accumulating: {res}")
    assert not failed(res), res
    store = lambda da_, loss_, f_=f: failed(A.msssim_ratios(a, b, z, embed(da_, 0), 0, 0.0, loss_, f_))
    accum = lambda da_, loss_: failed(A.msssim_ratios(a, b, embed(old, 0), embed(da_, 0), 0, loss0, loss_, fa))
    # the loss and gradient taken against the augmented target
    assert {'da', 'loss'} <= set(store(*msssim_model(a, augmented(b, dt, c), dt, f)))
    assert {'da', 'loss'} <= set(accum(*msssim_model(a, augmented(b, dt, c), dt, fa, old, loss0)))
    # stored where it should accumulate, accumulated where it should store: the gradient, then the loss word
    assert accum(msssim_model(a, b, dt, fa)[0], loss_a) == ['da']
    assert failed(A.msssim_ratios(a, b, embed(old, 0), embed(msssim_model(a, b, dt, f, old)[0], 0), 0, loss0, loss, f)) == ['da']
    assert accum(da_a, msssim_model(a, b, dt, fa)[1]) == ['loss']
    assert failed(A.msssim_ratios(a, b, z, embed(da, 0), 0, 2.0, msssim_model(a, b, dt, f, loss0=2.0)[1], f)) == ['loss']
    if ls is not None:            # the scale word on the loss instead of the gradient
        assert {'da', 'loss'} <= set(store(*msssim_model(a, b, dt, f, ls_in_grad=False, ls_in_loss=True)))
        assert {'da', 'loss'} <= set(accum(*msssim_model(a, b, dt, fa, old, loss0, ls_in_grad=False, ls_in_loss=True)))
    # one level fewer: one level's pooling transpose dropped
    assert store(msssim_model(a, b, dt, f, scales=MS - 1)[0], loss) == ['da']
    assert accum(msssim_model(a, b, dt, fa, old, loss0, scales=MS - 1)[0], loss_a) == ['da']
    pad = embed(da, 0)
    pad[1, 3, 4, c] = 1.0
    assert store(pad, loss) == ['da untouched outside the view']
    pad = embed(da_a, 0)
    pad[0, MH - 1, MW - 1, 7] = -1.0
    assert failed(A.msssim_ratios(a, b, embed(old, 0), pad, 0, loss0, loss_a, fa)) == ['da untouched outside the view']
    if dt != 'f32':               # (module docstring: as the dSSIM gradient, at fp32 the max-norm gate is wider than two ulps by construction)
        top = np.unravel_index(int(da.double().abs().argmax()), tuple(da.shape))
        assert store(bump(da, top, 2), loss) == ['da']
    # independent operands: the gate's premise does not hold, and the row says so
    ind = stored(A.lattice((B, MH, MW, c), 4).numpy(), dt)
    da_i, loss_i = msssim_model(b, ind, dt, f)                # (the tanh image against a lattice one, with the reference's own result)
    res = A.msssim_ratios(b, ind, z, embed(da_i, 0), 0, 0.0, loss_i, f)
    print(f"msssim {dt} c{c} independent operands: smallest factor {A.MSSSIM_PREMISE / res['premise']:.4f}")
    assert 'premise' in failed(res), res


# ---- DiffAugment ----------------------------------------------------------------------------------------------------------------------
def test_draw_compare():
    f = dict(n=2 * B, h=256, w=256, policy=15, seed=123, stream_id=48)
    t0 = np.full((A.AUG_RECORDS, 8), A.AUG_FILL, dtype=np.int32)
    mk = lambda counter: np.concatenate([DR.table(DR.draw(123, counter, 48, 2 * B, 256, 256, ALL)), t0[2 * B:]])
    assert not failed(A.diffaug_draw_ratios(t0, 5, mk(5), 6, f))
    assert failed(A.diffaug_draw_ratios(t0, 5, mk(6), 6, f)) == ['table (bits)']                     # drawn with the counter one off
    assert failed(A.diffaug_draw_ratios(t0, 5, mk(4), 6, f)) == ['table (bits)']
    assert failed(A.diffaug_draw_ratios(t0, 5, mk(5), 5, f)) == ['counter + 1']
    t1 = mk(5)
    t1[2 * B, 3] = 0
    assert failed(A.diffaug_draw_ratios(t0, 5, t1, 6, f)) == ['records past n unchanged']
    assert failed(A.diffaug_draw_ratios(t0, 5, mk(5), 6, dict(f, policy=7))) == ['table (bits)']     # saturation not drawn


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('dt', DTS)
def test_apply_compare(dt, c):
    recs = DR.draw(123, 5, 48, 2 * B, H, W, ALL)
    assert any(p['tx'] or p['ty'] for p in recs[B:]) and recs[:B] != recs[B:]
    sentinel = 0.5
    # forward: the real [input | target] pair (two images per sample), and the generated channels at offset c with records B ..
    for src, c0, s0 in ((stored(A.lattice((B, H, W, 2 * c), 9).numpy(), dt), 0, 0), (pair(dt, c)[0], c, B)):
        f = dict(group_c=c, sample0=s0, direction=0, dtype=CODE[dt])
        want = stored(DR.forward(src.double(), recs, c, s0).numpy() + 0.0, dt)
        dst0 = embed(torch.full_like(want, sentinel), c0)
        res = A.diffaug_apply_ratios(src, dst0, embed(want, c0), c0, recs, f)
        print(f"apply forward {dt} c{c} sample0 {s0}: {res}")
        assert not failed(res), res
        wrong = stored(DR.forward(src.double(), recs, c, B - s0).numpy() + 0.0, dt)                 # the other half's records
        assert 'dst' in failed(A.diffaug_apply_ratios(src, dst0, embed(wrong, c0), c0, recs, f))
        pad = embed(want, c0)
        pad[0, 1, 1, 7] = 1.0
        assert failed(A.diffaug_apply_ratios(src, dst0, pad, c0, recs, f)) == ['dst untouched outside the view']
    # backward: aug_dgen -> g.dgen2 with records B ..
    dy = stored(np.random.default_rng(4).standard_normal((B, H, W, c)) * 3.0, dt)
    f = dict(group_c=c, sample0=B, direction=1, dtype=CODE[dt])
    want = stored(DR.transpose(dy.double().numpy(), recs, c, B), dt)
    dst0 = embed(torch.full_like(want, sentinel), 0)
    res = A.diffaug_apply_ratios(dy, dst0, embed(want, 0), 0, recs, f)
    print(f"apply backward {dt} c{c}: {res}")
    assert not failed(res), res
    wrong = stored(DR.transpose(dy.double().numpy(), recs, c, 0), dt)                                # sample0 = 0 instead of B
    bad = failed(A.diffaug_apply_ratios(dy, dst0, embed(wrong, 0), 0, recs, f))
    assert bad and set(bad) <= {'dst', 'dst where bits move', 'fill is +0'}, bad
    neg = embed(want, 0)
    fill = np.argwhere(want.double().numpy() == 0)[0]
    neg[tuple(fill)] = -0.0
    assert 'fill is +0' in failed(A.diffaug_apply_ratios(dy, dst0, neg, 0, recs, f)) or bool(dy[tuple(fill)] == 0)


# ---- least squares ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTS)
def test_lsq_compare(dt):
    x = E.logits(900, 1)
    ls = ls_of(dt)
    col = lambda g: embed(lsgan_ref.cast(g, CODE[dt]).reshape(-1, 1, 1, 1), 0).reshape(-1, 8)
    for target, acc, loss0 in ((1.0, 0, 0.0), (0.0, 1, 0.375)):
        lscale, gscale = lsgan_ref.lsq_args(target)
        f = dict(target=target, loss_scale=lscale, loss_accumulate=acc, grad_scale=gscale, dtype=CODE[dt], ls=ls)
        loss, grad = lsgan_ref.lsq_model(x, target, gscale, ls or 1.0, lscale)
        loss1 = float(np.float32(loss0) + loss) if acc else float(loss)
        dx0 = col(np.zeros_like(grad))
        res = A.lsq_ratios(x, f, loss0, loss1, dx0, col(grad))
        print(f"lsq {dt} target {target}: {res}")
        assert not failed(res), res
        assert 'loss' in failed(A.lsq_ratios(x, f, loss0, float(loss) + (0.0 if acc else 0.375), dx0, col(grad)))   # stored / accumulated, swapped
        if ls is not None:
            _, g1 = lsgan_ref.lsq_model(x, target, gscale, 1.0, lscale)
            assert 'grad' in failed(A.lsq_ratios(x, f, loss0, loss1, dx0, col(g1)))
        pad = col(grad)
        pad[5, 3] = 1.0
        assert failed(A.lsq_ratios(x, f, loss0, loss1, dx0, pad)) == ['dx untouched beside the elements']
    real, fake = E.logits(900, 2), E.logits(900, 3, 0.5)
    m = lsgan_ref.fused_model(real, fake, ls or 1.0, 100.0, 0.37)
    f = dict(dtype=CODE[dt], ls=ls, lam=100.0, l1=0.37)
    names = ('g_dfake', 'd_dreal', 'd_dfake')
    g0 = {k: col(np.zeros(900, np.float32)) for k in names}
    got = {k: float(m[k]) for k in ('gan', 'disc', 'gen_total')}
    res = A.fused_lsq_ratios(real, fake, f, got, g0, {k: col(m[k]) for k in names})
    print(f"fused lsq {dt}: {res}")
    assert not failed(res), res
    swapped = {'g_dfake': col(m['g_dfake']), 'd_dreal': col(m['d_dfake']), 'd_dfake': col(m['d_dreal'])}
    assert {'d_dreal', 'd_dfake'} <= set(failed(A.fused_lsq_ratios(real, fake, f, got, g0, swapped)))
    assert 'gen_total' in failed(A.fused_lsq_ratios(real, fake, dict(f, l1=0.5), got, g0, {k: col(m[k]) for k in names}))


# ---- image pool -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('dt', DTS)
def test_pool_compare(dt, c):
    cap, seed = A.POOL_CAPACITY, 123
    src = stored(A.lattice((1, H, W, c), 5).numpy(), dt)
    pool0 = stored(A.lattice((cap, H, W, c), 6).numpy(), dt)
    dst0 = embed(torch.full_like(src, 0.5), 0)
    for sid, want in ((pool_ref.STREAM_Y, 'swap'), (pool_ref.STREAM_X, 'keep')):
        k = A.pool_launches(1, cap, seed, sid, want)
        state0 = [cap, k, 0]
        out, pool, state, trace = pool_ref.query(A._bits(src).numpy(), A._bits(pool0).numpy(), state0[:2], seed, sid)
        assert trace[0][0] == want
        tt = lambda bits: torch.from_numpy(bits).view(src.dtype)
        f = dict(seed=seed, stream_id=sid)
        res, tr = A.pool_ratios(src, pool0, state0, dst0, embed(tt(out), 0), 0, tt(pool), list(state) + [0], f)
        assert not failed(res) and tr == trace, res
        # the state advanced, nothing moved
        bad = failed(A.pool_ratios(src, pool0, state0, dst0, embed(src, 0), 0, pool0, list(state) + [0], f)[0])
        assert bad == (['dst (bits)', 'pool (bits)'] if want == 'swap' else []), bad
        assert failed(A.pool_ratios(src, pool0, state0, dst0, embed(tt(out), 0), 0, tt(pool), state0, f)[0]) == ['state']
        assert failed(A.pool_ratios(src, pool0, state0, dst0, embed(tt(out), 0), 0, tt(pool), list(state) + [1], f)[0]) == ['state']
        pad = embed(tt(out), 0)
        pad[0, 2, 2, c] = 1.0
        assert failed(A.pool_ratios(src, pool0, state0, dst0, pad, 0, tt(pool), list(state) + [0], f)[0]) == ['dst untouched outside the view']


# ---- learning-rate schedule ------------------------------------------------------------------------------------------------------------
def test_adam_begin_sched_compare():
    ds, de, ef = lr_schedule_ref.STEP_SCHEDULE
    f = dict(lr=2e-4, end_factor=ef, decay_start=ds, decay_end=de, beta1=0.5, beta2=0.999)
    for step0 in (0, A.SCHED_STEP0, 5):
        lr_t, lr_now = lr_schedule_ref.model(2e-4, ef, ds, de, 0.5, 0.999, step0 + 1)
        assert not failed(A.adam_begin_sched_ratios(step0, np.float32(0), np.float32(2e-4), False, step0 + 1, lr_t, lr_now, f))
        assert failed(A.adam_begin_sched_ratios(step0, np.float32(0), np.float32(2e-4), False, step0, lr_t, lr_now, f)) == ['step + 1']
    lr_t, lr_now = lr_schedule_ref.model(2e-4, ef, ds, de, 0.5, 0.999, A.SCHED_STEP0 + 1)
    assert float(lr_now) == float(np.float32(np.float32(2e-4) * 0.5))                                # the known start runs at lr / 2
    plain_t, plain_now = lr_schedule_ref.model(2e-4, ef, lr_schedule_ref.OFF_START, lr_schedule_ref.OFF_START + 1, 0.5, 0.999, A.SCHED_STEP0 + 1)
    bad = failed(A.adam_begin_sched_ratios(A.SCHED_STEP0, np.float32(0), np.float32(2e-4), False, A.SCHED_STEP0 + 1, plain_t, plain_now, f))
    assert bad == ['lr_t', 'lr_now']                                                                 # the schedule ignored
    # a skipped fp16 step keeps the counter and both rates
    keep = (np.float32(1e-4), np.float32(2e-4))
    assert not failed(A.adam_begin_sched_ratios(3, *keep, True, 3, *keep, f))
    assert failed(A.adam_begin_sched_ratios(3, *keep, True, 4, lr_t, lr_now, f)) == ['step kept', 'lr_t kept', 'lr_now kept']


# ---- the rule of the unchecked calls ---------------------------------------------------------------------------------------------------
def test_the_striking_and_mapping_rule():
    K1, K2 = ('conv', 0, 64, 64), ('conv', 1, 0, 16)
    plain = [('gan_pack_multi', None), ('gan_conv2d_fwd', K1), ('gan_l1', None), ('gan_copy_view', None), ('gan_conv2d_fwd', K1),
             ('gan_patchgan_losses', None), ('gan_conv2d_dgrad', K2), ('gan_adam_begin', None), ('gan_conv_wgrad', ('wgrad', 1))]
    option = [('gan_pack_multi', None), ('gan_diffaug_draw', None), ('gan_diffaug_apply', A.ANY), ('gan_conv2d_fwd', K1),
              ('gan_diffaug_apply', A.ANY), ('gan_dssim', A.ANY), ('gan_edge_l1', A.ANY), ('gan_diffaug_apply', A.ANY), ('gan_conv2d_fwd', K1),
              ('gan_patchgan_losses_lsq', A.ANY), ('gan_conv2d_dgrad', A.ANY), ('gan_diffaug_apply', A.ANY), ('gan_adam_begin_sched', A.ANY),
              ('gan_conv_wgrad', ('wgrad', 1))]
    assert not A.same_as_plain(option, plain, replaced_copy=3)
    assert A.same_as_plain(option, plain)                                                            # the copy not struck
    extra = option[:4] + [('gan_copy_view', None)] + option[4:]
    assert A.same_as_plain(extra, plain, replaced_copy=3)                                            # an extra launch
    swapped = list(option)
    swapped[8], swapped[9] = swapped[9], swapped[8]
    assert A.same_as_plain(swapped, plain, replaced_copy=3)                                          # a reordered launch
    other = [(n, ('conv', 9) if k == K1 else k) for n, k in option]
    assert A.same_as_plain(other, plain, replaced_copy=3)                                            # an unchecked call of another plan class
    pools_plain = [('gan_copy_view', None), ('gan_conv2d_fwd', K1), ('gan_bce_logits', None), ('gan_bce_logits', None)]
    pools = [('gan_copy_view', None), ('gan_pool_exchange', A.ANY), ('gan_conv2d_fwd', A.ANY), ('gan_lsq_logits', A.ANY), ('gan_lsq_logits', A.ANY)]
    assert not A.same_as_plain(pools, pools_plain)
    assert A.same_as_plain(pools[:-1], pools_plain)


def test_the_rule_places_gan_msssim_by_the_generator_loss():
    K1 = ('conv', 0, 64, 64)
    plain = [('gan_pack_multi', None), ('gan_conv2d_fwd', K1), ('gan_l1', None), ('gan_copy_view', None), ('gan_conv2d_fwd', K1),
             ('gan_patchgan_losses', None)]
    ms, l1, edge = ('gan_msssim', A.ANY), ('gan_l1', None), ('gan_edge_l1', A.ANY)
    seq = lambda *sec: plain[:2] + list(sec) + plain[3:]
    # 'msssim': gan_msssim stands where gan_l1 stood; 'msssim_l1': gan_l1 stays, gan_msssim is the extra call behind it
    assert not A.same_as_plain(seq(ms), plain, msssim='msssim') and not A.same_as_plain(seq(ms, edge), plain, msssim='msssim')
    assert not A.same_as_plain(seq(l1, ms), plain, msssim='msssim_l1') and not A.same_as_plain(seq(l1, ms, edge), plain, msssim='msssim_l1')
    # the place is the caller's to name: the other place, or none, does not fit
    assert A.same_as_plain(seq(ms), plain, msssim='msssim_l1') and A.same_as_plain(seq(l1, ms), plain, msssim='msssim')
    assert A.same_as_plain(seq(ms), plain) and A.same_as_plain(seq(l1, ms), plain)
    assert A.same_as_plain(seq(l1), plain, msssim='msssim') and A.same_as_plain(seq(l1), plain, msssim='msssim_l1')      # no gan_msssim at all
    assert A.same_as_plain(seq(ms, edge), plain, msssim='msssim_l1')                                 # 'msssim_l1' without its gan_l1
    assert A.same_as_plain(seq(ms, ms), plain, msssim='msssim')                                      # a second gan_msssim
    assert A.same_as_plain(seq(l1, ms, ms), plain, msssim='msssim_l1') and A.same_as_plain(seq(l1, ms, edge, ms), plain, msssim='msssim_l1')
    assert A.same_as_plain(seq(edge, ms), plain, msssim='msssim')                                    # recorded after the edge term
    assert A.same_as_plain(seq(l1, edge, ms), plain, msssim='msssim_l1')
    assert A.same_as_plain(seq(ms, l1), plain, msssim='msssim_l1')                                   # in front of its gan_l1
    with pytest.raises(AssertionError):
        A.same_as_plain(seq(ms), plain, msssim='dssim')


def test_every_option_entry_point_has_a_checker_and_a_plan():
    assert set(A.OPTION_ENTRIES) <= set(A.CHECKERS) and set(A.OPTION_ENTRIES) == set(A.OPTION_PLANS)
    assert not set(A.OPTION_ENTRIES) & set(A.ALLOWLIST)
    assert set(A.OPTION_MAP) | set(A.OPTION_STRUCK) == set(A.OPTION_ENTRIES)
    assert all(v in A.ALLOWLIST for v in A.OPTION_MAP.values())
    assert math.isinf(A.pixels_outside(torch.zeros(2, 8), torch.tensor([[0.0] * 8, [0.0] * 7 + [-0.0]]), 0, 3))     # -0.0 is a changed bit
