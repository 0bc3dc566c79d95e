"""fp64 references, gates, fp32 models and shared inputs of the least-squares GAN loss (gan_lsq_logits, gan_patchgan_losses_lsq;
DESIGN.md section 16), and the fp64 autograd references of one 'lsgan' training step per model (helper of tests/test_cpu_lsgan.py
and tests/test_gpu_lsgan.py; numpy and torch-CPU only, not a conftest).

The references are written from the formulas of include/gan_amd.h, not from the kernels:
    loss = mean((x - t)^2)                       dx = grad_scale * ls * 2 (x - t) / count
    gan  = mean((f - 1)^2)                       disc = 0.5 * (mean((r - 1)^2) + mean(f^2))
    g_dfake = 2 (f - 1) ls / n                   d_dreal = (r - 1) ls / n            d_dfake = f ls / n
The gates count roundings as tests/elementwise_ref.py does (EPS32 = one fp32 ulp of 1.0 per rounding); its helpers are called where
they apply as they are (block_partials, finalize_model, the caps arithmetic, ratio / ulp / K_ULP)."""
import functools
import math
import os
import re

import numpy as np
import torch

from gan_amd import _lib as L
from tests import elementwise_ref as E
from tests.launch_audit import EPS32, K_ULP, TDT, ratio, ulp

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR = {'gan_lsq_logits': 'gan_bce_logits', 'gan_patchgan_losses_lsq': 'gan_patchgan_losses'}       # new entry point -> the one it mirrors


# ---- launch arithmetic, read from the launch code -------------------------------------------------------------------------------
def source_cap(name):
    """The grid cap `if (blocks > N) blocks = N;` in the body of entry point `name` (gan_amd/csrc/elementwise.hip)."""
    src = open(os.path.join(ROOT, 'gan_amd', 'csrc', 'elementwise.hip')).read()
    body = src[src.index(f'int {name}('):]
    body = body[:body.index('\n}\n')]
    m = re.search(r'if \(blocks > (\d+)\) blocks = (\d+);', body)
    assert m and m.group(1) == m.group(2) and '(count + 255) / 256' in body and 'dim3(256)' in body, name
    return int(m.group(1))


CAPS = {name: (source_cap(name), 1) for name in PAIR}          # (block cap, elements per thread and trip), as elementwise_ref.CAPS


def cap_elems(name):
    return CAPS[name][0] * E.THREADS


def blocks_of(name, count):
    return min((count + E.THREADS - 1) // E.THREADS, CAPS[name][0])


def trips(name, count):
    per = blocks_of(name, count) * E.THREADS
    return (count + per - 1) // per


# ---- the GPU cases ------------------------------------------------------------------------------------------------------------------
# 1, 63 (below a wave), 257 (one past a block), 900 (one 30 x 30 map), and the smallest count whose grid-stride loop takes a
# second, ragged trip at the cap: one element more than the capped grid covers
LSQ_COUNTS = (1, 63, 257, 900, cap_elems('gan_lsq_logits') + 1)
FUSED_COUNTS = (1, 63, 257, 900, cap_elems('gan_patchgan_losses_lsq') + 1)
LS_ON, LS_SKIP = E.LS_ON, E.LS_SKIP
LAM, L1V = 100.0, 0.37


def logits(count, seed, shift=0.0):
    """elementwise_ref.logits: normal logits (sigma 3) with +-100, +-20, +-1e-6, +-0 planted at the head and, reversed, at the tail -
    the very last logit, the one a lost tail loses, is -100."""
    return E.logits(count, seed, shift)


lsq_args = E.bce_args          # (loss_scale, grad_scale): the generator term unscaled, a discriminator term halved (as the step calls it)


# ---- fp64 references ---------------------------------------------------------------------------------------------------------------
def lsq_ref(x32, target, grad_scale):
    """-> (mean((x - t)^2), grad_scale * 2 (x - t) / count), fp64.  grad_scale includes the dynamic loss scale."""
    d = x32.astype(np.float64) - float(target)
    return float((d * d).mean()), d * (2.0 * grad_scale / d.size)


def fused_ref(real32, fake32, ls0=1.0):
    gan, g_dfake = lsq_ref(fake32, 1.0, ls0)
    lr_, d_dreal = lsq_ref(real32, 1.0, 0.5 * ls0)
    lf, d_dfake = lsq_ref(fake32, 0.0, 0.5 * ls0)
    return dict(gan=gan, real=lr_, fake0=lf, disc=0.5 * (lr_ + lf), g_dfake=g_dfake, d_dreal=d_dreal, d_dfake=d_dfake)


# ---- gates ---------------------------------------------------------------------------------------------------------------------------
def grad_gate(ref, dt):
    """Stored gradient: K_ULP * ulp_dt(ref) + 3 * EPS32 * |ref|.
    K_ULP = 1 ulp of the storage type, as elementwise_ref.bce_grad_gate: the rounding to storage (half) and a reference on the
    other side of a binade edge (half).  The fp32 evaluation is a chain of products of x - t, so its error is RELATIVE (no
    cancellation: x and t are exact fp32 inputs, the subtraction rounds once): x - t, grad_scale * ls, the product, 1 / count and
    the last product = 5 roundings of half an ulp = 2.5 EPS32 |ref|, taken as 3 (float(count) beyond 2^24, second order)."""
    r = E.t64(ref)
    return K_ULP * ulp(r, dt) + 3 * EPS32 * r.abs()


def loss_gate(name, count, term_mean):
    """Loss scalar: EPS32 * (T + 10) * mean_i (x_i - t)^2, the form of elementwise_ref.loss_gate with this term's own count.
    T = additions per thread (trips of the capped grid); 10 = the subtraction and the square of the term (2, against the 8 of exp,
    log1p and three adds of cross-entropy) + the 6 shuffle levels + the 4-way block add (once) + the final conversion to float.
    Every term is >= 0, so a partial sum never exceeds the total.  The second stage sums in double and adds nothing."""
    return EPS32 * (trips(name, count) + 10) * term_mean


def _r(err, gate):
    return E._r(err, gate)


def _overflows(ref, gate, dt):
    """(must, may): elements whose correctly rounded stored value is +-inf whatever the gate allows / whose reference lies within
    the gate of the overflow threshold (largest finite value + half an ulp).  Only f16 gets there: 2 * ls * |x - t| / count
    beyond 65,504 - the gradient of an unbounded logit under a large loss scale, which the scale's inf check then sees."""
    fi = torch.finfo(TDT[dt])
    edge = fi.max + 0.5 * float(ulp(torch.tensor([fi.max], dtype=torch.float64), dt))
    a = E.t64(ref).abs()
    return a - gate > edge, (a + gate >= edge) & (a - gate <= edge)



def grad_ratio(got, ref, dt):
    """Worst |got - ref| / gate over the finite range; an element that must overflow must be the signed inf, one at the edge may be."""
    r = E.t64(ref)
    gate = grad_gate(ref, dt)
    must, may = _overflows(ref, gate, dt)
    g = got.double()
    inf_ok = torch.isinf(g) & (torch.sign(g) == torch.sign(r))
    if bool((must & ~inf_ok).any()):
        return math.inf
    fin = ~(must | (may & inf_ok))
    return ratio(got[fin], r[fin], gate[fin])


def check_lsq(x, target, grad_scale, ls0, dt, loss, grad, loss_scale=1.0):
    """loss: the fp32 scalar of a call with loss_accumulate = 0 (loss_scale a power of two: that multiply is exact); grad: the stored
    gradient [count] or None.  -> {item: error / gate}."""
    ref_l, ref_g = lsq_ref(x, target, grad_scale * ls0)
    res = {'loss': _r(abs(float(loss) - loss_scale * ref_l), abs(loss_scale) * loss_gate('gan_lsq_logits', x.size, ref_l))}
    if grad is not None:
        res['grad'] = grad_ratio(grad, ref_g, dt)
    return res


def check_accumulate(before, single, accumulated):
    """loss_accumulate = 1 on a loss_out that held `before`: exactly the fp32 sum of the two stored values (the launch is
    deterministic, `single` is the same call's loss with loss_accumulate = 0).  0 or inf."""
    want = F32(before) + F32(single)
    return 0.0 if F32(accumulated).view(np.uint32) == want.view(np.uint32) else math.inf


def check_fused(real, fake, ls0, dt, got, lam=LAM, l1=0.0):
    """got: dict with the fp32 scalars gan, disc, optionally gen_total, and the stored gradients g_dfake / d_dreal / d_dfake (or None).
    disc = 0.5 * (r + f) as elementwise_ref.check_patchgan: the two means each within their loss gate, halved exactly, plus the ONE
    rounding of the add.  gen_total: exactly the fp32 gan + lambda * l1 of the stored gan, two roundings."""
    ref = fused_ref(real, fake, ls0)
    n = real.size
    name = 'gan_patchgan_losses_lsq'
    gg, gr, gf = loss_gate(name, n, ref['gan']), loss_gate(name, n, ref['real']), loss_gate(name, n, ref['fake0'])
    res = {'gan': _r(abs(float(got['gan']) - ref['gan']), gg),
           'disc': _r(abs(float(got['disc']) - ref['disc']), 0.5 * (gr + gf) + 0.5 * EPS32 * abs(ref['disc']))}
    if got.get('gen_total') is not None:
        want = F32(got['gan']) + F32(lam) * F32(l1)
        res['gen_total'] = 0.0 if F32(got['gen_total']).view(np.uint32) == F32(want).view(np.uint32) else math.inf
    for k in ('g_dfake', 'd_dreal', 'd_dfake'):
        if got.get(k) is not None:
            res[k] = grad_ratio(got[k], ref[k], dt)
    return res


# ---- fp32 models: numpy float32 in the kernels' operation order, the launch code's block and grid decomposition --------------------
def lsq_model(x, target, grad_scale, ls0=1.0, loss_scale=1.0):
    """lsq_kernel + l1_finalize_kernel -> (loss fp32, fp32 gradient before the rounding to storage)."""
    d = (x - F32(target)).astype(F32)
    g2 = F32(2) * (F32(grad_scale) * F32(ls0))
    inv = F32(1) / F32(x.size)
    grad = ((g2 * d) * inv).astype(F32)
    return E.finalize_model(E.block_partials((d * d).astype(F32), blocks_of('gan_lsq_logits', x.size)), x.size, loss_scale), grad


def fused_model(real, fake, ls0=1.0, lam=LAM, l1=0.0):
    """patchgan_lsq_kernel + patchgan_finalize_kernel -> dict of fp32 scalars and fp32 gradients."""
    one, half = F32(1), F32(0.5)
    df, dr = (fake - one).astype(F32), (real - one).astype(F32)
    blocks = blocks_of('gan_patchgan_losses_lsq', real.size)
    g, rr, ff = (E.finalize_model(E.block_partials(t.astype(F32), blocks), real.size) for t in (df * df, dr * dr, fake * fake))
    inv = F32(ls0) / F32(real.size)
    return dict(gan=g, disc=half * rr + half * ff, gen_total=g + F32(lam) * F32(l1),
                g_dfake=((F32(2) * df) * inv).astype(F32), d_dreal=(dr * inv).astype(F32), d_dfake=(fake * inv).astype(F32))


def cast(x32, dt):
    return E.cast_ref(np.asarray(x32, dtype=F32), dt)


# ---- one 'lsgan' training step per model in fp64 (oracle.torch_ref's networks, the MSE terms, autograd) --------------------------------
def _mse(x, t):
    return ((x - t) ** 2).mean()


def p2p_setup(B=1, S=256, C=1):
    """Parameters, inputs and dropout masks of the Pix2Pix step case (as tests/test_gpu_step.py::_setup_p2p, at batch 1)."""
    from oracle import gan_oracle as O
    Gp, Dp = O.init_generator(C, seed=11), O.init_discriminator(C, True, seed=12)
    rng = np.random.default_rng(0)
    for P in (Gp, Dp):
        for k in P:
            if k.endswith(('.gamma', '.beta', '.bias')):
                P[k] = (P[k] + 0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    inp, tar = O.synthetic_pair(B, S, C, seed=123)
    return Gp, Dp, inp, tar, O.dropout_masks(B, S, seed=5)


@functools.lru_cache(maxsize=None)
def p2p_step_ref(lam=100.0):
    """-> dict: losses (gen_total, gan, l1, disc), gen, gG, gD, logit_max.  Computed once and shared; callers must not write to it."""
    from oracle import torch_ref as T
    Gp, Dp, inp, tar, masks = p2p_setup()
    G, D = T.params(Gp), T.params(Dp)
    x, y = T.t(inp), T.t(tar)
    gen = T.generator(G, x, 'batchnorm', [T.t(m) for m in masks])
    d_real, d_fake = T.discriminator(D, x, y, 'batchnorm'), T.discriminator(D, x, gen, 'batchnorm')
    gan = _mse(d_fake, 1.0)
    l1 = (y - gen).abs().mean()
    gen_total = gan + lam * l1
    disc = 0.5 * (_mse(d_real, 1.0) + _mse(d_fake, 0.0))
    gG = torch.autograd.grad(gen_total, list(G.values()), retain_graph=True)
    gD = torch.autograd.grad(disc, list(D.values()))
    return dict(losses=np.array([v.item() for v in (gen_total, gan, l1, disc)]), gen=gen.detach().numpy(),
                gG={k: g.numpy() for k, g in zip(G, gG)}, gD={k: g.numpy() for k, g in zip(D, gD)},
                logit_max=float(max(d_real.abs().max(), d_fake.abs().max())))


def cyc_setup(B=1, S=256, C=1):
    """Parameters, inputs and masks of the CycleGAN step case (as tests/test_gpu_step.py::test_cyclegan_train_step_parity)."""
    from oracle import gan_oracle as O
    n = 'instancenorm'
    Ps = [O.init_generator(C, n, seed=21), O.init_generator(C, n, seed=22),
          O.init_discriminator(C, False, n, seed=23), O.init_discriminator(C, False, n, seed=24)]
    rx, ry = O.synthetic_pair(B, S, C, seed=9)
    keys = ['fake_y', 'cycled_x', 'fake_x', 'cycled_y', 'same_x', 'same_y']
    return Ps, rx, ry, {k: O.dropout_masks(B, S, seed=40 + i) for i, k in enumerate(keys)}


@functools.lru_cache(maxsize=None)
def cyc_step_ref(lam=10.0):
    """-> dict: the 7 losses (gen_g, gen_f, cycle, total_g, total_f, disc_x, disc_y), fake_y, grads [Gg, Gf, Dx, Dy], logit_max."""
    from oracle import torch_ref as T
    Ps, rx, ry, masks = cyc_setup()
    Gg, Gf, Dx, Dy = (T.params(P) for P in Ps)
    x, y = T.t(rx), T.t(ry)
    mk = lambda k: [T.t(m) for m in masks[k]]
    n = 'instancenorm'
    fake_y = T.generator(Gg, x, n, mk('fake_y'))
    cycled_x = T.generator(Gf, fake_y, n, mk('cycled_x'))
    fake_x = T.generator(Gf, y, n, mk('fake_x'))
    cycled_y = T.generator(Gg, fake_x, n, mk('cycled_y'))
    same_x = T.generator(Gf, x, n, mk('same_x'))
    same_y = T.generator(Gg, y, n, mk('same_y'))
    d_rx, d_ry = T.discriminator(Dx, x, None, n), T.discriminator(Dy, y, None, n)
    d_fx, d_fy = T.discriminator(Dx, fake_x, None, n), T.discriminator(Dy, fake_y, None, n)
    gen_g, gen_f = _mse(d_fy, 1.0), _mse(d_fx, 1.0)
    cyc = lam * (x - cycled_x).abs().mean() + lam * (y - cycled_y).abs().mean()
    tot_g = gen_g + cyc + lam * 0.5 * (y - same_y).abs().mean()
    tot_f = gen_f + cyc + lam * 0.5 * (x - same_x).abs().mean()
    dxl = 0.5 * (_mse(d_rx, 1.0) + _mse(d_fx, 0.0))
    dyl = 0.5 * (_mse(d_ry, 1.0) + _mse(d_fy, 0.0))
    grads = [torch.autograd.grad(l, list(P.values()), retain_graph=True) for l, P in ((tot_g, Gg), (tot_f, Gf), (dxl, Dx), (dyl, Dy))]
    return dict(losses=np.array([v.item() for v in (gen_g, gen_f, cyc, tot_g, tot_f, dxl, dyl)]), fake_y=fake_y.detach().numpy(),
                grads=[{k: g.numpy() for k, g in zip(P, gs)} for P, gs in zip((Gg, Gf, Dx, Dy), grads)],
                logit_max=float(max(t.abs().max() for t in (d_rx, d_ry, d_fx, d_fy))))
