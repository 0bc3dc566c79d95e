"""CPU side of the least-squares GAN loss checks (tests/lsgan_ref.py, tests/test_gpu_lsgan.py).  Without a
GPU it shows:
  - the fp64 references agree with torch autograd of ((x - t) ** 2).mean();
  - every gate passes a float32 model of its kernel (the launch code's block and grid decomposition) on the exact inputs of every
    GPU case, for bf16, f16 and f32, with a margin of two;
  - every gate rejects the named wrong variants by a factor of two on at least one item;
  - the header declares both entry points with the argument lists of the cross-entropy ones, _lib.py binds them;
  - both command lines accept --gan-loss."""
import math
import os
import re

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from tests import elementwise_ref as E
from tests import lsgan_ref as R

F32 = np.float32
DTS = (L.F32, L.BF16, L.F16)
NAME = {L.F32: 'f32', L.BF16: 'bf16', L.F16: 'f16'}
MODEL_MAX = 0.5           # a faithful fp32 model stays within half of every gate
MUTANT_MIN = 2.0          # a wrong variant lands at least twice outside


def _pair(count):
    return R.logits(count, count), R.logits(count, count + 1, -0.5)


def test_references_agree_with_autograd():
    x = R.logits(900, 1)
    for t in (1.0, 0.0):
        loss, grad = R.lsq_ref(x, t, 1.0)
        xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        l = ((xt - t) ** 2).mean()
        l.backward()
        assert abs(loss - l.item()) <= 1e-14 * abs(loss) and np.abs(grad - xt.grad.numpy()).max() <= 1e-15 * np.abs(grad).max()
    real, fake = _pair(900)
    ref = R.fused_ref(real, fake, 1.0)
    r = torch.from_numpy(real.astype(np.float64)).requires_grad_(True)
    f = torch.from_numpy(fake.astype(np.float64)).requires_grad_(True)
    gan = ((f - 1.0) ** 2).mean()
    disc = 0.5 * (((r - 1.0) ** 2).mean() + ((f - 0.0) ** 2).mean())
    (g_dfake,) = torch.autograd.grad(gan, [f])
    d_dreal, d_dfake = torch.autograd.grad(disc, [r, f])
    assert abs(ref['gan'] - gan.item()) <= 1e-14 * ref['gan'] and abs(ref['disc'] - disc.item()) <= 1e-14 * ref['disc']
    for k, a in (('g_dfake', g_dfake), ('d_dreal', d_dreal), ('d_dfake', d_dfake)):
        assert np.abs(ref[k] - a.numpy()).max() <= 1e-15 * np.abs(ref[k]).max(), k


def test_every_count_reaches_its_edge():
    for name, counts in (('gan_lsq_logits', R.LSQ_COUNTS), ('gan_patchgan_losses_lsq', R.FUSED_COUNTS)):
        cap, vec = R.CAPS[name]
        assert (cap, vec) == E.CAPS[R.PAIR[name]]            # "the existing grid caps": the launch arithmetic of the mirrored entry point
        assert counts[:4] == (1, 63, 257, 900) and all(c % 256 for c in counts)
        last = counts[-1]
        assert last == cap * 256 + 1 and R.trips(name, last) == 2 and R.trips(name, last - 1) == 1 and R.blocks_of(name, last) == cap
        x = R.logits(last, last)
        assert x[-1] == -100.0 and x[0] == -100.0 and x[1] == 100.0 and {0.0} == set(np.abs(x[6:8]))     # the planted +-100 and +-0
        assert np.signbit(x[6]) and not np.signbit(x[7])


def test_gates_pass_the_fp32_models():
    worst = {}
    for count in R.LSQ_COUNTS:
        x = R.logits(count, count)
        for target in (1.0, 0.0):
            ls_, gs_ = R.lsq_args(target)
            for ls0 in (1.0, R.LS_ON[0]):
                loss, grad = R.lsq_model(x, target, gs_, ls0, ls_)
                for dt in DTS:
                    for k, v in R.check_lsq(x, target, gs_, ls0, dt, loss, R.cast(grad, dt), ls_).items():
                        E.note(worst, 'gan_lsq_logits', f'{k} {NAME[dt]}', v)
                acc = F32(1.5) + F32(loss)
                E.note(worst, 'gan_lsq_logits', 'accumulate', R.check_accumulate(1.5, loss, acc))
    for count in R.FUSED_COUNTS:
        real, fake = _pair(count)
        for ls0 in (1.0, R.LS_ON[0]):
            mdl = R.fused_model(real, fake, ls0, R.LAM, R.L1V)
            for dt in DTS:
                got = dict(mdl, **{k: R.cast(mdl[k], dt) for k in ('g_dfake', 'd_dreal', 'd_dfake')})
                for k, v in R.check_fused(real, fake, ls0, dt, got, R.LAM, R.L1V).items():
                    E.note(worst, 'gan_patchgan_losses_lsq', f'{k} {NAME[dt]}', v)
    print(E.table(worst, 'least-squares loss: fp32 models on the CPU'))
    for name, items in worst.items():
        for k, v in items.items():
            assert v <= MODEL_MAX, (name, k, v)
    # f16 with the loss scale on: the single-element case (x = -100) overflows and the gate demands the signed inf there
    x = R.logits(1, 1)
    _, grad = R.lsq_model(x, 1.0, 1.0, R.LS_ON[0])
    st = R.cast(grad, L.F16)
    assert torch.isinf(st).all() and float(st[0]) < 0
    assert R.check_lsq(x, 1.0, 1.0, R.LS_ON[0], L.F16, 10201.0, st)['grad'] == 0.0
    assert R.check_lsq(x, 1.0, 1.0, R.LS_ON[0], L.F16, 10201.0, -st)['grad'] == math.inf                   # the wrong sign
    assert R.check_lsq(x, 1.0, 1.0, R.LS_ON[0], L.F16, 10201.0, torch.full_like(st, -65504.0))['grad'] == math.inf     # clamped
    # ... and a finite reference does not accept an inf
    x = R.logits(63, 63)
    _, grad = R.lsq_model(x, 1.0, 1.0, 1.0)
    st = R.cast(grad, L.F16)
    st[0] = -math.inf
    assert R.check_lsq(x, 1.0, 1.0, 1.0, L.F16, 0.0, st)['grad'] == math.inf


def test_lsq_gates_reject_wrong_kernels():
    out = {}
    for count in R.LSQ_COUNTS[1:]:
        x = R.logits(count, count)
        loss, grad = R.lsq_model(x, 1.0, 1.0)
        chk = lambda l=loss, g=grad, ls0=1.0, t=1.0: R.check_lsq(x, t, 1.0, ls0, L.F32, l, None if g is None else R.cast(g, L.F32))
        out[f'factor 2 missing {count}'] = chk(g=(grad * F32(0.5)).astype(F32))['grad']
        out[f'/(count-1) {count}'] = chk(g=(grad * (F32(count) / F32(count - 1))).astype(F32))['grad']
        l0, g0 = R.lsq_model(x, 0.0, 1.0)                    # target 0 where 1 is meant
        res = chk(l=l0, g=g0)
        out[f'target 0 for 1: loss {count}'], out[f'target 0 for 1: grad {count}'] = res['loss'], res['grad']
        # ls not applied to the gradients
        out[f'ls not applied {count}'] = chk(ls0=R.LS_ON[0])['grad']
        # loss_accumulate overwriting
        out[f'accumulate overwrites {count}'] = R.check_accumulate(1.5, loss, loss)
        if count > R.cap_elems('gan_lsq_logits'):            # the tail beyond the grid cap dropped (the last logit is -100)
            d = (x - F32(1)).astype(F32)
            kept = (d * d)[:R.cap_elems('gan_lsq_logits')]
            out[f'lost tail {count}'] = chk(l=F32(kept.astype(np.float64).sum() / count), g=None)['loss']
    for k, v in out.items():
        print(f"  LSQ {k}: {v:.3g}")
        assert v >= MUTANT_MIN, (k, v)


def test_fused_gates_reject_wrong_kernels():
    out, fma_differs = {}, []
    keys = ('g_dfake', 'd_dreal', 'd_dfake')
    for count in R.FUSED_COUNTS[1:]:
        real, fake = _pair(count)
        mdl = R.fused_model(real, fake, 1.0, R.LAM, R.L1V)

        def worst(got, ls0=1.0, l1=R.L1V, items=None):
            got = dict(got, **{k: R.cast(got[k], L.F32) for k in keys})
            res = R.check_fused(real, fake, ls0, L.F32, got, R.LAM, l1)
            return max(v for k, v in res.items() if items is None or k in items)
        half, two = F32(0.5), F32(2)
        out[f'factor 2 missing {count}'] = worst(dict(mdl, g_dfake=mdl['g_dfake'] * half), items=('g_dfake',))
        n1 = F32(count) / F32(count - 1)
        out[f'/(count-1) {count}'] = worst(dict(mdl, **{k: (mdl[k] * n1).astype(F32) for k in keys}), items=keys)
        sw = R.fused_model(fake, real, 1.0, R.LAM, R.L1V)              # real and fake exchanged = every target wrong
        t0 = R.fused_model(real, (fake + F32(1)).astype(F32), 1.0, R.LAM, R.L1V)      # gan against target 0: (f + 1) - 1 = f
        out[f'target 0 for 1: gan {count}'] = worst(dict(mdl, gan=t0['gan'], gen_total=t0['gan'] + F32(R.LAM) * F32(R.L1V)), items=('gan',))
        out[f'real / fake exchanged {count}'] = worst(sw)
        out[f'0.5 of disc missing: loss {count}'] = worst(dict(mdl, disc=mdl['disc'] * two), items=('disc',))
        out[f'0.5 of disc missing: grads {count}'] = worst(dict(mdl, d_dreal=mdl['d_dreal'] * two, d_dfake=mdl['d_dfake'] * two), items=keys)
        out[f'0.5 of disc twice: loss {count}'] = worst(dict(mdl, disc=mdl['disc'] * half), items=('disc',))
        out[f'0.5 of disc twice: grads {count}'] = worst(dict(mdl, d_dreal=mdl['d_dreal'] * half, d_dfake=mdl['d_dfake'] * half), items=keys)
        out[f'g_dfake / d_dfake swapped {count}'] = worst(dict(mdl, g_dfake=mdl['d_dfake'], d_dfake=mdl['g_dfake']), items=keys)
        out[f'ls not applied {count}'] = worst(mdl, ls0=R.LS_ON[0], items=keys)
        if count > R.cap_elems('gan_patchgan_losses_lsq'):
            d = (fake - F32(1)).astype(F32)
            lossy = F32((d * d)[:R.cap_elems('gan_patchgan_losses_lsq')].astype(np.float64).sum() / count)
            out[f'lost tail {count}'] = worst(dict(mdl, gan=lossy, gen_total=lossy + F32(R.LAM) * F32(R.L1V)), items=('gan',))
        # gen_total formed with an fma: one rounding of the exact gan + lambda * l1 (exact in double: 24 + 24 bit product)
        for l1 in (R.L1V, 0.123, 0.77, 0.0419):
            g = mdl['gan']
            fma = F32(float(g) + float(F32(R.LAM)) * float(F32(l1)))
            fma_differs.append(worst(dict(mdl, gen_total=fma), l1=l1, items=('gen_total',)))
    out['gen_total with an fma (worst case)'] = max(fma_differs)
    print(f"  fma differs from the two-rounding sum in {sum(v > 0 for v in fma_differs)} of {len(fma_differs)} cases")
    for k, v in out.items():
        print(f"  FUSED {k}: {v:.3g}")
        assert v >= MUTANT_MIN, (k, v)


# ---- header, binding, command lines --------------------------------------------------------------------------------------------------------
def _declared_args(header, name):
    m = re.search(r'\bint ' + name + r'\(([^;]*?)\);', header, re.S)
    assert m, f"{name} is not declared in include/gan_amd.h"
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_header_declares_and_lib_binds_both_entry_points():
    header = open(os.path.join(R.ROOT, 'include', 'gan_amd.h')).read()
    for new, old in R.PAIR.items():
        args = _declared_args(header, new)
        assert args == _declared_args(header, old), (new, args)          # the documented argument lists: one for one
        assert new in L.SYMBOLS and L.SYMBOLS[new] == L.SYMBOLS[old]
    assert _declared_args(header, 'gan_lsq_logits')[:3] == ['const float* x', 'int64_t count', 'float target']
    assert len(_declared_args(header, 'gan_patchgan_losses_lsq')) == 16
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        assert lib.gan_lsq_logits.argtypes == lib.gan_bce_logits.argtypes
        assert lib.gan_patchgan_losses_lsq.argtypes == lib.gan_patchgan_losses.argtypes
        # argument errors come back before anything is launched (no GPU needed)
        assert lib.gan_lsq_logits(None, 1, 1.0, 1.0, 0, None, 1.0, L.F32, None, 8, None, None, None) != 0
        assert lib.gan_patchgan_losses_lsq(None, None, 1, L.F32, None, None, None, 8, 100.0, None, None, None, None, None, None, None) != 0


def test_both_clis_parse_gan_loss():
    from gan_amd import cycle_gan, pix2pix
    p = ['--data', 'd', '--output', 'o', '--train', '--epochs', '1']
    c = ['--input-images', 'x', '--target-images', 'y', '--output', 'o', '--train', '--epochs', '1']
    for mod, base in ((pix2pix, p), (cycle_gan, c)):
        assert mod.parse_opt(base).gan_loss == 'bce'
        assert mod.parse_opt(base + ['--gan-loss', 'bce']).gan_loss == 'bce'
        opt = mod.parse_opt(base + ['--gan-loss', 'lsgan'])
        assert opt.gan_loss == 'lsgan' and vars(opt)['gan_loss'] == 'lsgan'            # vars(opt) is the config written to config.json
        for bad in ('mse', 'LSGAN', ''):
            with pytest.raises(SystemExit):
                mod.parse_opt(base + ['--gan-loss', bad])
    # composes with the secondary loss, the dtype and the averaging flags
    opt = pix2pix.parse_opt(p + ['--gan-loss', 'lsgan', '--generator-loss', 'dssim', '--dtype', 'f16', '--ema-decay', '0.9'])
    assert (opt.gan_loss, opt.generator_loss, opt.dtype, opt.ema_decay) == ('lsgan', 'dssim', 'f16', 0.9)


def test_step_classes_take_the_keyword():
    import inspect
    from gan_amd.steps import CycleGANStep, Pix2PixStep
    for cls in (Pix2PixStep, CycleGANStep):
        assert inspect.signature(cls.__init__).parameters['gan_loss'].default == 'bce'
