"""CPU side of the elementwise-kernel checks (tests/elementwise_ref.py, tests/test_gpu_elementwise.py).  Without a GPU it shows:
  - the references agree with independent code (the oracle, torch autograd in fp64, published constants);
  - every gate passes a faithful fp32 model of its kernel, on the exact inputs of every GPU case, with a margin of two;
  - every gate rejects the named wrong variants of its kernel, on the same inputs, by a factor of two;
  - every GPU shape reaches the edge its comment claims, from the launch arithmetic alone."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from gan_amd import _lib as L
from oracle import gan_oracle as O
from tests import elementwise_ref as E

F32 = np.float32
DTS = (L.F32, L.BF16, L.F16)
NAME = {L.F32: 'f32', L.BF16: 'bf16', L.F16: 'f16'}
MODEL_MAX = 0.5           # a faithful fp32 model stays within half of every gate
MUTANT_MIN = 2.0          # a wrong variant lands at least twice outside


def _bits(x):
    return np.asarray(x, dtype=F32).view(np.uint32)


def _from_bits(*b):
    return np.array(b, dtype=np.uint32).view(F32)


# ---- references against independent code ------------------------------------------------------------------------------------------------
def test_references_agree_with_the_oracle_and_autograd():
    x = E.logits(1800, 1)
    for t in (1.0, 0.0):
        loss, grad = E.bce_ref(x, t, 1.0)
        ol, og = O.bce_logits(x.astype(np.float64), t)
        assert abs(loss - ol) < 1e-14 * max(1, abs(ol)) and np.abs(grad - og).max() < 1e-18
        xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        l = F.binary_cross_entropy_with_logits(xt, torch.full_like(xt, t))
        l.backward()
        assert abs(loss - l.item()) < 1e-14 * max(1, abs(loss)) and np.abs(grad - xt.grad.numpy()).max() < 1e-18
    a, b = E.lattice((2, 16, 16, 3), 2)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    loss, grad = E.l1_ref(a64.reshape(-1), b64.reshape(-1), 1.0)
    ol, og = O.l1_mean(a64, b64)
    assert abs(loss - ol) < 1e-15 and np.array_equal(grad, og.reshape(-1))
    at = torch.from_numpy(a64).requires_grad_(True)
    (at - torch.from_numpy(b64)).abs().mean().backward()
    assert np.array_equal(grad, at.grad.numpy().reshape(-1)) and (grad == 0).sum() >= 16 * 3      # sign(0) = 0 on the planted row
    # Adam: three steps of the oracle's TF-form Adam in fp64 against moments_ref + update_ref chained
    p, m, v, g = E.adam_inputs(1028, 3)
    omb1, omb2, eps = E.adam_consts()
    opt = O.AdamTF(float(F32(E.LR)), 1.0 - float(omb1), 1.0 - float(omb2))
    P = {'w': p.astype(np.float64)}
    opt.apply(P, {'w': np.zeros(p.size)})           # creates the slots (zero gradient, zero moments: nothing moves)
    assert np.array_equal(P['w'], p.astype(np.float64))
    opt.m['w'][:], opt.v['w'][:] = m, v
    opt.apply(P, {'w': g.astype(np.float64)})
    lr_t = float(F32(E.LR)) * math.sqrt(1 - (1.0 - float(omb2)) ** 2) / (1 - (1.0 - float(omb1)) ** 2)
    mr, vr = E.adam_moments_ref(m, v, g, 1.0)
    # the oracle's eps is the double 1e-7, the kernel's the float: compare through the update with the oracle's own eps
    u = mr * lr_t / (np.sqrt(vr) + O.ADAM_EPS)
    assert np.allclose(opt.m['w'], mr, rtol=1e-14, atol=0) and np.allclose(opt.v['w'], vr, rtol=1e-14, atol=0)
    assert np.abs(P['w'] - (p.astype(np.float64) - u)).max() < 1e-15
    u2, p2 = E.adam_update_ref(p, mr, vr, lr_t)
    assert np.abs(u2 - u).max() <= 1e-7 * np.abs(u).max()           # eps float vs double: 1e-7 * 1.2e-8 relative to sqrt(v) ~ 1e-4
    assert np.array_equal(p2, p.astype(np.float64) - u2)
    # lr_t: extended precision against plain double, and the closed form at t = 1
    for t in (1, 2, 1000, 100000):
        assert E.ulps_apart32(E.lr_t_ref(E.LR, E.BETA1, E.BETA2, t), E.lr_t_model(E.LR, E.BETA1, E.BETA2, t)) <= 1
    b2 = float(F32(E.BETA2))
    assert abs(float(E.lr_t_ref(E.LR, E.BETA1, E.BETA2, 1)) - float(F32(E.LR)) * math.sqrt(1 - b2) / 0.5) < 1e-12


def test_splitmix64_and_mask_reference():
    assert E.mix64(0) == 0xE220A8397B1DCDAF                 # first output of SplitMix64 seeded with 0
    assert int(E._mix64_np(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF
    seed, step, sid = 2 ** 63 + 5, 5, 10
    key = E.mix64(seed ^ (step << 32) ^ sid)
    m = E.mask_ref(77, seed, step, sid).numpy()
    for i in (0, 9):                                         # the vector form against scalar Python integers
        h = E.mix64(key ^ i)
        assert [int(b) for b in m[8 * i:8 * i + 8][:77 - 8 * i]] == [(h >> (8 * e + 7)) & 1 for e in range(8)][:77 - 8 * i]
    assert m.size == 77 and set(np.unique(m)) <= {0, 1}
    k3 = E.mix64((key + 3) & E.M64)
    assert E.mask_key(seed, step, sid, 3) == k3 and E.mask_key(seed, step, sid, 0) == key
    big = E.mask_ref(16387, 0, 0, 0).numpy()
    assert abs(big.mean() - 0.5) < 0.02


def test_cast_references_round_to_nearest_even():
    bf = lambda *b: E.cast_ref(_from_bits(*b), L.BF16).view(torch.int16).numpy().view(np.uint16).tolist()
    assert bf(0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff, 0x7f7fffff, 0x00000001, 0x80000000) == \
        [0x3f80, 0x3f82, 0x3f81, 0x3f80, 0x7f80, 0x0000, 0x8000]
    h = lambda *v: E.cast_ref(np.array(v, dtype=F32), L.F16).float().numpy().tolist()
    above = float(np.nextafter(F32(2.0 ** -25), F32(1)))
    assert h(65520.0, 65519.0, 2.0 ** -25, above) == [math.inf, 65504.0, 0.0, 2.0 ** -24]
    e = E.edge_values()
    assert np.isnan(e).sum() == 3 and np.isinf(e).sum() == 2 and (e == 0).sum() == 2
    # every pattern reaches every channel of every view and both halves of a packed pair
    x = E.edge_cycle(2 * 33 * 33 * 3)
    assert all(np.isnan(x.reshape(-1, 3)[:, c]).any() for c in range(3)) and np.isnan(x[0::2]).any() and np.isnan(x[1::2]).any()
    assert E.mismatches(E.cast_ref(x, L.BF16), E.cast_ref(x, L.BF16)) == 0
    assert E.wire_unpack_ref(E.cast_ref(_from_bits(0x3f818000), L.BF16), 1.0 / 3.0).numpy()[0] == F32(1.015625) * F32(1.0 / 3.0)


def test_weight_layout_reference():
    rng = np.random.default_rng(0)
    w = rng.standard_normal((16, 3, 5)).astype(F32)
    nat, tr = E.wprep_ref(w, L.F32)
    assert nat.shape == (16, 3, 8) and tr.shape == (16, 5, 8)
    for tap, a, b in ((0, 0, 0), (7, 2, 4), (15, 1, 3)):
        assert nat[tap, a, b] == w[tap, a, b] and tr[tap, b, a] == w[tap, a, b]
    assert (nat[..., 5:] == 0).all() and (tr[..., 3:] == 0).all()


# ---- every GPU shape reaches its edge ----------------------------------------------------------------------------------------------------
def test_every_shape_reaches_its_edge():
    def crosses(name, count):
        """More elements than the capped grid covers in one trip, and a ragged tail: no multiple of a block's elements."""
        blocks, vec = E.CAPS[name]
        assert count > blocks * 256 * vec, (name, count)
        assert count % (256 * vec) != 0 and E.trips(name, count) == 2 and E.blocks_of(name, count) == blocks, (name, count)
        assert count - blocks * 256 * vec < 256 * vec * blocks          # the second trip is partial: some threads stop after one
    crosses('gan_bce_logits', E.BCE_COUNTS[-1])
    crosses('gan_patchgan_losses', E.PATCHGAN_COUNTS[-1])
    n, h, w, c = E.L1_SHAPES[-1]
    assert n * h * w * c == 526683
    crosses('gan_l1', n * h * w * c)
    crosses('gan_adam_tf', E.ADAM_COUNTS[-1])
    crosses('gan_grads_check', E.CHECK_COUNTS[-1])
    crosses('gan_grad_pack', E.WIRE_COUNTS[-1])
    crosses('gan_grad_unpack', E.WIRE_COUNTS[-1])
    assert all(cnt % 4 == 0 for cnt in E.ADAM_COUNTS + E.CHECK_COUNTS) and all(cnt % 8 == 0 for cnt in E.WIRE_COUNTS)
    # the small cases stay below one trip and are ragged against the 256-thread block (or are a single element / vector)
    for cnt in E.BCE_COUNTS[:-1] + E.PATCHGAN_COUNTS[:-1]:
        assert cnt % 256 != 0 and cnt < 1024 * 256
    assert E.BCE_COUNTS[1] == 255 and E.BCE_COUNTS[2] == 257                # one below and one above a block
    assert E.ADAM_COUNTS[1] // 4 == 257                                     # one float4 more than a block
    # dropout: 2,053 bytes = 257 words (one more than a single-kernel block), 16,387 bytes = 2,049 words (multi-kernel block)
    words = lambda cnt: (cnt + 7) // 8
    assert words(2053) == E.MASK_WORDS_PER_BLOCK['gan_dropout_mask'] + 1 and 2053 % 8 != 0
    assert words(16387) == E.MASK_WORDS_PER_BLOCK['gan_dropout_mask_multi'] + 1 and 16387 % 8 != 0
    assert {cnt % 8 for cnt in E.MASK_COUNTS} >= {0, 1, 3, 5, 7} and min(E.MASK_COUNTS) == 1
    # pack: 6,534 elements are ragged against both block sizes and need more than one block of each
    n, h, w, c = E.PACK_SHAPES[-1]
    tot = n * h * w * c
    assert tot == 6534 and all(tot % per != 0 and tot > per for per in E.PACK_ELEMS_PER_BLOCK.values())
    assert all(off + 3 <= pitch for pitch, off in E.PACK_VIEWS)
    # weight prep: a side of 1, a side below 8, sides ragged against 8 and against the 64-wide tile, more than one tile per side
    assert any(A == 1 for A, B in E.WPREP_SHAPES) and any(B == 1 for A, B in E.WPREP_SHAPES)
    assert any(A % 8 and A > 64 for A, B in E.WPREP_SHAPES) and any(B % 8 and B > 128 for A, B in E.WPREP_SHAPES)
    assert any(A % 8 == 4 and B % 8 == 0 for A, B in E.WPREP_SHAPES)


# ---- the gates pass a faithful kernel -------------------------------------------------------------------------------------------------------
def _cast(x, dt):
    return E.cast_ref(x, dt)


def test_gates_pass_the_fp32_models():
    worst = {}
    for count in E.BCE_COUNTS:
        x = E.logits(count, count)
        for target in (1.0, 0.0):
            ls_, gs_ = E.bce_args(target)
            for ls0 in (1.0, E.LS_ON[0]):
                loss, grad = E.bce_model(x, target, gs_, ls0, ls_)
                for dt in DTS:
                    for k, v in E.check_bce(x, target, gs_, ls0, dt, loss, _cast(grad, dt), ls_).items():
                        E.note(worst, 'gan_bce_logits', f'{k} {NAME[dt]}', v)
    for count in E.PATCHGAN_COUNTS:
        real, fake = E.logits(count, count), E.logits(count, count + 1, -0.5)
        for ls0 in (1.0, E.LS_ON[0]):
            mdl = E.patchgan_model(real, fake, ls0, 100.0, 0.37)
            for dt in DTS:
                got = dict(mdl, **{k: _cast(mdl[k], dt) for k in ('g_dfake', 'd_dreal', 'd_dfake')})
                for k, v in E.check_patchgan(real, fake, ls0, dt, got, 100.0, 0.37).items():
                    E.note(worst, 'gan_patchgan_losses', f'{k} {NAME[dt]}', v)
    for shape in E.L1_SHAPES:
        a, b = E.lattice(shape, shape[2])
        for dt in DTS:
            a_st, b_st = E.stored(a, dt), E.stored(b, dt)
            for ls0 in (1.0, E.LS_ON[0]):
                loss, grad = E.l1_model(a_st.float().numpy(), b_st.float().numpy(), E.L1_GRAD_SCALE, ls0, E.L1_LOSS_SCALE)
                for k, v in E.check_l1(a_st, b_st, E.L1_GRAD_SCALE, ls0, dt, loss, _cast(grad, dt), E.L1_LOSS_SCALE).items():
                    E.note(worst, 'gan_l1', f'{k} {NAME[dt]}', v)
    lr_t = E.lr_t_model(E.LR, E.BETA1, E.BETA2, 1)
    for count in E.ADAM_COUNTS:
        p, m, v, g = E.adam_inputs(count, count)
        for wire in (0, 1):
            gw = E.cast_ref(g, L.BF16).float().numpy() if wire else g
            for gs in (1.0, 0.5, 1.0 / 1024.0, 0.5 / 1024.0):
                p1, m1, v1 = E.adam_model(p, m, v, gw, lr_t, gs)
                for k, val in E.check_adam(p, m, v, gw, gs, lr_t, p1, m1, v1).items():
                    E.note(worst, 'gan_adam_tf', k, val)
                z = np.arange(3, count, 64)                       # g = m = v = 0: p finite and unchanged
                assert np.array_equal(p1[z].view(np.uint32), p[z].view(np.uint32))
    for s in E.ADAM_BEGIN_STEPS:
        d = E.ulps_apart32(E.lr_t_ref(E.LR, E.BETA1, E.BETA2, s + 1), E.lr_t_model(E.LR, E.BETA1, E.BETA2, s + 1))
        E.note(worst, 'gan_adam_begin', 'lr_t (ulps of fp32, gate 1)', d)
    print(E.table(worst, 'fp32 models on the CPU'))
    for name, items in worst.items():
        for k, v in items.items():
            print(f"    {name} {k}: {v:.3f}")
            assert v <= (1.0 if name == 'gan_adam_begin' else MODEL_MAX), (name, k, v)


# ---- the gates have teeth --------------------------------------------------------------------------------------------------------------------
def test_bce_gates_reject_wrong_kernels():
    out = {}
    for count in E.BCE_COUNTS[1:]:
        x = E.logits(count, count)
        loss, grad = E.bce_model(x, 1.0, 1.0)
        # gradient divided by count - 1 (fp32 storage: in bf16 / f16 a relative 1 / (count - 1) is below one ulp of storage from 65 / 513 elements on)
        bad = (grad * (F32(count) / F32(count - 1))).astype(F32)
        out[f'/(count-1) {count}'] = E.check_bce(x, 1.0, 1.0, 1.0, L.F32, loss, _cast(bad, L.F32))['grad']
        # the loss that drops the last partial block (target 1: the last logit is -100, its term 100)
        if count > 256:
            terms = ((np.maximum(x, F32(0)) - x) + np.log1p(np.exp(-np.abs(x)))).astype(F32)
            kept = terms[:count - count % 256]
            lossy = F32(kept.astype(np.float64).sum() / count)
            out[f'lost tail {count}'] = E.check_bce(x, 1.0, 1.0, 1.0, L.F32, lossy, None)['loss']
    # BCE from the unsplit sigmoid 1 / (1 + exp(-v)) at v = -100: exp overflows, the sigmoid is 0 and the loss -log(0).  (The GRADIENT
    # of that variant is within the gate in IEEE arithmetic - 1 / inf = 0 is 3.8e-44 from sigmoid(-100) - so the loss is what rejects it.)
    x = E.logits(1, 1)
    assert x[0] == -100.0
    with np.errstate(over='ignore', divide='ignore'):
        sig = F32(1) / (F32(1) + np.exp(-x))
        loss = F32(-np.log(sig).mean())
    res = E.check_bce(x, 1.0, 1.0, 1.0, L.F32, loss, _cast((sig - F32(1)).astype(F32), L.F32))
    out['unsplit sigmoid at -100: loss'] = res['loss']
    print("unsplit sigmoid at -100: gradient ratio", res['grad'])
    for k, v in out.items():
        print(f"  BCE {k}: {v:.3g}")
        assert v >= MUTANT_MIN, (k, v)


def test_l1_gates_reject_wrong_kernels():
    out = {}
    for shape in E.L1_SHAPES[1:]:
        a, b = E.lattice(shape, shape[2])
        for dt in DTS:
            a_st, b_st = E.stored(a, dt), E.stored(b, dt)
            a32, b32 = a_st.float().numpy(), b_st.float().numpy()
            loss, grad = E.l1_model(a32, b32, E.L1_GRAD_SCALE)
            d = (a32 - b32).reshape(-1)
            assert (d == 0).sum() >= shape[2] * shape[3]
            gs = F32(E.L1_GRAD_SCALE) / F32(d.size)
            plus = np.where(d >= 0, gs, -gs).astype(F32)                            # sign(0) = +1
            out[f'sign(0)=+1 {shape} {NAME[dt]}'] = E.check_l1(a_st, b_st, E.L1_GRAD_SCALE, 1.0, dt, loss, _cast(plus, dt))['grad']
            if shape[3] > 1:
                out[f'1/pixels {shape} {NAME[dt]}'] = E.check_l1(a_st, b_st, E.L1_GRAD_SCALE, 1.0, dt, loss, _cast(grad * F32(shape[3]), dt))['grad']
    for k, v in out.items():
        print(f"  L1 {k}: {v:.3g}")
        assert v >= MUTANT_MIN, (k, v)


def test_adam_gates_reject_wrong_kernels():
    omb1, omb2, eps = E.adam_consts()
    lr_t = E.lr_t_model(E.LR, E.BETA1, E.BETA2, 1)
    out = {}
    for count in E.ADAM_COUNTS[:2]:
        p, m, v, g = E.adam_inputs(count, count)
        if count == 4:
            g = g.copy()
            g[:] = F32(0.25), F32(-1e-3), F32(0.0), F32(3e-5)     # (the planted zeros would leave nothing to update)
            m, v = m.copy(), v.copy()
            m[3], v[3] = F32(1e-4), F32(1e-8)
        p1, m1, v1 = E.adam_model(p, m, v, g, lr_t, 1.0)
        chk = lambda pp, mm, vv: E.check_adam(p, m, v, g, 1.0, lr_t, pp, mm, vv)
        out[f'eps inside sqrt {count}'] = chk((p - (m1 * lr_t) / np.sqrt(v1 + eps)).astype(F32), m1, v1)['p']
        out[f'lr for lr_t {count}'] = chk((p - (m1 * F32(E.LR)) / (np.sqrt(v1) + eps)).astype(F32), m1, v1)['p']
        pl, ml, vl = p1.copy(), m1.copy(), v1.copy()
        pl[-4:], ml[-4:], vl[-4:] = p[-4:], m[-4:], v[-4:]                          # the last float4 skipped
        res = chk(pl, ml, vl)
        out[f'last float4 skipped {count}'] = max(res['m'], res['v'])
        # v updated from the slot the m update was written to: v_old read after m_new overwrote it
        vb = (m1 + (g * g - m1) * omb2).astype(F32)
        with np.errstate(invalid='ignore'):          # (that v can be negative: the reference update of it is NaN, only 'v' is read)
            out[f'v_old read after the m update {count}'] = chk((p - (m1 * lr_t) / (np.sqrt(np.abs(vb)) + eps)).astype(F32), m1, vb)['v']
    for k, val in out.items():
        print(f"  Adam {k}: {val:.3g}")
        assert val >= MUTANT_MIN, (k, val)


def test_exact_checks_reject_wrong_casts_masks_and_layouts():
    x = E.edge_cycle(2 * 33 * 33 * 3)
    bits = x.view(np.uint32)
    ref = E.cast_ref(x, L.BF16)
    trunc = torch.from_numpy((bits >> 16).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    half_up = torch.from_numpy(((bits.astype(np.uint64) + 0x8000) >> 16).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    assert E.exact(trunc, ref) == math.inf and E.exact(half_up, ref) == math.inf
    # ... and on the tie patterns alone: truncation misses the odd tie and the value above, half-up the even tie
    t = _from_bits(0x3f808000, 0x3f818000, 0x3f808001)
    tb = t.view(np.uint32)
    as_bf = lambda u: torch.from_numpy(u.astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    assert E.mismatches(as_bf(tb >> 16), E.cast_ref(t, L.BF16)) == 2
    assert E.mismatches(as_bf((tb + 0x8000) >> 16), E.cast_ref(t, L.BF16)) == 1
    # f16 by truncation: the nearest value pulled towards zero wherever rounding went away from zero
    fin = x[np.isfinite(x)]
    with np.errstate(over='ignore'):
        h = fin.astype(np.float16)
    away = np.abs(h.astype(np.float64)) > np.abs(fin.astype(np.float64))
    ht = np.where(away, np.nextafter(h, np.float16(0)), h).astype(np.float16)
    assert away.any() and E.exact(torch.from_numpy(ht), E.cast_ref(fin, L.F16)) == math.inf
    assert E.exact(torch.from_numpy(h), E.cast_ref(fin, L.F16)) == 0.0               # numpy's own cast is round-to-nearest-even too
    # masks
    for count in E.MASK_COUNTS:
        ref = E.mask_ref(count, 2 ** 63 + 5, 5, 10, draw=3)
        if count >= 7:            # (a mask of one byte differs from a wrong one only half the time)
            assert E.exact(E.mask_ref(count, 2 ** 63 + 5, 5, 10, draw=3, bit=0), ref) == math.inf, count
            assert E.exact(E.mask_ref(count, 2 ** 63 + 5, 5, 10, draw=3, use_draw=False), ref) == math.inf, count
    # tr padding left unwritten (the NaN the buffer was filled with stays)
    for A, B in E.WPREP_SHAPES:
        w = np.resize(E.edge_cycle(16 * A * B, 1), (16, A, B))
        for dt in DTS:
            nat, tr = E.wprep_ref(w, dt)
            if A % 8:
                bad = tr.clone()
                bad[..., A:] = float('nan')
                assert E.exact(bad, tr) == math.inf
            if B % 8:
                bad = nat.clone()
                bad[..., B:] = float('nan')
                assert E.exact(bad, nat) == math.inf
    # -0 against +0 in the padding, and a NaN of another payload, are told apart / accepted as documented
    z = torch.zeros(4)
    assert E.exact(-z, z) == math.inf and E.exact(torch.from_numpy(_from_bits(0x7fc00000)), torch.from_numpy(_from_bits(0x7f800001))) == 0.0
