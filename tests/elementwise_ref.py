"""References, gates, fp32 models and shared inputs of the loss / Adam / cast / mask kernels of gan_amd/csrc/elementwise.hip
(helper of tests/test_cpu_elementwise.py and tests/test_gpu_elementwise.py; numpy and torch-CPU only, not a conftest).

Three kinds of expected values:
  - fp64 references, computed from the exact stored inputs the kernel reads (fp32 arrays, 16-bit values widened exactly);
  - bit-exact references where one answer is right: the casts (torch's CPU round-to-nearest-even), the wire format, the dropout
    mask (SplitMix64 in integers), the weight layouts, sum3;
  - numpy float32 models of the gated kernels in the kernels' own operation order (for the losses including the reduction order).
    tests/test_cpu_elementwise.py proves with them, without a GPU, that every gate passes a faithful kernel with a margin of two
    and rejects the named wrong variants by a factor of two.

Every gate counts roundings; EPS32 = 2^-23 is one ulp of 1.0 in fp32, so ONE correctly rounded fp32 operation errs by at most
0.5 * EPS32 * |result|.  The count is written beside each gate."""
import math

import numpy as np
import torch

from gan_amd import _lib as L
from tests.launch_audit import EPS32, K_ULP, TDT, ratio, ulp      # noqa: F401  (ratio, TDT: re-exported to the two test files)

F32 = np.float32
DTYPES = {'f32': L.F32, 'bf16': L.BF16, 'f16': L.F16}

# ---- launch arithmetic -----------------------------------------------------------------------------------------------------------
# name -> (block cap, elements per thread and trip); every kernel runs 256 threads per block and strides by the whole grid
THREADS = 256
CAPS = {
    'gan_bce_logits': (1024, 1),          # elementwise.hip:603   if (blocks > 1024) blocks = 1024;
    'gan_patchgan_losses': (256, 1),      # elementwise.hip:624   if (blocks > 256) blocks = 256;
    'gan_l1': (2048, 1),                  # elementwise.hip:647   if (blocks > 2048) blocks = 2048;
    'gan_adam_tf': (4096, 4),             # elementwise.hip:677   if (blocks > 4096) blocks = 4096;   (float4 per thread)
    'gan_grads_check': (4096, 4),         # elementwise.hip:692   if (blocks > 4096) blocks = 4096;   (uint4 per thread)
    'gan_grad_pack': (4096, 8),           # elementwise.hip:885   ... < 4096 ? ... : 4096             (8 elements per thread)
    'gan_grad_unpack': (4096, 8),         # elementwise.hip:893
}
# one launch covers: words (8 mask bytes) per block of the two dropout kernels, elements per block of the two pack kernels
MASK_WORDS_PER_BLOCK = {'gan_dropout_mask': 256, 'gan_dropout_mask_multi': 2048}      # elementwise.hip:407, :464
PACK_ELEMS_PER_BLOCK = {'gan_pack': 256, 'gan_pack_multi': 2048}                      # elementwise.hip:417, :434


def cap_elems(name):
    """Elements the capped grid covers in ONE trip."""
    blocks, vec = CAPS[name]
    return blocks * THREADS * vec


def blocks_of(name, count):
    blocks, vec = CAPS[name]
    return min((count // vec + THREADS - 1) // THREADS, blocks)


def trips(name, count):
    """T: serial trips of the busiest thread = additions per thread of a loss kernel."""
    _, vec = CAPS[name]
    per = blocks_of(name, count) * THREADS * vec
    return (count + per - 1) // per


# ---- the GPU cases (shared, so that the CPU file proves its claims on exactly the inputs the GPU file feeds) ------------------------
BCE_COUNTS = (1, 255, 257, 1800, 262144 + 257)          # the last: the 1,024-block cap plus a ragged second trip
PATCHGAN_COUNTS = (2700, 65536 + 300)                   # the last: the 256-block cap plus a ragged second trip
L1_SHAPES = ((1, 1, 1, 1), (2, 16, 16, 3), (1, 9, 29, 1), (1, 419, 419, 3))      # the last: 526,683 elements, the cap covers 524,288
ADAM_COUNTS = (4, 1028, 4194304 + 1200)                 # the last: the 4,096-block cap plus a ragged second trip
CHECK_COUNTS = (4, 4194304 + 1200)
WIRE_COUNTS = (8, 8388608 + 2400)                       # the cap covers 8,388,608
MASK_COUNTS = (1, 7, 8, 9, 77, 2053, 16387)             # 2,053 bytes = 257 words, 16,387 bytes = 2,049 words: one past a block
MASK_KEYS = ((0, 0), (0, 5), (2 ** 63 + 5, 0), (2 ** 63 + 5, 5))     # (seed, step)
MASK_SIDS = (0, 10)
PACK_SHAPES = ((1, 1, 1, 1), (2, 8, 8, 3), (2, 33, 33, 3))           # the last: 6,534 elements, ragged against 256 and 2,048
PACK_VIEWS = ((8, 0), (8, 2), (8, 5), (16, 0), (16, 2), (16, 5))     # (pitch, channel offset)
WPREP_SHAPES = ((1, 64), (64, 1), (3, 64), (100, 72), (65, 129))     # (A, B)
ADAM_BEGIN_STEPS = (0, 1, 999, 99999)
LS_ON = (1024.0, 1.0 / 1024.0, 0.0, 0.0)                # loss-scale state: gradients x 1024, Adam x 1/1024
LS_SKIP = (1024.0, 1.0 / 1024.0, 0.0, 1.0)              # [3] != 0: this step is skipped
LR, BETA1, BETA2, ADAM_EPS = 2e-4, 0.5, 0.999, 1e-7
# gan_l1 arguments: 25 / total x 1024 stays finite in f16 down to ONE element; the power-of-two loss_scale multiplies exactly
L1_GRAD_SCALE, L1_LOSS_SCALE = 25.0, 2.0

# planted logits: the first min(count, 8) elements and (from 16 elements on) the last 8 in reverse, so that the very last logit of
# every larger case - the one a lost tail loses - is -100
PLANTED = np.array([-100.0, 100.0, -20.0, 20.0, -1e-6, 1e-6, -0.0, 0.0], dtype=F32)


def logits(count, seed, shift=0.0):
    x = (3.0 * np.random.default_rng(seed).standard_normal(count) + shift).astype(F32)
    k = min(count, PLANTED.size)
    x[:k] = PLANTED[:k]
    if count >= 2 * PLANTED.size:
        x[-PLANTED.size:] = PLANTED[::-1]
    return x


def lattice(shape, seed):
    """Two images on the normalize() lattice k / 127.5 - 1 (about 1 pair in 256 exactly equal), row 0 of image 0 all equal when
    there is more than one row; a single-element tensor is made unequal."""
    rng = np.random.default_rng(seed)
    a = (rng.integers(0, 256, shape).astype(F32) / F32(127.5) - F32(1.0)).astype(F32)
    b = (rng.integers(0, 256, shape).astype(F32) / F32(127.5) - F32(1.0)).astype(F32)
    if shape[1] > 1:
        b[0, 0] = a[0, 0]
    elif a.size == 1:
        a.flat[0], b.flat[0] = F32(0.5), F32(-0.25)
    return a, b


def adam_inputs(count, seed):
    """(p, m, v, g) fp32.  Moments as tests/test_gpu_launch_audit.py::_reset sets them; gradient magnitudes 1e-6..1; p = 0 on a
    quarter of the elements (the update term of the p gate is then the whole gate); exact zeros planted: g = 0 on every 16th
    element, g = m = v = 0 on elements 3, 67, ... (p != 0) and 8, 72, ... (p = 0)."""
    rng = np.random.default_rng(seed)
    p = (0.05 * rng.standard_normal(count)).astype(F32)
    p[p == 0] = F32(0.01)
    p[0::4] = 0
    m = (1e-4 * rng.standard_normal(count)).astype(F32)
    v = (1e-8 * rng.random(count) + 1e-10).astype(F32)
    g = (rng.standard_normal(count) * 10.0 ** rng.integers(-6, 1, count)).astype(F32)
    g[2::16] = 0
    for z in (3, 8):
        g[z::64] = 0
        m[z::64] = 0
        v[z::64] = 0
    return p, m, v, g


def edge_values():
    """fp32 bit patterns at which a cast goes wrong: halfway cases of bf16 and f16 (both parities, and one fp32 ulp off the tie),
    f16 overflow and subnormals, fp32 max (bf16: rounds to inf), fp32 subnormals, +-0, inf, NaN (quiet, signalling, negative)."""
    bits = [0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff, 0xbf808000, 0xbf818000,       # bf16 ties: to even, above, below
            0x3f801000, 0x3f803000, 0x3f801001, 0x3f800fff, 0xbf801000, 0xbf803000,       # f16 ties
            0x7f7fffff, 0xff7fffff, 0x00000001, 0x007fffff, 0x80000001,                   # fp32 max, fp32 subnormals
            0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffc00000]
    vals = [65520.0, 65519.0, 65504.0, -65520.0, 1e5, 2.0 ** -25, float(np.nextafter(F32(2.0 ** -25), F32(1))), 2.0 ** -24,
            3 * 2.0 ** -25, 5 * 2.0 ** -25, -2.0 ** -25, 2.0 ** -14, 2.0 ** -15, 2.0 ** -14 - 2.0 ** -25, 6e-8, 1.0, -1.0, -0.3, 3.4e38]
    out = np.concatenate([np.array(bits, dtype=np.uint32).view(F32), np.array(vals, dtype=F32)])
    assert out.size == 43          # a prime: coprime to the pitches, the channel counts and the lane counts
    return out


def edge_cycle(n, seed=0):
    """n fp32 values: the 43 edge patterns cycled through the tensor, every fifth element an ordinary random value (43 and 5 are
    coprime to the pitches, channel and lane counts: every channel and lane position meets every pattern)."""
    x = np.resize(edge_values(), n).copy()
    r = np.random.default_rng(seed).standard_normal(n).astype(F32)
    x[4::5] = r[4::5]
    return x


def t64(a):
    if isinstance(a, torch.Tensor):          # (the data-parallel audit's end check gates whole networks where they live)
        return a.double()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def stored(x32, dt):
    """fp32 numpy -> CPU tensor of the storage type (what the device buffer holds; .double() widens it exactly)."""
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=F32)).to(TDT[dt])


# ---- bit-exact references -------------------------------------------------------------------------------------------------------------
def cast_ref(x32, dt):
    """fp32 -> storage type, round to nearest even (torch CPU)."""
    return stored(x32, dt)


def mismatches(got, ref):
    """Elements that differ: NaNs are compared with isnan, every other bit pattern as an integer."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    if not got.is_floating_point():
        return int((got != ref).sum())
    it = torch.int16 if got.element_size() == 2 else torch.int32
    ng, nr = torch.isnan(got), torch.isnan(ref)
    return int(((ng != nr) | (~nr & (got.contiguous().view(it) != ref.contiguous().view(it)))).sum())


def exact(got, ref):
    """Gate entry of a bit-exact check: 0 or inf."""
    return 0.0 if mismatches(got, ref) == 0 else math.inf


def wire_unpack_ref(bf, scale):
    """bf16 -> fp32 times scale: ONE numpy float32 multiply."""
    return torch.from_numpy(bf.float().numpy() * F32(scale))


M64 = (1 << 64) - 1


def mix64(z):
    """SplitMix64 finaliser (elementwise.hip:399-404) on a Python int."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _mix64_np(z):
    with np.errstate(over='ignore'):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mask_key(seed, step, sid, draw=0):
    key = mix64((seed ^ ((step & 0xffffffff) << 32) ^ sid) & M64)
    if draw:
        key = mix64((key + draw) & M64)
    return key


def mask_ref(count, seed, step, sid, draw=0, bit=7, use_draw=True):
    """Dropout mask bytes: byte 8i+e = bit 8e+7 of mix64(key ^ i).  (bit / use_draw: the wrong variants of the CPU tests.)"""
    key = mask_key(seed, step, sid, draw if use_draw else 0)
    i = np.arange((count + 7) // 8, dtype=np.uint64)
    h = _mix64_np(np.uint64(key) ^ i)
    e = np.arange(8, dtype=np.uint64)
    b = ((h[:, None] >> (e[None, :] * np.uint64(8) + np.uint64(bit))) & np.uint64(1)).astype(np.uint8)
    return torch.from_numpy(b.reshape(-1)[:count].copy())


def pad8(c):
    return (c + 7) // 8 * 8


def wprep_ref(master, dt):
    """master fp32 [16][A][B] -> nat [16][A][B8], tr [16][B][A8] of the storage type, the padding written as +0."""
    _, A, B = master.shape
    t = cast_ref(master, dt)
    nat = torch.zeros((16, A, pad8(B)), dtype=TDT[dt])
    tr = torch.zeros((16, B, pad8(A)), dtype=TDT[dt])
    nat[..., :B] = t
    tr[..., :A] = t.transpose(1, 2)
    return nat, tr


def sum3_ref(a, b, c):
    return (a.astype(F32) + b.astype(F32)) + c.astype(F32)


def flag_ref(g32):
    """gan_grads_check: 1 when any element has an all-ones exponent."""
    return float(((g32.view(np.uint32) & np.uint32(0x7f800000)) == np.uint32(0x7f800000)).any())


# ---- fp64 references -----------------------------------------------------------------------------------------------------------------
def _sigmoid_minus_t(x, t):
    """sigmoid(x) - t in fp64 WITHOUT the cancellation at confident logits: sigmoid(x) - 1 = -sigmoid(-x)."""
    e = np.exp(-np.abs(x))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)              # sigmoid(|x|), sigmoid(-|x|)
    if t == 1.0:
        return -np.where(x >= 0, small, big)
    sig = np.where(x >= 0, big, small)
    return sig if t == 0.0 else sig - t


def bce_terms(x, t):
    return np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))


def bce_ref(x32, target, grad_scale):
    """-> (mean loss, (sigmoid(x) - t) * grad_scale / count), fp64.  grad_scale includes the dynamic loss scale."""
    x = x32.astype(np.float64)
    return float(bce_terms(x, target).mean()), _sigmoid_minus_t(x, target) * (grad_scale / x.size)


def patchgan_ref(real32, fake32, ls0=1.0):
    """-> dict: gan = BCE(1, fake), disc = 0.5 * (BCE(1, real) + BCE(0, fake)), the three means and the three logit gradients."""
    gan, g_dfake = bce_ref(fake32, 1.0, ls0)
    lr_, d_dreal = bce_ref(real32, 1.0, 0.5 * ls0)
    lf, d_dfake = bce_ref(fake32, 0.0, 0.5 * ls0)
    return dict(gan=gan, real=lr_, fake0=lf, disc=0.5 * (lr_ + lf), g_dfake=g_dfake, d_dreal=d_dreal, d_dfake=d_dfake)


def l1_ref(a, b, grad_scale):
    """a, b: stored values widened to fp64.  -> (mean |a-b|, sign(a-b) * grad_scale / total) with sign(0) = 0."""
    d = a - b
    return float(np.abs(d).mean()), np.sign(d) * (grad_scale / d.size)


def f32c(x):
    """An fp32 kernel argument, widened: the value the kernel really receives."""
    return float(F32(x))


def adam_consts(b1=BETA1, b2=BETA2, eps=ADAM_EPS):
    """(1 - beta1, 1 - beta2, eps) as the host computes them in fp32 (elementwise.hip:680)."""
    return F32(1) - F32(b1), F32(1) - F32(b2), F32(eps)


def adam_moments_ref(m0, v0, g, gs):
    """fp64 m, v from the stored fp32 / widened bf16 inputs; gs = grad_scale * (1 / loss scale)."""
    omb1, omb2, _ = (float(c) for c in adam_consts())
    m0, v0, gr = m0.astype(np.float64), v0.astype(np.float64), g.astype(np.float64) * gs
    return m0 + (gr - m0) * omb1, v0 + (gr * gr - v0) * omb2


def adam_update_ref(p0, m1, v1, lr_t):
    """fp64 (u, p) = (lr_t * m / (sqrt(v) + eps), p0 - u) of the moments given (see adam_gates for which)."""
    eps = float(adam_consts()[2])
    u = m1.astype(np.float64) * float(lr_t) / (np.sqrt(v1.astype(np.float64)) + eps)
    return u, p0.astype(np.float64) - u


def lr_t_ref(lr, b1, b2, t):
    """lr * sqrt(1 - b2^t) / (1 - b1^t) in extended precision from the fp32 arguments, rounded once to fp32."""
    ld = np.longdouble
    lr, b1, b2 = ld(F32(lr)), ld(F32(b1)), ld(F32(b2))
    return F32(lr * np.sqrt(ld(1) - b2 ** ld(t)) / (ld(1) - b1 ** ld(t)))


def ulps_apart32(a, b):
    """Distance of two finite positive fp32 values in ulps."""
    return abs(int(np.asarray(a, F32).view(np.int32)) - int(np.asarray(b, F32).view(np.int32)))


# ---- gates -------------------------------------------------------------------------------------------------------------------------------
def bce_grad_gate(ref, dt, grad_scale, count):
    """Stored gradient of BCE / PatchGAN: K_ULP * ulp_dt(ref) + 6 * EPS32 * |grad_scale| / count.
    K_ULP = 1 ulp of the storage type: the rounding to storage (half) and a reference on the other side of a binade edge (half).
    The absolute term, because sigmoid(x) - t cancels at confident logits: exp within 3 ulp of e <= 1 (OpenCL full profile) = 3,
    the add 1 + e, the correctly rounded divide, the two multiplies = 6 roundings of a value <= 1, scaled by grad_scale / count."""
    return K_ULP * ulp(t64(ref), dt) + 6 * EPS32 * abs(grad_scale) / count


def l1_grad_gate(ref, dt):
    """Stored gradient of L1: K_ULP * ulp_dt(ref) - the host's one correctly rounded divide grad_scale / total and the rounding to
    storage; the power-of-two loss scale multiplies exactly.  Where a == b the reference is 0 and the gate is the smallest
    subnormal: the stored value must be exactly 0."""
    return K_ULP * ulp(t64(ref), dt)


def loss_gate(name, count, bound_mean):
    """Loss scalars: EPS32 * (T + 16) * mean_i(bound_i).  T = additions per thread (trips of the capped grid); 16 = exp (3) +
    log1p (2) + the three adds of the term + the 6 shuffle levels + the 4-way block add (counted once) + the final conversion to
    float.  The second stage sums in double and adds nothing.  bound_i = |x_i| + 1 for BCE, |a_i - b_i| for L1."""
    return EPS32 * (trips(name, count) + 16) * bound_mean


def adam_gates(m0, v0, g, gs, p_ref, u_ref):
    """m: 2 * EPS32 * (|g*gs| + |m_old|)     - subtract, multiply, add: 3 half-ulps of at most that sum, x 4/3 for contraction
       v: 2 * EPS32 * ((g*gs)^2 + v_old)     - square, subtract, multiply, add: 4 half-ulps
       p: 1 * EPS32 * |p_ref| + 8 * EPS32 * |u_ref|   - the final subtract (half an ulp of p, x 2) and the update: multiply, sqrtf,
          add, divide = 4 half-ulps of u, x 4 for sqrtf and the divide not being correctly rounded on the device.
    m and v are gated against the fp64 values of the stored inputs.  u_ref and p_ref are computed in fp64 FROM THE NEW MOMENTS THE
    KERNEL STORED (as the launch audit does for the fused Adam): the p gate counts the roundings of the p statement alone, and an
    m that cancels (g*gs near -m_old) would otherwise carry its absolute error, legitimately within the m gate, into an update far
    smaller than that error."""
    m0, v0, gr = t64(m0), t64(v0), t64(g) * gs
    return (2 * EPS32 * (gr.abs() + m0.abs()), 2 * EPS32 * (gr * gr + v0), EPS32 * t64(p_ref).abs() + 8 * EPS32 * t64(u_ref).abs())


# ---- fp32 models: numpy float32 in the kernels' own operation order ---------------------------------------------------------------------------
def block_partials(terms, blocks):
    """Per-thread strided sums (serial, in trip order), the 64-lane xor butterfly, then red[0] + red[1] + red[2] + red[3]."""
    per = blocks * THREADS
    T = (terms.size + per - 1) // per
    pad = np.zeros(T * per, dtype=F32)
    pad[:terms.size] = terms
    s = np.zeros(per, dtype=F32)
    for k in range(T):
        s = s + pad[k * per:(k + 1) * per]
    v = s.reshape(blocks, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    red = v[..., 0]
    return ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]


def finalize_model(partials, count, loss_scale=1.0):
    """Second stage: the block sums added in double, times 1/count in double, ONE conversion to float, times loss_scale."""
    return F32(np.sum(partials.astype(np.float64)) * (1.0 / count)) * F32(loss_scale)


def _sig32(v, e):
    one = F32(1)
    return np.where(v >= 0, one / (one + e), e / (one + e)).astype(F32)


def bce_model(x, target, grad_scale, ls0=1.0, loss_scale=1.0):
    """bce_kernel + l1_finalize_kernel -> (loss fp32, fp32 gradient before the rounding to storage)."""
    t = F32(target)
    e = np.exp(-np.abs(x))
    terms = (np.maximum(x, F32(0)) - x * t) + np.log1p(e)
    gs = F32(grad_scale) * F32(ls0)
    inv = F32(1) / F32(x.size)
    grad = (gs * (_sig32(x, e) - t)) * inv
    return finalize_model(block_partials(terms, blocks_of('gan_bce_logits', x.size)), x.size, loss_scale), grad.astype(F32)


def patchgan_model(real, fake, ls0=1.0, lam=100.0, l1=0.0):
    """patchgan_bce_kernel + patchgan_finalize_kernel -> dict of fp32 scalars and fp32 gradients."""
    r, f = real, fake
    er, ef = np.exp(-np.abs(r)), np.exp(-np.abs(f))
    lr_, lf = np.log1p(er), np.log1p(ef)
    zero, one, half = F32(0), F32(1), F32(0.5)
    blocks = blocks_of('gan_patchgan_losses', r.size)
    s = [block_partials(t, blocks) for t in ((np.maximum(f, zero) - f) + lf, (np.maximum(r, zero) - r) + lr_, np.maximum(f, zero) + lf)]
    g, rr, ff = (finalize_model(p, r.size) for p in s)
    inv = F32(ls0) / F32(r.size)
    sr, sf = _sig32(r, er), _sig32(f, ef)
    return dict(gan=g, disc=half * rr + half * ff, gen_total=g + F32(lam) * F32(l1),
                g_dfake=((sf - one) * inv).astype(F32), d_dreal=((half * (sr - one)) * inv).astype(F32), d_dfake=((half * sf) * inv).astype(F32))


def l1_model(a, b, grad_scale, ls0=1.0, loss_scale=1.0):
    """l1_kernel + l1_finalize_kernel on the stored values widened to fp32 -> (loss fp32, fp32 gradient before storage)."""
    a, b = a.reshape(-1).astype(F32), b.reshape(-1).astype(F32)
    d = a - b
    gs = (F32(grad_scale) / F32(d.size)) * F32(ls0)
    grad = np.where(d > 0, gs, np.where(d < 0, -gs, F32(0))).astype(F32)
    return finalize_model(block_partials(np.abs(d), blocks_of('gan_l1', d.size)), d.size, loss_scale), grad


def adam_model(p, m, v, g, lr_t, gs):
    """adam_kernel: the three statements of gan_adam1 (common.h:95-100) without contraction."""
    omb1, omb2, eps = adam_consts()
    gr = g.astype(F32) * F32(gs)
    m1 = m + (gr - m) * omb1
    v1 = v + (gr * gr - v) * omb2
    p1 = p - (m1 * F32(lr_t)) / (np.sqrt(v1) + eps)
    return p1.astype(F32), m1.astype(F32), v1.astype(F32)


def lr_t_model(lr, b1, b2, t):
    """adam_begin_kernel: double arithmetic from the fp32 arguments, one rounding."""
    lr, b1, b2 = float(F32(lr)), float(F32(b1)), float(F32(b2))
    return F32(lr * math.sqrt(1.0 - math.pow(b2, t)) / (1.0 - math.pow(b1, t)))


# ---- the comparisons (ONE definition: the GPU tests feed them kernel outputs, the CPU tests the fp32 models and the wrong variants) ------
def _r(err, gate):
    """error / gate of a scalar; a zero gate demands a zero error."""
    if not math.isfinite(err):
        return math.inf
    if gate == 0:
        return 0.0 if err == 0 else math.inf
    return err / gate


def bce_args(target):
    """(loss_scale, grad_scale) of the BCE cases: the generator term unscaled, a discriminator term halved (as the step calls it)."""
    return (1.0, 1.0) if target == 1.0 else (0.5, 0.5)


def check_bce(x, target, grad_scale, ls0, dt, loss, grad, loss_scale=1.0):
    """loss: the fp32 scalar of a call with loss_accumulate = 0 (loss_scale a power of two: that multiply is exact);
    grad: the stored gradient [count] or None.  -> {item: error / gate}."""
    gs = grad_scale * ls0
    ref_l, ref_g = bce_ref(x, target, gs)
    bound = float(np.abs(x.astype(np.float64)).mean() + 1.0)
    res = {'loss': _r(abs(float(loss) - loss_scale * ref_l), abs(loss_scale) * loss_gate('gan_bce_logits', x.size, bound))}
    if grad is not None:
        res['grad'] = ratio(grad, t64(ref_g), bce_grad_gate(ref_g, dt, gs, x.size))
    return res


def check_patchgan(real, fake, ls0, dt, got, lam=100.0, l1=0.0):
    """got: dict with the fp32 scalars gan, disc, optionally gen_total, and the stored gradients g_dfake / d_dreal / d_dfake (or None).
    disc = 0.5 * (r + f): the two means each within their loss gate, halved exactly, plus the ONE rounding of the add
    (0.5 * EPS32 * |disc|).  gen_total: exactly the fp32 gan + lambda * l1 of the stored gan."""
    ref = patchgan_ref(real, fake, ls0)
    n = real.size
    gf = loss_gate('gan_patchgan_losses', n, float(np.abs(fake.astype(np.float64)).mean() + 1.0))
    gr = loss_gate('gan_patchgan_losses', n, float(np.abs(real.astype(np.float64)).mean() + 1.0))
    res = {'gan': _r(abs(float(got['gan']) - ref['gan']), gf),
           'disc': _r(abs(float(got['disc']) - ref['disc']), 0.5 * (gr + gf) + 0.5 * EPS32 * abs(ref['disc']))}
    if got.get('gen_total') is not None:
        want = F32(got['gan']) + F32(lam) * F32(l1)
        res['gen_total'] = 0.0 if F32(got['gen_total']).view(np.uint32) == F32(want).view(np.uint32) else math.inf
    for k, scale in (('g_dfake', ls0), ('d_dreal', 0.5 * ls0), ('d_dfake', 0.5 * ls0)):
        if got.get(k) is not None:
            res[k] = ratio(got[k], t64(ref[k]), bce_grad_gate(ref[k], dt, scale, n))
    return res


def check_l1(a_st, b_st, grad_scale, ls0, dt, loss, grad, loss_scale=1.0):
    """a_st, b_st: the stored dense tensors; loss of a call with loss_accumulate = 0; grad: stored dense gradient or None."""
    a, b = a_st.double().numpy().reshape(-1), b_st.double().numpy().reshape(-1)
    ref_l, ref_g = l1_ref(a, b, grad_scale * ls0)
    res = {'loss': _r(abs(float(loss) - loss_scale * ref_l), abs(loss_scale) * loss_gate('gan_l1', a.size, ref_l))}
    if grad is not None:
        res['grad'] = ratio(grad.reshape(-1), t64(ref_g), l1_grad_gate(ref_g, dt))
    return res


def check_adam(p0, m0, v0, g, gs, lr_t, p1, m1, v1):
    """fp32 numpy arrays: the inputs (g already widened to fp32), the kernel's arguments and what it left -> ratios of m, v, p."""
    mr, vr = adam_moments_ref(m0, v0, g, gs)
    u, pr = adam_update_ref(p0, m1, v1, lr_t)
    gm, gv, gp = adam_gates(m0, v0, g, gs, pr, u)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return {'m': ratio(f(m1), t64(mr), gm), 'v': ratio(f(v1), t64(vr), gv), 'p': ratio(f(p1), t64(pr), gp)}


def table(worst, title):
    """The worst error / gate per entry point and item, in the style of launch_audit.table."""
    lines = [f"== elementwise kernels {title}: worst error / gate"]
    for name in sorted(worst):
        for item in sorted(worst[name]):
            lines.append(f"  {name[4:] if name.startswith('gan_') else name:24s} {item:52s} {worst[name][item]:.3f}")
    return '\n'.join(lines)


def note(worst, name, item, value):
    """Record a ratio under (entry point, item), keeping the worst; returns the value."""
    d = worst.setdefault(name, {})
    d[item] = max(d.get(item, 0.0), float(value))
    return value
