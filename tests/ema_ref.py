"""fp64 reference and gate of gan_ema_update (gan_amd/csrc/elementwise.hip; helper of tests/test_cpu_ema.py and
tests/test_gpu_ema.py: numpy only, not a conftest).

The kernel:  d_t = decay, or with a step counter min(decay, (1 + t) / (10 + t));  omd = 1.0f - d_t;  s' = fmaf(w - s, omd, s).

Two checks, both derived, none measured:
  - d_t, as the kernel reports it through `decay_used`, is within ONE fp32 ulp of the fp64 d_t (decay is the fp32 value passed);
  - per element, with omd formed in fp32 from the REPORTED d_t as the kernel forms it,
        ref = s + (w - s) * omd                in fp64 from the fp32 inputs
        |got - ref| <= 2^-23 * (|s| + |w - s| * omd)
    One rounded subtract (relative 2^-24, scaled by omd) plus one rounded fma (relative 2^-24 of a result no larger than
    |s| + |w - s| * omd * (1 + 2^-24)) stay below 2^-24 * (|s| + 2 * |w - s| * omd); the gate is 2^-23 * (|s| + |w - s| * omd).
    The model has no underflow term: it holds where the result and the product are normal numbers or exact.
  - where w == s bitwise the result is s bitwise: w - s = +0, and fma(+0, omd, s) = s.  The one exception IEEE 754 makes is
    s = w = -0: (-0) - (-0) = +0 and (+0) + (-0) = +0, so there the arithmetic above returns +0; bitwise_rule_mask() leaves
    that pair to the gate (which wants a zero)."""
import numpy as np

F32 = np.float32
EPS32 = 2.0 ** -23


def decay_at(decay, step=None):
    """fp64 d_t of the fp32 `decay` at step count `step` (None: no warm-up)."""
    d = float(F32(decay))
    if step is None:
        return d
    t = float(int(step))
    return min(d, (1.0 + t) / (10.0 + t))


def ulp32(x):
    return float(np.spacing(F32(abs(x))))


def decay_ok(decay_used, decay, step=None):
    """The reported d_t is within one fp32 ulp of the fp64 d_t."""
    want = decay_at(decay, step)
    return abs(float(F32(decay_used)) - want) <= ulp32(want)


def omd_of(decay_used):
    """1 - d_t as the kernel forms it: one fp32 subtract."""
    return F32(1.0) - F32(decay_used)


def reference(s, w, decay_used):
    """fp64 s + (w - s) * omd from the fp32 arrays and the fp32 omd."""
    s64, w64 = np.asarray(s, F32).astype(np.float64), np.asarray(w, F32).astype(np.float64)
    return s64 + (w64 - s64) * float(omd_of(decay_used))


def bound(s, w, decay_used):
    s64, w64 = np.asarray(s, F32).astype(np.float64), np.asarray(w, F32).astype(np.float64)
    return EPS32 * (np.abs(s64) + np.abs(w64 - s64) * float(omd_of(decay_used)))


def bitwise_rule_mask(s, w):
    """Elements where w == s bitwise and s is not -0."""
    sb, wb = np.asarray(s, F32).view(np.uint32), np.asarray(w, F32).view(np.uint32)
    return (sb == wb) & (sb != np.uint32(0x80000000))


def element_failures(s, w, got, decay_used):
    """Indices that miss the per-element gate or the bitwise rule."""
    s, w, got = (np.asarray(a, F32).reshape(-1) for a in (s, w, got))
    err = np.abs(got.astype(np.float64) - reference(s, w, decay_used))
    bad = ~(err <= bound(s, w, decay_used))                         # (a NaN fails)
    same = bitwise_rule_mask(s, w)
    bad |= same & (got.view(np.uint32) != s.view(np.uint32))
    return np.flatnonzero(bad)


def worst_ratio(s, w, got, decay_used):
    """max |got - ref| / bound over the elements with a non-zero bound (printed beside the assertions)."""
    s, w, got = (np.asarray(a, F32).reshape(-1) for a in (s, w, got))
    err = np.abs(got.astype(np.float64) - reference(s, w, decay_used))
    b = bound(s, w, decay_used)
    nz = b > 0
    return float((err[nz] / b[nz]).max()) if nz.any() else 0.0


def passes(s, w, got, decay_used, decay, step=None):
    """The whole gate: the reported d_t and every element."""
    return bool(decay_ok(decay_used, decay, step)) and element_failures(s, w, got, decay_used).size == 0


def model_f32(s, w, decay, step=None):
    """numpy float32 model of the kernel in its own operation order -> (new shadow, d_t): d_t rounded once from fp64, one fp32
    subtract, the fma in fp64 (the product of two fp32 numbers is exact there) rounded to fp32."""
    s, w = np.asarray(s, F32), np.asarray(w, F32)
    d = F32(decay_at(decay, step))
    omd = F32(1.0) - d
    diff = (w - s).astype(F32)
    with np.errstate(over='ignore'):
        out = (diff.astype(np.float64) * float(omd) + s.astype(np.float64)).astype(F32)
    return out, d


def closed_form(s0, ws, decay):
    """s_n = d^n s_0 + (1 - d) * sum_k d^(n-1-k) w_k in fp64, constant decay."""
    d = float(F32(decay))
    n = len(ws)
    out = d ** n * np.asarray(s0, np.float64)
    for k, w in enumerate(ws):
        out = out + (1.0 - d) * d ** (n - 1 - k) * np.asarray(w, np.float64)
    return out


def planted(count, seed):
    """(s, w) of `count` elements: N(0, 1) with the special cases planted at the head (as many as fit).  The subnormal cases are
    those whose exact result is a normal number or exact (see the module docstring: the gate has no underflow term)."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(count).astype(F32)
    w = rng.standard_normal(count).astype(F32)
    sub = np.array([1], np.uint32).view(F32)[0]                     # the smallest subnormal
    sub2 = np.array([0x007fffff], np.uint32).view(F32)[0]           # the largest
    cases = [(1.25, 1.25), (0.0, 0.0), (-3.0e-5, -3.0e-5), (sub, sub), (-sub2, -sub2),         # w == s bitwise
             (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.0, 1.0), (-0.0, -1.0),                  # signed zeros
             (sub2, 1.0), (1.0, sub), (-sub, 2.0),                                              # subnormal against normal
             (1e30, 1e-30), (1e-30, 1e30), (-1e30, 1e-30),                                      # 60 orders of magnitude apart
             (1.0, -1.0), (-0.75, 0.75), (0.001, -0.999), (3.0, -2997.0)]                       # opposite signs, cancelling at omd 0.5 / 0.001
    for i, (a, b) in enumerate(cases[:count]):
        s[i], w[i] = a, b
    if count >= 2 * len(cases):                                     # and at the tail, in the last (ragged) vectors
        for i, (a, b) in enumerate(cases):
            s[count - 1 - i], w[count - 1 - i] = a, b
    return s, w
