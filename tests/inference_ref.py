"""Inference mode (`model(x, training=False)`), the reference side shared by tests/test_gpu_inference.py,
tests/test_gpu_eval_audit.py and the CPU tests: an fp64 numpy forward built from the oracle's primitives (O.conv2d_fwd,
O.convT2d_fwd, O.act_fwd, O.BN_EPS) with BatchNorm in its inference form and no dropout; calibrated BatchNorm state (random gamma,
a fifth of it negative, random beta, moving statistics near the layer's real ones); the float32 fold, one operation at a time.
Helper module, not a conftest."""
import numpy as np

from oracle import gan_oracle as O


# ---------------------------------------------------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------------------------------------------------
def bn_eval(y, P, name):
    """Keras BatchNormalization(training=False): gamma * (y - moving_mean) * rsqrt(moving_variance + eps) + beta."""
    g, b = P[name + '.gamma'], P[name + '.beta']
    mm, mv = P[name + '.moving_mean'], P[name + '.moving_variance']
    return g * (y - mm) / np.sqrt(mv + O.BN_EPS) + b


def _f64(P):
    return {k: np.asarray(v, np.float64) for k, v in P.items()}


def generator_eval_ref(P, x, calibrate=None):
    """-> (tanh output, bottleneck activation a7).  calibrate(name, y) -> None: called with every BN layer's pre-normalisation
    output before it is normalised (the fixture below sets moving statistics from it)."""
    P = _f64(P)
    h = np.asarray(x, np.float64)
    skips = []
    for i in range(8):
        y = O.conv2d_fwd(h, P[f'down{i}.kernel'], 2)
        if i > 0:
            if calibrate:
                calibrate(f'down{i}', y, P)
            y = bn_eval(y, P, f'down{i}')
        h = O.act_fwd(y, 'lrelu')
        skips.append(h)
    a7 = h
    skips = skips[:-1][::-1]
    for j in range(7):
        y = O.convT2d_fwd(h, P[f'up{j}.kernel'])
        if calibrate:
            calibrate(f'up{j}', y, P)
        h = np.concatenate([O.act_fwd(bn_eval(y, P, f'up{j}'), 'relu'), skips[j]], axis=-1)
    return O.act_fwd(O.convT2d_fwd(h, P['last.kernel']) + P['last.bias'], 'tanh'), a7


def discriminator_eval_ref(P, inp, tar, calibrate=None):
    P = _f64(P)
    h = np.concatenate([inp, tar], axis=-1).astype(np.float64)
    for name, stride in [('down0', 2), ('down1', 2), ('down2', 2), ('conv', 1)]:
        y = O.conv2d_fwd(h, P[name + '.kernel'], stride)
        if name != 'down0':
            if calibrate:
                calibrate(name, y, P)
            y = bn_eval(y, P, name)
        h = O.act_fwd(y, 'lrelu')
    return O.conv2d_fwd(h, P['last.kernel'], 1) + P['last.bias']


def calibrated(P, forward, seed):
    """Non-trivial BatchNorm state: gamma, beta random; moving statistics near the statistics the layer actually sees (so that
    every depth of the network carries signal), perturbed.  `forward(P, calibrate)` walks the network once."""
    rng = np.random.default_rng(seed)
    P = {k: np.array(v, np.float32) for k, v in P.items()}

    def cal(name, y, P64):
        c = y.shape[-1]
        mean, var = y.mean(axis=(0, 1, 2)), y.var(axis=(0, 1, 2))
        P[name + '.gamma'] = (rng.uniform(0.6, 1.4, c) * rng.choice([-1.0, 1.0], c, p=[0.2, 0.8])).astype(np.float32)
        P[name + '.beta'] = rng.normal(0.0, 0.2, c).astype(np.float32)
        P[name + '.moving_mean'] = (mean + 0.3 * np.sqrt(var) * rng.standard_normal(c)).astype(np.float32)
        P[name + '.moving_variance'] = (var * rng.uniform(0.5, 2.0, c) + 1e-3).astype(np.float32)
        for k in ('.gamma', '.beta', '.moving_mean', '.moving_variance'):
            P64[name + k] = P[name + k].astype(np.float64)
    forward(P, cal)
    return P


_CACHE = {}


def gen_params(seed=11, S=256):
    """Calibrated on two images of size S (the statistics a layer sees depend on the image size)."""
    if (seed, S) not in _CACHE:
        P = O.init_generator(1, seed=seed)
        x = O.synthetic_pair(2, S, 1, seed=seed + 100)[0]
        _CACHE[(seed, S)] = calibrated(P, lambda P_, cal: generator_eval_ref(P_, x, cal), seed)
    return _CACHE[(seed, S)]


def disc_params(seed=12):
    key = ('D', seed)
    if key not in _CACHE:
        P = O.init_discriminator(1, True, seed=seed)
        inp, tar = O.synthetic_pair(2, 256, 1, seed=seed + 100)
        _CACHE[key] = calibrated(P, lambda P_, cal: discriminator_eval_ref(P_, inp, tar, cal), seed)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------
# the fold
# ---------------------------------------------------------------------------------------------------------------------
def _np_fold(master, gamma, beta, mean, var, transposed):
    """numpy float32, one IEEE operation at a time (the kernel's contraction is off)."""
    eps = np.float32(O.BN_EPS)
    s = gamma * (np.float32(1.0) / np.sqrt(var + eps))
    bias = beta - mean * s
    w = master.reshape(16, *master.shape[-2:])
    w = np.transpose(w, (0, 2, 1)) if transposed else w          # -> [tap][co][ci]
    return s, bias.astype(np.float32), (w * s[None, :, None]).astype(np.float32)
