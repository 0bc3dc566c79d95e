"""Launch audit of a captured training step and of the inference forward (helper of tests/test_gpu_launch_audit.py,
tests/test_gpu_wide_audit.py and tests/test_gpu_eval_audit.py; not a conftest).

record(): every library call the step's capture body makes (Ctx.capture_graph's fn: the eager warm-up step is left out), or an
eager call makes inside Recorder.recording() (the inference calls: nothing of them is captured), with the descriptors the product
code itself built.  replay(): the recorded calls re-issued one at a time, in recorded order, on one stream; before
each call the regions it reads and writes are snapshot through the HIP runtime torch loaded (gan_amd/_lib.py: one runtime per
process), after it the outputs are read back and compared with an fp64 reference computed from the snapshot - so no error
compounds across layers and every gate is a rounding bound of that one call (GATES below).

Every recorded entry point either has a checker here or is named in ALLOWLIST with the reason it is not checked; a call that has
neither fails the audit.

Data-parallel step (tests/test_gpu_ddp_audit.py): IdentitySync is a GradSync of world 2 whose exchange does nothing - the "sum over
ranks" is this rank's own wire contents, so Adam's 1/world halves every update; WireAudit follows the bf16 wire buffers through the
compute calls (who wrote which element, exactly once); AdamEnd checks m, v, master and the NK copies of whole networks after the
Adam graphs' calls; replay(check=...) leaves the calls the one-GPU audit already covers unchecked.

RGB steps (tests/test_gpu_rgb_audit.py, channels = 3): thin_call() is the predicate of the calls that differ from the channels = 1
step (an operand with <= 8 channels), conv_class() / wgrad_class() the plan class of a descriptor as the host tables of
tests/test_cpu_launch_audit.py key it, missing_required() names the required calls no checked row holds, pad_channels() the
image-side buffers whose padding channels are not bit-zero.

Wide sweeps (tests/test_gpu_wide_audit.py): captured_step() is the body it shares with tests/test_gpu_launch_audit.py (build, capture,
reset_step, lattice inputs), outside_classes() the predicate of the calls whose plan class no earlier case has audited,
missing_classes() names the classes a case was added for that none of its checked rows holds.

Option-carrying steps (tests/test_gpu_option_audit.py; dSSIM, MS-SSIM, the Sobel edge term, DiffAugment, least-squares GAN loss, the
learning-rate schedule, CycleGAN's image pools): option_step() builds, captures and resets such a step beside captured_step(); OptionStart puts the
option state (DiffAugment table and counter, pools, mask counters, lr_now and the schedule's counter, loss scale) at a known start;
the checkers of gan_dssim, gan_msssim, gan_edge_l1, gan_diffaug_draw, gan_diffaug_apply, gan_lsq_logits, gan_patchgan_losses_lsq,
gan_pool_exchange and gan_adam_begin_sched each split into a thin generator that reads the device and a device-free *_ratios function,
which tests/test_cpu_option_audit.py puts right and planted wrong results through; option_call() is the predicate of the calls such
an audit checks, same_as_plain() the rule by which the unchecked rest earns AS_ONE_GPU, issue() the unchecked serial re-issue the
captured graph is compared with; near_target() gives an MS-SSIM step a target near the generator's own output, the inputs for which
the loss gate of gan_msssim is derived."""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import re
import time

import numpy as np
import torch
import torch.nn.functional as F

from gan_amd import _lib as L

# ---- gates ------------------------------------------------------------------------------------------------------------------
# A stored 16-bit value: |got - ref| <= K_ULP * ulp(ref) + C_ACC * EPS32 * sum|terms|.  K_ULP = 1: round-to-nearest storage is half an
# ulp off the exact fp32 result, and the other half covers a ref that sits on the other side of a binade edge.  C_ACC: the fp32
# accumulation of at most ~2^12 partial sums per output (16 taps x K/32 MFMA blocks x split-K slabs): the random-walk error of such a
# blocked sum stays within sqrt(4096) = 64 unit roundoffs of sum|terms| (the worst-case bound, 4096 eps, would hide a lost slab).
# sum|terms| is the cheap upper bound max|x| * sum|w| per output channel (abs_bound; for wgrad max|big| * sum|small| per column):
# an exact |x| x |w| pass would double the reference's cost, and the term only matters where the result cancels.
# fp32 outputs (exact-MFMA path, slabs, partials): the same formula, ulp of fp32.  The finishing slab reduce (GanNormFuse) and the
# fused backward epilogue round the conv result to storage before they use it (splitk_norm.h: "as stored"): the forward form is
# checked against the stored y it wrote, the backward form (whose da is never stored) carries one extra ulp of da, times the
# derivative, through dz, the statistics and dy.
EPS32 = 2.0 ** -23
C_ACC = 64.0
K_ULP = 1.0
MANT = {L.F32: 23, L.BF16: 7, L.F16: 10}
MIN_ULP = {L.F32: 2.0 ** -149, L.BF16: 2.0 ** -133, L.F16: 2.0 ** -24}
TDT = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16}
ACC = C_ACC * EPS32

# Entry points the planner / builder only QUERY (host side, enqueue nothing): passed straight through, never recorded.
QUERIES = {'gan_conv_plan_info', 'gan_conv_workspace_bytes', 'gan_wgrad_plan_info', 'gan_wgrad_workspace_bytes', 'gan_conv_tap_shared',
           'gan_wgrad_adam_fused', 'gan_wgrad_wire_direct', 'gan_conv_stack_eligible', 'gan_conv_stack_plan_bytes', 'gan_conv_stack_plan',
           'gan_conv_stack_barrier_bytes', 'gan_norm_workspace_bytes', 'gan_norm_sync_bytes', 'gan_norm_sync_error_offset',
           'gan_set_option', 'gan_get_option', 'gan_launch_log', 'gan_version', 'gan_crc32c'}

# Recorded entry points that are not checked here, and why.
ALLOWLIST = {
    'gan_bce_logits': 'loss scalar + (sigmoid(x)-t)/n row: per element against fp64 (cap-crossing counts, planted +-0 / +-100 logits, scale '
                      'state, loss_accumulate) by test_gpu_elementwise::test_bce_logits',
    'gan_patchgan_losses': 'the three BCE terms in one pass: per element against fp64 by test_gpu_elementwise::test_patchgan_losses',
    'gan_l1': 'mean |a-b| scalar + sign row (sign(0) = 0): per element against fp64 on pitched views by test_gpu_elementwise::test_l1',
    'gan_sum3': 'three scalars added: bit-equal to the fp32 (a+b)+c by test_gpu_elementwise::test_sum3',
    'gan_adam_begin': 'step counter + lr_t scalar: within one ulp of the extended-precision value at t = 1..100,000 and kept on a skipped '
                      'step by test_gpu_elementwise::test_adam_begin; read back here as the input of every fused-Adam check',
    'gan_adam_tf': 'Adam of the norm / bias vectors (no planner choice): m, v, p per element against fp64 (cap-crossing count, wire '
                   'gradient, scale state, skipped step) by test_gpu_elementwise::test_adam_tf; data-parallel step: every vector element '
                   'against fp64 after the Adam graphs (AdamEnd.check)',
    'gan_adam_prepare_multi': 'the flat multi-tensor Adam + NK refresh: bit-equal to gan_adam_tf + gan_weights_prepare (both checked by '
                              'test_gpu_elementwise) in test_gpu_ops::test_fused_adam_prepare_equals_adam_then_prepare; '
                              'the NK copies it writes are the weights every later conv reads, decoded from the device here; data-parallel '
                              'step (segment tables, wire gradient, grad_scale 1/world): every kernel element and NK copy after the Adam '
                              'graphs (AdamEnd.check)',
    'gan_weights_prepare_multi': 'NK copies of the master: bit-equal to the cast master in both layouts, padding zeroed, by '
                                 'test_gpu_elementwise::test_weights_prepare_multi; decoded from the device copy by every conv check here',
    'gan_pack': 'fp32 -> storage cast of the inputs: bit-equal to round-to-nearest-even on ties, overflow, subnormals, inf, NaN by '
                'test_gpu_elementwise::test_pack_unpack_copy_view',
    'gan_pack_multi': 'as gan_pack, 1 and 4 pairs: test_gpu_elementwise::test_pack_unpack_copy_view',
    'gan_unpack': 'exact widening: test_gpu_elementwise::test_pack_unpack_copy_view',
    'gan_copy_view': 'a typed copy between views: bit-equal, nothing outside the view written, by '
                     'test_gpu_elementwise::test_pack_unpack_copy_view',
    'gan_dropout_mask': 'counter-hash Bernoulli mask: bit-equal to the integer SplitMix64 reference (elementwise_ref.mask_ref) by '
                        'test_gpu_elementwise::test_dropout_masks; read here as an input of every dropout check',
    'gan_dropout_mask_multi': 'as gan_dropout_mask, with the draw counter and the unaligned byte path: test_gpu_elementwise::test_dropout_masks',
    'gan_grads_check': 'fp16 inf/nan flag of the loss scale: one inf / nan at the first, last (second trip) and a middle element by '
                       'test_gpu_elementwise::test_grads_check; the state machine by test_gpu_configs::test_loss_scale_state_machine',
    'gan_loss_scale_update': 'fp16 loss-scale state machine: test_gpu_configs::test_loss_scale_state_machine',
    'gan_grad_pack': 'data-parallel wire format: bit-equal to the bf16 round-to-nearest-even cast by test_gpu_elementwise::test_grad_pack_unpack; '
                     'in a data-parallel capture (replay(wire=...)) its RANGE is recorded by check_pack_range: every element of the wire '
                     'buffers written exactly once, by a direct wgrad or by a pack (WireAudit.coverage)',
    'gan_grad_unpack': 'data-parallel wire format: bit-equal to one fp32 multiply by test_gpu_elementwise::test_grad_pack_unpack; the fp16 '
                       'data-parallel step: the whole unpacked buffer bit-equal to wire * 1/world in AdamEnd.check',
    'gan_tile_gather_u8': 'uint8 source -> typed tiles through the normalize table: bit-equal to lut[src] of every tile (origins pulled '
                          'back at the edges, a column window, sub-ranges of tiles, pad channels as gan_pack leaves them) for f32 / bf16 / '
                          'f16 by test_gpu_tiles::test_gather_is_bit_exact_and_leaves_the_pad_channels_as_pack_does',
    'gan_tile_blend': 'hat-weighted blend of the tiles: every pixel against the fp64 reference tests/tile_ref.py (gate 1e-5) by '
                      'test_gpu_tiles::test_blend_matches_the_fp64_reference; split launches bit-equal to one launch, and nothing outside '
                      'the covered pixels written, by test_split_launches_and_repeated_calls_give_the_same_bits / '
                      'test_a_launch_owns_only_the_pixels_its_tiles_cover',
    'gan_conv_stack_launch': 'layer stacks (conv.stack, off by default; out of scope)',
    'gan_norm_stats_partial': 'norm.fin_in_apply only (off by default; out of scope)',
    'gan_norm_finalize_act_fwd': 'norm.fin_in_apply only (off by default; out of scope)',
}


def ulp(ref, dt):
    """ulp of the storage type at |ref| (fp64 tensor)."""
    _, e = torch.frexp(ref.abs())
    u = torch.ldexp(torch.ones_like(ref), (e - 1 - MANT[dt]).to(torch.int32))
    return torch.where(ref == 0, MIN_ULP[dt], torch.clamp(u, min=MIN_ULP[dt]))


def ratio(got, ref, gate):
    """Worst |got - ref| / gate (0 for empty)."""
    if got.numel() == 0:
        return 0.0
    d = (got.double() - ref.double()).abs()
    if not torch.isfinite(got.double()).all():
        return math.inf
    return float((d / gate.clamp(min=1e-300)).max())


# ---- device memory through torch's HIP runtime ---------------------------------------------------------------------------------
_hip = None


def hip():
    global _hip
    if _hip is None:
        path = None
        with open('/proc/self/maps') as f:           # the libamdhip64 torch loaded (gan_amd/_lib.py: ONE runtime per process)
            for ln in f:
                if 'libamdhip64' in ln:
                    path = ln.split()[-1]
                    break
        if path is None:
            raise RuntimeError("the HIP runtime is not loaded (import torch and touch the GPU first)")
        _hip = C.CDLL(path)
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    return _hip


def read(ptr, count, dt=L.F32, tdtype=None):
    """count elements at device address ptr -> CPU tensor (storage type)."""
    t = torch.empty(int(count), dtype=tdtype or TDT[dt])
    if count:
        rc = hip().hipMemcpy(t.data_ptr(), ptr, t.numel() * t.element_size(), 2)      # hipMemcpyDeviceToHost
        if rc:
            raise RuntimeError(f"hipMemcpy D2H failed ({rc})")
    return t


class View:
    """Snapshot of a GanTensor: the whole span it addresses (pixels x pitch, last pixel up to c) and its dense [n,h,w,c] part."""

    def __init__(self, t, dt):
        self.t, self.dt = t, dt
        self.rows = t.n * t.h * t.w
        self.span = (self.rows - 1) * t.pitch + t.c if self.rows else 0
        self.raw = read(t.ptr, self.span, dt)

    @classmethod
    def of_host(cls, raw, t, dt):
        """A snapshot made of a host tensor (the CPU models of tests/test_cpu_launch_audit.py): raw = the span's elements."""
        v = cls.__new__(cls)
        v.t, v.dt, v.rows, v.raw = t, dt, t.n * t.h * t.w, raw
        v.span = raw.numel()
        return v

    def dense(self):
        t = self.t
        return torch.as_strided(self.raw, (t.n, t.h, t.w, t.c), (t.h * t.w * t.pitch, t.w * t.pitch, t.pitch, 1)).double()

    def changed_channels(self, other):
        """channel index (position % pitch) of every stored element that differs bitwise from `other`'s snapshot of the span."""
        it = torch.int16 if self.raw.element_size() == 2 else torch.int32
        pos = (self.raw.view(it) != other.raw.view(it)).nonzero().reshape(-1)
        return pos % self.t.pitch


def untouched(before, after, c0, c1):
    """Gate entry for stored bytes a call must not change: everything in the span outside channels [c0, c1)."""
    ch = before.changed_channels(after)
    return math.inf if int(((ch < c0) | (ch >= c1)).sum()) else 0.0


def unchanged(before, after, c0, c1):
    """Gate entry: channels [c0, c1) of the span must keep their bits."""
    ch = before.changed_channels(after)
    return math.inf if int(((ch >= c0) & (ch < c1)).sum()) else 0.0


# ---- fp64 references --------------------------------------------------------------------------------------------------------
def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def conv_ref(op, x, w, stride):
    """The four conv entry points from the device operand w[16][rows][x.c] (row = y channel, column = x channel for all four).
    op 0 conv_fwd / 3 convT_dgrad gather from the fine grid, op 1 conv_dgrad / 2 convT_fwd scatter onto it:
    y[o] = sum_tap w[tap] x[o*s - 1 + tap]  /  y[o*s - 1 + tap] += w[tap] x[o]   (tap = kh*4 + kw)."""
    yc, xc = w.shape[1], w.shape[2]
    w4 = w.reshape(4, 4, yc, xc)
    if op in (0, 3):
        return nhwc(F.conv2d(nchw(x), w4.permute(2, 3, 0, 1).contiguous(), stride=stride, padding=1))
    return nhwc(F.conv_transpose2d(nchw(x), w4.permute(3, 2, 0, 1).contiguous(), stride=stride, padding=1))


def abs_bound(x, w):
    """Upper bound of sum|terms| of every output of conv_ref: max|x| times the sum of |w| over taps and x channels of its y channel
    (per channel, broadcast over pixels - the cheap bound; the exact one, conv_ref(|x|, |w|), doubles the reference's cost)."""
    return float(x.abs().max()) * w.abs().sum((0, 2))


def wgrad_ref(big, small, stride, big_c, small_c):
    """dw[tap][b][s] = sum_{n,o} big[n, o*s - 1 + tap, b] small[n, o, s] (HWIO for Conv2D, (kh,kw,cout,cin) for Conv2DTranspose)."""
    bg, sm = nchw(big[..., :big_c]), nchw(small[..., :small_c])
    dw = torch.nn.grad.conv2d_weight(bg, (small_c, big_c, 4, 4), sm, stride=stride, padding=1)
    return dw.permute(2, 3, 1, 0).reshape(16, big_c, small_c)


def act_f(z, act, slope):
    if act == L.ACT_LRELU:
        return torch.where(z > 0, z, z * slope)
    if act == L.ACT_RELU:
        return z.clamp(min=0)
    if act == L.ACT_TANH:
        return torch.tanh(z)
    return z


def act_d(z, act, slope):
    """(derivative, derivative on the other side of the kink): z is the pre-activation value (for tanh: the activation)."""
    if act == L.ACT_LRELU:
        return torch.where(z > 0, 1.0, slope).double(), torch.where(z >= 0, 1.0, slope).double()
    if act == L.ACT_RELU:
        return (z > 0).double(), (z >= 0).double()
    if act == L.ACT_TANH:
        d = 1.0 - z * z
        return d, d
    one = torch.ones_like(z)
    return one, one


def kink_d(z, zbound, act, slope):
    """Derivative where the fp32 z of the kernel may sit on either side of a kink (|z| <= its rounding bound): both accepted."""
    d, d2 = act_d(z, act, slope)
    near = z.abs() <= zbound
    lo = torch.where(near, torch.minimum(d, d2), d)
    hi = torch.where(near, torch.maximum(d, d2), d)
    return lo, hi


def between(got, lo, hi, gate):
    """|got - [lo, hi]| / gate: an interval reference (an element whose derivative may be taken on either side of a kink)."""
    g = got.double()
    if not torch.isfinite(g).all():
        return math.inf
    d = torch.clamp(lo - g, min=0) + torch.clamp(g - hi, min=0)
    return float((d / gate.clamp(min=1e-300)).max()) if d.numel() else 0.0


def grp(t, groups):
    """[n,h,w,c] -> [groups, rows per group, c]"""
    return t.reshape(groups, -1, t.shape[-1])


def stats_gate(y, ey, groups):
    """mean / biased variance of y ([n,h,w,c], fp64) per group and the bounds of the kernel's values: ey = per-element bound of the
    y the kernel summed, plus the fp32 accumulation of the sums."""
    yg, eg = grp(y, groups), grp(ey, groups)
    R = yg.shape[1]
    m = yg.mean(1)
    var = torch.clamp(((yg - m.unsqueeze(1)) ** 2).mean(1), min=0.0)
    dm = eg.mean(1) + ACC * yg.abs().mean(1)
    dvar = ACC * (yg * yg).mean(1) + 2 * (yg.abs() * eg).mean(1) + 2 * m.abs() * dm
    return m, var, dm, dvar, R


def rstd_of(var, dvar, eps):
    r = 1.0 / torch.sqrt(var + eps)
    dr = 0.5 * r ** 3 * dvar + 4 * EPS32 * r
    return r, dr


# ---- recording ----------------------------------------------------------------------------------------------------------------
class Call:
    def __init__(self, name, fn, args):
        self.name, self.fn, self.args = name, fn, args
        self.label = ''
        self.result = None


class _Wrap:
    def __init__(self, rec, name, fn):
        self.rec, self.name, self.fn = rec, name, fn

    def __call__(self, *args):
        if self.rec.active:
            self.rec.calls.append(Call(self.name, self.fn, args))
        return self.fn(*args)


class Recorder:
    """Wraps the gan_* entry points of the loaded library (before the step object is built: the op lists hold the bound functions)
    and records the calls made while Ctx.capture_graph runs its body, or inside `with rec.recording():` around an eager call."""

    def __init__(self, monkeypatch):
        self.lib = L.load()
        self.calls, self.active = [], False
        self.graph_starts = []
        self.orig = {}
        for name in L.SYMBOLS:
            if name in QUERIES:
                continue
            fn = getattr(self.lib, name)
            self.orig[name] = fn
            monkeypatch.setattr(self.lib, name, _Wrap(self, name, fn))

    @contextlib.contextmanager
    def recording(self):
        """Record the calls an eager piece of product code makes (an inference call: call.infer(fold=True), infer_tiled, ...)."""
        was, self.active = self.active, True
        try:
            yield self
        finally:
            self.active = was

    def hook_capture(self, monkeypatch):
        """Record inside the body of every Ctx.capture_graph (patched on the class: an instance attribute would tie the context into a
        reference cycle whose later collection - inside another capture - destroys graphs mid-capture)."""
        from gan_amd.nets import Ctx
        orig = Ctx.capture_graph
        rec = self

        def capture_graph(ctx, fn, *a, **k):
            def body():
                rec.graph_starts.append(len(rec.calls))          # one entry per captured graph, in capture order
                rec.active = True
                try:
                    fn()
                finally:
                    rec.active = False
            return orig(ctx, body, *a, **k)
        monkeypatch.setattr(Ctx, 'capture_graph', capture_graph)


def _nets_of(obj):
    """[(tag, net)] of a step object (nets()), or of an inference call / model object (or a list of them), which hold one `.net`."""
    if hasattr(obj, 'nets'):
        nets = obj.nets()
        tags = ['G', 'D'] if len(nets) == 2 else ['Gg', 'Gf', 'Dx', 'Dy'][:len(nets)]
        return list(zip(tags, nets))
    out = []
    for o in obj if isinstance(obj, (list, tuple)) else [obj]:
        net = getattr(o, 'net', None)
        if net is not None and all(net is not n for _, n in out):
            out.append(('G' if type(net).__name__ == 'GeneratorNet' else 'D', net))
    return out


def label_calls(calls, step):
    """Layer label of every call: the op tuple that holds its descriptor (label + shape), and the network tensor its weight /
    gradient pointer lies in.  `step`: a step object, or an inference call / model object (or a list of them): these have no nets();
    their weights are the network's NK copies (P.tr / P.nat) or the folded ones (FoldedParams.nk), and their fold call is given the
    tensors it must leave alone (Call.guards: the master, nat, tr and the moving statistics, check_fold)."""
    by_addr = {}
    seen = set()

    def walk(o, depth=0):
        if id(o) in seen or depth > 4:
            return
        seen.add(id(o))
        if isinstance(o, (list, tuple)):
            if len(o) >= 3 and callable(o[0]) and isinstance(o[1], tuple) and isinstance(o[2], str):
                for a in o[1]:
                    obj = getattr(a, '_obj', None)
                    if obj is not None:
                        meta = o[3] if len(o) > 3 and isinstance(o[3], dict) else {}
                        by_addr[C.addressof(obj)] = f"{o[2]} {meta.get('shape', '')}".strip()
                return
            for e in o:
                walk(e, depth + 1)
        elif isinstance(o, dict):
            for e in o.values():
                walk(e, depth + 1)
        elif hasattr(o, '__dict__') and type(o).__module__.startswith('gan_amd'):
            for e in vars(o).values():
                walk(e, depth + 1)
    walk(step)
    ranges = []
    folds = {}
    for tag, net in _nets_of(step):
        P = net.params
        Fo = net.__dict__.get('_folded')
        if Fo is not None:
            for name, t in Fo.nk.items():
                ranges.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), f"{tag}.{name}.folded"))
            folds[Fo._table.data_ptr()] = (f"{tag} fold", [P.master] + list(P.nat.values()) + list(P.tr.values()) + list(P.state.values()))
        for name, (o, shape) in P.entries.items():
            n = int(np.prod(shape))
            for which in ('master', 'grad', 'm', 'v'):
                base = getattr(P, which).data_ptr() + 4 * o
                ranges.append((base, base + 4 * n, f"{tag}.{name}"))
        for name in P.nat:
            for t in (P.nat[name], P.tr[name]):
                ranges.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), f"{tag}.{name}"))

    def owner(ptr):
        for a, b, nm in ranges:
            if ptr and a <= ptr < b:
                return nm
        return ''
    for c in calls:
        if c.name == 'gan_bn_fold_multi' and c.args[0] in folds:
            c.label, c.guards = folds[c.args[0]]
            continue
        obj = getattr(c.args[0], '_obj', None) if c.args else None
        lab = by_addr.get(C.addressof(obj), '') if obj is not None else ''
        w = ''
        if isinstance(obj, L.GanConvDesc):
            w = owner(obj.w)
        elif isinstance(obj, L.GanWgradDesc):
            w = owner(obj.dw) or (owner(L.GanAdamFuse.from_address(obj.adam_fuse).master) if obj.adam_fuse else '')
        elif isinstance(obj, (L.GanNormDesc, L.GanNormBwdDesc)):
            w = owner(obj.gamma)
        elif c.name == 'gan_bias_grad':
            w = owner(c.args[2])                 # (no descriptor: the bias whose gradient it writes)
        c.label = (w + ' ' + lab).strip() or c.name


# ---- checkers: generators that snapshot, yield (the call runs), then read back and return {item: worst error / gate} --------------
OPS = {'gan_conv2d_fwd': 0, 'gan_conv2d_dgrad': 1, 'gan_convT2d_fwd': 2, 'gan_convT2d_dgrad': 3}


def conv_plan(d, op):
    info = (C.c_int32 * 5)()
    L.check(L.load().gan_conv_plan_info(C.byref(d), op, info), "conv_plan_info")
    ts = L.load().gan_conv_tap_shared(C.byref(d), op)
    return list(info), ts


def conv_pre(op, x, w, bias, stride):
    """(fp64 pre-activation output of a conv launch, fp32 accumulation bound of each of its elements): check_conv's reference, on
    host tensors (x [n,h,w,c], w [16][rows][x.c], bias [rows] or None) so that tests/test_cpu_launch_audit.py can put models of the
    kernel - a right one and wrong ones - through the very gate the device values go through."""
    ref = conv_ref(op, x, w, stride)
    S = abs_bound(x, w).expand_as(ref)
    if bias is not None:
        ref = ref + bias
        S = S + bias.abs()
    return ref, ACC * S


def y_gate(ref, eacc, act, slope, ydt):
    """(expected stored output, its gate) of a launch without a fused backward epilogue: check_conv's 'y' item."""
    out = act_f(ref, act, slope)
    return out, K_ULP * ulp(out, ydt) + eacc


def check_conv(call):
    d = call.args[0]._obj
    op = OPS[call.name]
    dt = d.dtype
    info, ts = conv_plan(d, op)
    bf = L.GanBwdFuse.from_address(d.bwd_fuse) if d.bwd_fuse else None
    nf = L.GanNormFuse.from_address(d.norm_fuse) if d.norm_fuse else None
    full = info[4] == -1 and nf is not None
    partials = info[4] > 0 and d.stats_partial and d.stats_groups > 0
    call.plan = f"op{op} tile {info[0]}x{info[1]} split {info[2]} par {info[3]} stats {info[4]} ts {ts}" + \
        (" bwd_fuse" if bf else "") + (" norm_fuse" if full else "")
    ydt = L.F32 if d.y_f32 else dt
    xv = View(d.x, dt)
    x = xv.dense()
    # rows [0, y.c) of every tap: the extent the kernels read.  (D's dx dgrad is given a pointer advanced by some rows into the
    # operand: whole [16][w_rows] tables from there would end that many rows behind the allocation.)
    nw = (15 * d.w_rows + d.y.c) * d.x.c
    w = torch.zeros(16 * d.w_rows * d.x.c, dtype=TDT[dt])
    w[:nw] = read(d.w, nw, dt)
    w = w.double().reshape(16, d.w_rows, d.x.c)[:, :d.y.c]
    bias = read(d.bias, d.y.c).double() if d.bias else None
    y0 = View(d.y, ydt)
    pre = {}
    if bf is not None:
        pre['ref'] = View(bf.ref, dt).dense()
        pre['add'] = View(bf.add, dt).dense() if bf.add.ptr else None
        G = d.stats_groups if bf.mean else 0
        if bf.mean:
            pre['mean'] = read(bf.mean, G * bf.cols).double().reshape(G, bf.cols)
            pre['rstd'] = read(bf.rstd, G * bf.cols).double().reshape(G, bf.cols)
            pre['gamma'] = read(bf.gamma, bf.cols).double()
            pre['beta'] = read(bf.beta, bf.cols).double()
        if bf.dropmask:
            pre['mask'] = _mask(bf.dropmask, d.y.n, d.y.h, d.y.w, bf.cols, bf.mask_pitch)
    if full:
        out0 = View(nf.out, dt)
        G = d.stats_groups
        C_ = nf.out.c
        if nf.gamma:
            pre['ngamma'] = read(nf.gamma, C_).double()
            pre['nbeta'] = read(nf.beta, C_).double()
        if nf.moving_mean:
            pre['mm'] = read(nf.moving_mean, C_).double()
            pre['mv'] = read(nf.moving_var, C_).double()
        if nf.dropmask:
            pre['nmask'] = _mask(nf.dropmask, d.y.n, d.y.h, d.y.w, C_, C_)
        if nf.dgamma:
            pre['dg'] = read(nf.dgamma, C_).double()
            pre['db'] = read(nf.dbeta, C_).double()
    yield
    res = {}
    y1 = View(d.y, ydt)
    yg = y1.dense()
    ref, eacc = conv_pre(op, x, w, bias, d.stride)
    assert tuple(ref.shape) == (d.y.n, d.y.h, d.y.w, d.y.c), (call.name, tuple(ref.shape), (d.y.n, d.y.h, d.y.w, d.y.c))
    if bf is None:
        out, gate = y_gate(ref, eacc, d.act, d.slope, ydt)
        res['y'] = ratio(yg, out, gate)
        res['y untouched outside y.c'] = untouched(y0, y1, 0, d.y.c)
        if partials:
            G = d.stats_groups
            chunks = info[4]
            p = read(d.stats_partial, G * chunks * d.y.c * 2).double().reshape(G, chunks, d.y.c, 2).sum(1)
            ys = grp(yg, G)                          # the epilogues sum the STORED values (conv_gemm.hip): no rounding allowance
            res['stats sum'] = ratio(p[..., 0], ys.sum(1), ACC * ys.abs().sum(1))
            res['stats sumsq'] = ratio(p[..., 1], (ys * ys).sum(1), ACC * (ys * ys).sum(1))
        if full:
            res.update(_norm_fuse_fwd(d, nf, pre, out0, ref, eacc, yg, dt))
        return res
    # dgrad with the layer-below backward in its epilogue (GanBwdFuse)
    cols = bf.cols
    da = ref[..., :cols]
    ea = eacc[..., :cols] + K_ULP * ulp(da, dt)      # the epilogue rounds da to storage before it adds `add` ("as stored")
    if pre['add'] is not None:
        da = da + pre['add'][..., :cols]
        ea = ea + ACC * pre['add'][..., :cols].abs()
    m2 = 2.0 * pre['mask'] if 'mask' in pre else torch.ones_like(da)
    G = d.stats_groups if bf.mean else 1
    if bf.mean:
        r = pre['ref'][..., :cols]
        rg = grp(r, G)
        xhat = ((rg - pre['mean'].unsqueeze(1)) * pre['rstd'].unsqueeze(1)).reshape(r.shape)
        z = grp(xhat, G) * pre['gamma'] + pre['beta']
        zb = 8 * EPS32 * (grp(xhat, G).abs() * pre['gamma'].abs() + pre['beta'].abs()) + 1e-30
        lo, hi = kink_d(z.reshape(r.shape), zb.reshape(r.shape), bf.act, bf.slope)
    else:
        a = pre['ref'][..., :cols]
        lo, hi = kink_d(a, torch.zeros_like(a), bf.act, bf.slope)     # act'(a): a == 0 takes either side
    zlo, zhi = torch.minimum(da * lo * m2, da * hi * m2), torch.maximum(da * lo * m2, da * hi * m2)
    ez = ea * hi.abs() * m2
    if not full:
        res['dz'] = between(yg[..., :cols], zlo, zhi, K_ULP * ulp(zhi, dt) + ez)
        if d.y.c > cols:
            rest = ref[..., cols:]
            res['plain gradient c>=cols'] = ratio(yg[..., cols:], rest, K_ULP * ulp(rest, dt) + eacc[..., cols:])
        res['y untouched outside y.c'] = untouched(y0, y1, 0, d.y.c)
        if partials and bf.mean:
            chunks = info[4]
            p = read(d.stats_partial, G * chunks * cols * 2).double().reshape(G, chunks, cols, 2).sum(1)
            dz = grp(yg[..., :cols], G)                  # the stored dz (checked above), its unrounded value within half an ulp
            xh = grp(xhat, G)
            u = 0.5 * ulp(dz, dt)
            res['bwd sum dz'] = ratio(p[..., 0], dz.sum(1), ACC * dz.abs().sum(1) + u.sum(1))
            res['bwd sum dz*xhat'] = ratio(p[..., 1], (dz * xh).sum(1), ACC * (dz * xh).abs().sum(1) + (u * xh.abs()).sum(1) +
                                           4 * EPS32 * (dz * xh).abs().sum(1))
        return res
    # GanNormFuse backward: the launch finishes the layer below (dy, dgamma, dbeta); dz never stored
    out1 = View(nf.out, dt)
    res['y[:cols] untouched'] = unchanged(y0, y1, 0, cols)
    res['y untouched outside y.c'] = untouched(y0, y1, 0, d.y.c)
    if d.y.c > cols:
        rest = ref[..., cols:]
        res['plain gradient c>=cols'] = ratio(yg[..., cols:], rest, K_ULP * ulp(rest, dt) + eacc[..., cols:])
    # the kink interval is narrow (|z| within a few eps): take the derivative of the reference side, count the rest as its bound
    dz = da * lo * m2
    edz = ez + (da * (hi - lo) * m2).abs()
    xh = grp(xhat, G)
    dzg, eg = grp(dz, G), grp(edz, G)
    R = dzg.shape[1]
    s1, s2 = dzg.mean(1, keepdim=True), (dzg * xh).mean(1, keepdim=True)
    e1 = eg.mean(1, keepdim=True) + ACC * dzg.abs().mean(1, keepdim=True)
    e2 = (eg * xh.abs()).mean(1, keepdim=True) + ACC * (dzg * xh).abs().mean(1, keepdim=True)
    gr = (pre['gamma'] * pre['rstd']).unsqueeze(1)
    dy = gr * (dzg - s1 - xh * s2)
    edy = gr.abs() * (eg + e1 + xh.abs() * e2) + 4 * EPS32 * gr.abs() * (dzg.abs() + s1.abs() + (xh * s2).abs())
    got = grp(out1.dense(), G)
    res['norm_fuse dy'] = ratio(got, dy, K_ULP * ulp(dy, dt) + edy)
    res['norm_fuse out untouched outside c'] = untouched(out0, out1, 0, nf.out.c)
    if nf.dgamma:
        acc = float(nf.accumulate)
        dg = read(nf.dgamma, cols).double()
        db = read(nf.dbeta, cols).double()
        rg_ = (dzg * xh).sum((0, 1)) + acc * pre['dg']
        rb_ = dzg.sum((0, 1)) + acc * pre['db']
        res['norm_fuse dgamma'] = ratio(dg, rg_, (eg * xh.abs()).sum((0, 1)) + ACC * ((dzg * xh).abs().sum((0, 1)) + acc * pre['dg'].abs()))
        res['norm_fuse dbeta'] = ratio(db, rb_, eg.sum((0, 1)) + ACC * (dzg.abs().sum((0, 1)) + acc * pre['db'].abs()))
    return res


def _mask(ptr, n, h, w, c, pitch):
    raw = read(ptr, (n * h * w - 1) * pitch + c, tdtype=torch.uint8)
    return torch.as_strided(raw, (n, h, w, c), (h * w * pitch, w * pitch, pitch, 1)).double()


def _norm_fuse_fwd(d, nf, pre, out0, ref, eacc, yg, dt):
    """GanNormFuse forward: the finishing reduce takes mean / rstd / moving averages and out from y AS STORED (splitk_norm.h: the
    arithmetic of reduce + stats_finalize + norm_act_fwd), so the reference is computed from the stored y - itself checked against
    the fp64 convolution above - with the gates of those separate launches."""
    res = {}
    G = d.stats_groups
    C_ = nf.out.c
    y = yg[..., :C_]
    m, var, dm, dvar, R = stats_gate(y, torch.zeros_like(y), G)
    rs, drs = rstd_of(var, dvar, nf.eps)
    gm = read(nf.mean, G * C_).double().reshape(G, C_)
    gr = read(nf.rstd, G * C_).double().reshape(G, C_)
    res['norm_fuse mean'] = ratio(gm, m, dm + 4 * EPS32 * m.abs())
    res['norm_fuse rstd'] = ratio(gr, rs, drs)
    if nf.moving_mean:
        mm, mv = pre['mm'].clone(), pre['mv'].clone()
        emm, emv = torch.zeros_like(mm), torch.zeros_like(mv)
        adj = R / max(R - 1, 1)
        k = 1.0 - nf.momentum
        for g in range(G):                       # once per group, in order
            mm = mm + (m[g] - mm) * k
            mv = mv + (var[g] * adj - mv) * k
            emm = emm * nf.momentum + k * dm[g] + 4 * EPS32 * (mm.abs() + m[g].abs())
            emv = emv * nf.momentum + k * dvar[g] * adj + 4 * EPS32 * (mv.abs() + var[g].abs() * adj)
        res['norm_fuse moving_mean'] = ratio(read(nf.moving_mean, C_).double(), mm, emm)
        res['norm_fuse moving_var'] = ratio(read(nf.moving_var, C_).double(), mv, emv)
    yg_ = grp(y, G)
    xhat = (yg_ - m.unsqueeze(1)) * rs.unsqueeze(1)
    gam, bet = pre['ngamma'], pre['nbeta']
    z = xhat * gam + bet
    ez = gam.abs() * (rs.unsqueeze(1) * dm.unsqueeze(1) + (yg_ - m.unsqueeze(1)).abs() * drs.unsqueeze(1)) \
        + 4 * EPS32 * ((xhat * gam).abs() + bet.abs())
    m2 = 2.0 * grp(pre['nmask'], G) if 'nmask' in pre else torch.ones_like(z)
    out = act_f(z * m2, nf.act, nf.slope)
    out1 = View(nf.out, dt)
    got = grp(out1.dense(), G)
    res['norm_fuse out'] = ratio(got, out, K_ULP * ulp(out, dt) + ez * m2)
    res['norm_fuse out untouched outside c'] = untouched(out0, out1, 0, C_)
    return res


def wgrad_plan(d):
    """check_wgrad's plan string from the host planner alone."""
    info = (C.c_int32 * 4)()
    L.check(L.load().gan_wgrad_plan_info(C.byref(d), info), "wgrad_plan_info")
    return f"wgrad tile {info[0]}x{info[1]} split {info[2]} fold {info[3]}" + (" adam_fuse" if d.adam_fuse else "") + \
        (" acc" if d.accumulate else "") + (f" conc{d.concurrent}" if d.concurrent else "") + (" wire" if d.dw_wire else "")


def wire_gate(ref, eg):
    """Gate of a gradient stored in the bf16 wire format: the audit's gate of any stored 16-bit value."""
    return K_ULP * ulp(ref, L.BF16) + eg


def check_wgrad(call):
    """gan_conv_wgrad against the fp64 wgrad_ref of the operands it read, in each of its three forms:
      - plain: dw (+= with accumulate) within the fp32 gate;
      - GanAdamFuse: dw untouched, m / v / master against fp64 Adam of the reference gradient, the NK copies bit-equal to the cast
        master;
      - dw_wire (data-parallel step, Pix2PixStep._capture_bucketed): the launch's last kernel writes the gradient as bf16 at this
        kernel's offset of the exchange's wire buffer.  Same reference, the gate of a stored 16-bit value (wire_gate); dw must keep
        its bits, and so must every element of the wire buffers outside [offset, offset + 16 * big_c * small_c) - the whole
        buffers are compared on the device (WireAudit), which covers the neighbouring kernels and the ALIGN padding on both
        sides.  A launch without dw_wire in a data-parallel capture must leave the wire buffers alone altogether."""
    d = call.args[0]._obj
    dt = d.dtype
    af = L.GanAdamFuse.from_address(d.adam_fuse) if d.adam_fuse else None
    call.plan = wgrad_plan(d)
    wa = _WIRE
    if d.dw_wire and wa is None:
        raise AssertionError("a dw_wire launch needs the wire buffers it writes into: replay(..., wire=WireAudit(...))")
    big, small = View(d.big, dt).dense(), View(d.small, dt).dense()
    n = 16 * d.big_c * d.small_c
    dw0 = read(d.dw, n)
    if af is not None:
        p0, m0, v0 = read(af.master, n).double(), read(af.m, n).double(), read(af.v, n).double()
    if wa is not None:
        wi, woff = wa.owner(d.dw_wire) if d.dw_wire else (None, 0)
        w0 = wa.snapshot()
    yield
    res = {}
    g = wgrad_ref(big, small, d.stride, d.big_c, d.small_c).reshape(-1)
    eg = wgrad_acc_bound(big, small, d.big_c, d.small_c)
    dw1 = read(d.dw, n)
    if wa is not None:
        res.update(wa.written(w0, wi, woff, woff + n if d.dw_wire else woff))
    if d.dw_wire:
        res['dw untouched'] = 0.0 if torch.equal(dw0.view(torch.int32), dw1.view(torch.int32)) else math.inf
        got = read(d.dw_wire, n, L.BF16)
        res['wire'] = ratio(got, g, wire_gate(g, eg))
        res['wire rounding bias'] = rounding_bias(got, g)
        return res
    if af is None:
        acc = float(d.accumulate)
        ref = g + acc * dw0.double()
        res['dw acc' if d.accumulate else 'dw'] = ratio(dw1, ref, eg + ACC * acc * dw0.double().abs() + ulp(ref, L.F32))
        return res
    res['dw untouched'] = 0.0 if torch.equal(dw0.view(torch.int32), dw1.view(torch.int32)) else math.inf
    b1, b2 = af.beta1, af.beta2
    m1, v1 = read(af.m, n).double(), read(af.v, n).double()
    p1 = read(af.master, n).double()
    mr = m0 + (g - m0) * (1 - b1)
    vr = v0 + (g * g - v0) * (1 - b2)
    res['adam m'] = ratio(m1, mr, (1 - b1) * eg + 4 * EPS32 * (m0.abs() + g.abs()))
    res['adam v'] = ratio(v1, vr, (1 - b2) * (2 * g.abs() * eg + eg * eg) + 4 * EPS32 * (v0.abs() + g * g))
    lr_t = float(read(af.lr_t, 1)[0])
    step = lr_t * m1 / (torch.sqrt(v1) + af.eps)                       # TF-form Adam on the kernel's own new moments
    pr = p0 - step
    res['adam master'] = ratio(p1, pr, ulp(pr, L.F32) + 4 * EPS32 * step.abs())
    p1f = read(af.master, n).reshape(16, d.big_c, d.small_c)
    tdt = TDT[dt]
    if af.nk_native:
        sp = (d.small_c + 7) // 8 * 8
        nat = read(af.nk_native, 16 * d.big_c * sp, dt).reshape(16, d.big_c, sp)[..., :d.small_c]
        res['nk_native = cast(master)'] = 0.0 if torch.equal(nat, p1f.to(tdt)) else math.inf
    if af.nk_transposed:
        bp = (d.big_c + 7) // 8 * 8
        tr = read(af.nk_transposed, 16 * d.small_c * bp, dt).reshape(16, d.small_c, bp)[..., :d.big_c]
        res['nk_transposed = cast(master)'] = 0.0 if torch.equal(tr, p1f.transpose(1, 2).to(tdt)) else math.inf
    return res


def check_norm_stats(call):
    """gan_norm_stats / gan_norm_stats_finalize(chunks: the conv epilogue's partials): mean, rstd, moving averages against the
    statistics of the STORED y."""
    d = call.args[0]._obj
    dt, G, C_ = d.dtype, d.groups, d.y.c
    fin = call.name == 'gan_norm_stats_finalize'
    call.plan = f"groups {G}" + (f" chunks {call.args[1]}" if fin else "")
    y = View(d.y, dt).dense()
    mm0 = read(d.moving_mean, C_).double() if d.moving_mean else None
    mv0 = read(d.moving_var, C_).double() if d.moving_var else None
    yield
    m, var, dm, dvar, R = stats_gate(y, torch.zeros_like(y), G)     # (a conv epilogue's partials are sums of the stored y too)
    rs, drs = rstd_of(var, dvar, d.eps)
    res = {'mean': ratio(read(d.mean, G * C_).double().reshape(G, C_), m, dm + 4 * EPS32 * m.abs()),
           'rstd': ratio(read(d.rstd, G * C_).double().reshape(G, C_), rs, drs)}
    if mm0 is not None:
        k = 1.0 - d.momentum
        adj = R / max(R - 1, 1)
        emm, emv = torch.zeros_like(mm0), torch.zeros_like(mv0)
        for g in range(G):
            mm0 = mm0 + (m[g] - mm0) * k
            mv0 = mv0 + (var[g] * adj - mv0) * k
            emm = emm * d.momentum + k * dm[g] + 4 * EPS32 * (mm0.abs() + m[g].abs())
            emv = emv * d.momentum + k * dvar[g] * adj + 4 * EPS32 * (mv0.abs() + var[g].abs() * adj)
        res['moving_mean'] = ratio(read(d.moving_mean, C_).double(), mm0, emm)
        res['moving_var'] = ratio(read(d.moving_var, C_).double(), mv0, emv)
    return res


def check_norm_act_fwd(call):
    d = call.args[0]._obj
    dt, G, C_ = d.dtype, d.groups, d.y.c
    call.plan = f"groups {G} act {d.act}" + (" dropout" if d.dropmask else "")
    y = View(d.y, dt).dense()
    mean = read(d.mean, G * C_).double().reshape(G, C_)
    rstd = read(d.rstd, G * C_).double().reshape(G, C_)
    gam, bet = read(d.gamma, C_).double(), read(d.beta, C_).double()
    mask = _mask(d.dropmask, d.y.n, d.y.h, d.y.w, C_, C_) if d.dropmask else None
    a0 = View(d.a, dt)
    yield
    a1 = View(d.a, dt)
    xh = (grp(y, G) - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    z = xh * gam + bet
    m2 = 2.0 * grp(mask, G) if mask is not None else torch.ones_like(z)
    out = act_f(z * m2, d.act, d.slope)
    ez = 4 * EPS32 * ((xh * gam).abs() + bet.abs()) * m2
    return {'a': ratio(grp(a1.dense(), G), out, K_ULP * ulp(out, dt) + ez), 'a untouched outside c': untouched(a0, a1, 0, d.a.c)}


def check_norm_act_bwd(call):
    """gan_norm_act_bwd (dz from da, da2, mask, act) and gan_norm_act_bwd_fused (da holds the stored dz, the workspace the
    producing dgrad's partials): dy, dgamma, dbeta."""
    d = call.args[0]._obj
    dt, G, C_ = d.dtype, d.groups, d.y.c
    fused = call.name == 'gan_norm_act_bwd_fused'
    call.plan = f"groups {G}" + (f" fused chunks {call.args[1]}" if fused else f" act {d.act}" + (" dropout" if d.dropmask else ""))
    y = View(d.y, dt).dense()
    da = View(d.da, dt).dense()
    da2 = View(d.da2, dt).dense() if d.da2.ptr else None
    mean = read(d.mean, G * C_).double().reshape(G, C_)
    rstd = read(d.rstd, G * C_).double().reshape(G, C_)
    gam, bet = read(d.gamma, C_).double(), read(d.beta, C_).double()
    mask = _mask(d.dropmask, d.y.n, d.y.h, d.y.w, C_, C_) if (d.dropmask and not fused) else None
    dg0 = read(d.dgamma, C_).double() if d.dgamma else None
    db0 = read(d.dbeta, C_).double() if d.dbeta else None
    dy0 = View(d.dy, dt)
    yield
    res = {}
    xh = (grp(y, G) - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    if fused:
        dz = grp(da, G)
        edz = 0.5 * ulp(dz, dt)                  # the producer's partials summed dz before its rounding to storage
        dzs = dz                                 # the apply pass reads the stored dz
    else:
        g_ = da + da2 if da2 is not None else da
        z = xh * gam + bet
        zb = 8 * EPS32 * ((xh * gam).abs() + bet.abs()) + 1e-30
        m2 = 2.0 * grp(mask, G) if mask is not None else torch.ones_like(z)
        lo, hi = kink_d(z * m2, zb * m2, d.act, d.slope)
        dz = grp(g_, G) * lo * m2
        edz = (grp(g_, G) * (hi - lo) * m2).abs() + 4 * EPS32 * dz.abs()
        dzs = dz
    s1 = dz.mean(1, keepdim=True)
    s2 = (dz * xh).mean(1, keepdim=True)
    e1 = edz.mean(1, keepdim=True) + ACC * dz.abs().mean(1, keepdim=True)
    e2 = (edz * xh.abs()).mean(1, keepdim=True) + ACC * (dz * xh).abs().mean(1, keepdim=True)
    gr = (gam * rstd).unsqueeze(1)
    ref = gr * (dzs - s1 - xh * s2)
    gate = K_ULP * ulp(ref, dt) + gr.abs() * ((0 if fused else edz) + e1 + xh.abs() * e2) + \
        4 * EPS32 * gr.abs() * (dzs.abs() + s1.abs() + (xh * s2).abs())
    dy1 = View(d.dy, dt)
    res['dy'] = ratio(grp(dy1.dense(), G), ref, gate)
    res['dy untouched outside c'] = untouched(dy0, dy1, 0, d.dy.c)
    if dg0 is not None:
        acc = float(d.accumulate)
        rg_ = (dz * xh).sum((0, 1)) + acc * dg0
        rb_ = dz.sum((0, 1)) + acc * db0
        res['dgamma'] = ratio(read(d.dgamma, C_).double(), rg_, (edz * xh.abs()).sum((0, 1)) + ACC * ((dz * xh).abs().sum((0, 1)) + acc * dg0.abs()))
        res['dbeta'] = ratio(read(d.dbeta, C_).double(), rb_, edz.sum((0, 1)) + ACC * (dz.abs().sum((0, 1)) + acc * db0.abs()))
    return res


def check_act_bwd(call):
    d = call.args[0]._obj
    dt, C_ = d.dtype, d.dy.c
    call.plan = f"act {d.act}" + (" dbias" if d.dbias else "")
    a = View(d.a, dt).dense()
    g_ = View(d.da, dt).dense()
    if d.da2.ptr:
        g_ = g_ + View(d.da2, dt).dense()
    db0 = read(d.dbias, C_).double() if d.dbias else None
    dy0 = View(d.dy, dt)
    yield
    lo, hi = kink_d(a, torch.zeros_like(a), d.act, d.slope)       # act'(a): a == 0 takes either side
    rlo, rhi = torch.minimum(g_ * lo, g_ * hi), torch.maximum(g_ * lo, g_ * hi)
    dy1 = View(d.dy, dt)
    got = dy1.dense()
    res = {'dy': between(got, rlo, rhi, K_ULP * ulp(rhi, dt) + 4 * EPS32 * rhi.abs()),
           'dy untouched outside c': untouched(dy0, dy1, 0, C_)}
    if db0 is not None:
        acc = float(d.accumulate)
        s = got.sum((0, 1, 2)) + acc * db0
        res['dbias'] = ratio(read(d.dbias, C_).double(), s, ACC * (got.abs().sum((0, 1, 2)) + acc * db0.abs()))
    return res


def check_bias_grad(call):
    dt, dyp, dbias, acc = call.args[0], call.args[1]._obj, call.args[2], call.args[3]
    call.plan = "acc" if acc else ""
    dy = View(dyp, dt).dense()
    db0 = read(dbias, dyp.c).double()
    yield
    s = dy.sum((0, 1, 2)) + acc * db0
    return {'dbias': ratio(read(dbias, dyp.c).double(), s, ACC * (dy.abs().sum((0, 1, 2)) + acc * db0.abs()))}


def fold_ref(master, gamma, beta, mean, var, eps, transposed, tdt):
    """gan_bn_fold_multi of one entry in float32, one IEEE operation at a time (the kernel's contraction is off): master [16, A, B]
    -> (bias [co], nk [16, co, pad8(ci)] of the storage type; padding columns zero).  transposed: a Conv2D kernel (HWIO: A = Cin,
    B = Cout), else a Conv2DTranspose kernel (A = Cout, B = Cin)."""
    # numpy float32 scalars-and-arrays arithmetic: every operation is one correctly rounded IEEE operation, none fused
    master, gamma, beta, mean, var = (t.to(torch.float32).numpy() for t in (master, gamma, beta, mean, var))
    s = gamma * (np.float32(1.0) / np.sqrt(var + np.float32(eps)))
    bias = torch.from_numpy((beta - mean * s).astype(np.float32))
    w = np.transpose(master, (0, 2, 1)) if transposed else master          # -> [tap][co][ci]
    co, ci = w.shape[1], w.shape[2]
    nk = torch.zeros((16, co, (ci + 7) // 8 * 8), dtype=tdt)
    nk[..., :ci] = torch.from_numpy((w * s[None, :, None]).astype(np.float32)).to(tdt)
    return bias, nk


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def bit_equal(got, ref):
    """Gate entry of a value that must come out bit for bit: 0 or inf."""
    return 0.0 if got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(_bits(got), _bits(ref)) else math.inf


def check_fold(call):
    """gan_bn_fold_multi: the device table of GanFoldEntry decoded; bias and folded NK copy of every entry BIT-EQUAL to fold_ref of
    the snapshot; the entry's inputs, and the tensors label_calls named (Call.guards: master, nat, tr, moving statistics), unchanged."""
    table, n, tiles, dt, eps = call.args[:5]
    call.plan = f"{n} entries, {tiles} tiles"
    size = C.sizeof(L.GanFoldEntry)
    raw = read(table, n * size, tdtype=torch.uint8).numpy().tobytes()
    ents = [L.GanFoldEntry.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(n)]
    pre = []
    for e in ents:
        co = e.B if e.transposed else e.A
        pre.append([read(e.master, 16 * e.A * e.B)] + [read(p, co) for p in (e.gamma, e.beta, e.moving_mean, e.moving_var)])
    guards = getattr(call, 'guards', [])
    g0 = [_bits(t).clone() for t in guards]
    yield
    res = {'bias': 0.0, 'nk': 0.0, 'inputs unchanged': 0.0}
    for e, p0 in zip(ents, pre):
        co, ci = (e.B, e.A) if e.transposed else (e.A, e.B)
        p1 = [read(e.master, 16 * e.A * e.B)] + [read(p, co) for p in (e.gamma, e.beta, e.moving_mean, e.moving_var)]
        res['inputs unchanged'] = max([res['inputs unchanged']] + [bit_equal(a, b) for a, b in zip(p1, p0)])
        bias, nk = fold_ref(p0[0].reshape(16, e.A, e.B), p0[1], p0[2], p0[3], p0[4], eps, e.transposed, TDT[dt])
        res['bias'] = max(res['bias'], bit_equal(read(e.bias, co), bias))
        res['nk'] = max(res['nk'], bit_equal(read(e.nk, nk.numel(), dt), nk.reshape(-1)))
    if guards:
        res['master / nat / tr / state unchanged'] = 0.0 if all(torch.equal(_bits(t), b) for t, b in zip(guards, g0)) else math.inf
    return res


CHECKERS = dict({k: check_conv for k in OPS}, gan_bn_fold_multi=check_fold, gan_conv_wgrad=check_wgrad, gan_norm_stats=check_norm_stats,
                gan_norm_stats_finalize=check_norm_stats, gan_norm_act_fwd=check_norm_act_fwd, gan_norm_act_bwd=check_norm_act_bwd,
                gan_norm_act_bwd_fused=check_norm_act_bwd, gan_act_bwd=check_act_bwd, gan_bias_grad=check_bias_grad)


def plan_of(call):
    """The plan string a checker gives `call`, from the descriptor and the host-side planner queries alone: nothing is read from the
    device and nothing is issued (replay asserts that every checker agrees with it).  '' for entry points without a checker."""
    n, a = call.name, call.args
    if n in OPS:
        d, op = a[0]._obj, OPS[n]
        info, ts = conv_plan(d, op)
        full = info[4] == -1 and bool(d.norm_fuse)
        return f"op{op} tile {info[0]}x{info[1]} split {info[2]} par {info[3]} stats {info[4]} ts {ts}" + \
            (" bwd_fuse" if d.bwd_fuse else "") + (" norm_fuse" if full else "")
    if n == 'gan_conv_wgrad':
        return wgrad_plan(a[0]._obj)
    if n in ('gan_norm_stats', 'gan_norm_stats_finalize'):
        return f"groups {a[0]._obj.groups}" + (f" chunks {a[1]}" if n == 'gan_norm_stats_finalize' else "")
    if n == 'gan_norm_act_fwd':
        d = a[0]._obj
        return f"groups {d.groups} act {d.act}" + (" dropout" if d.dropmask else "")
    if n in ('gan_norm_act_bwd', 'gan_norm_act_bwd_fused'):
        d = a[0]._obj
        return f"groups {d.groups}" + (f" fused chunks {a[1]}" if n == 'gan_norm_act_bwd_fused' else
                                       f" act {d.act}" + (" dropout" if d.dropmask else ""))
    if n == 'gan_act_bwd':
        d = a[0]._obj
        return f"act {d.act}" + (" dbias" if d.dbias else "")
    if n == 'gan_bias_grad':
        return "acc" if a[3] else ""
    if n == 'gan_bn_fold_multi':
        return f"{a[1]} entries, {a[2]} tiles"
    if n in OPTION_PLANS:
        return OPTION_PLANS[n](call)
    return ''


# ---- plan classes, thin operands, required calls, padding channels (the RGB audit) -------------------------------------------------
THIN_C = 8                   # an operand of at most this many channels: one 16-byte pixel (thin.hip, the tap-folded wgrad forms)


def conv_class(d, op, requested=None):
    """Plan class of a convolution descriptor as tests/test_cpu_launch_audit.py::plan_classes keys it: (op, tile, split or not,
    parity form, statistics, tap sharing), and for the streaming kernels (tile rows 0) the sub-form - 'two-launch' (Z through the
    workspace: conv_thin_n_kernel + conv_thin_col2im_kernel) or 'one-kernel' - from gan_conv_workspace_bytes.
    requested: whether statistics groups were asked for (the host tables know; default: what the descriptor holds)."""
    info, ts = conv_plan(d, op)
    asked = bool(d.stats_groups) if requested is None else bool(requested)
    st = ('full' if info[4] == -1 else 'stats' if info[4] > 0 else 'none') if asked else '-'
    key = ('conv', op, info[0], info[1], info[2] > 1, info[3], st, ts)
    if info[0] == 0:
        key += ('two-launch' if L.load().gan_conv_workspace_bytes(C.byref(d), op) > 0 else 'one-kernel',)
    return key


def wgrad_class(d, wire=0):
    info = (C.c_int32 * 4)()
    L.check(L.load().gan_wgrad_plan_info(C.byref(d), info), "wgrad_plan_info")
    return ('wgrad', info[0], info[1], info[2] > 1, info[3], int(wire))


def same_class(key):
    """A class key with a statistics request that was not honoured ('none') folded onto no request ('-'): nets._Builder drops such a
    request from the descriptor it records, the host tables keep it."""
    return tuple('-' if k == 'none' else k for k in key)


def call_class(call):
    """same_class() of a recorded conv / wgrad call (None for every other entry point)."""
    if call.name in OPS:
        return same_class(conv_class(call.args[0]._obj, OPS[call.name]))
    if call.name == 'gan_conv_wgrad':
        d = call.args[0]._obj
        return wgrad_class(d, bool(d.dw_wire))
    return None


def outside_classes(audited):
    """Predicate of replay(check=...): a recorded conv / wgrad call whose plan class (call_class) is not in `audited` - the calls
    a class audit of tests/test_gpu_wide_audit.py checks.  Every other entry point is issued unchecked."""
    def check(call):
        k = call_class(call)
        return k is not None and k not in audited
    return check


def missing_classes(calls, rows, required):
    """required: {class: tag of a launch the host table files under it}.  The classes no CHECKED row holds (in the manner of
    missing_required), each with what the case recorded of it."""
    held = {}
    for c, r in zip(calls, rows):
        k = call_class(c)
        if k is not None:
            held.setdefault(k, []).append(r[4] is not None)
    return [f"{tag} {k}: " + (f"{len(held[k])} call(s) recorded, none checked" if k in held else "no call of this class recorded")
            for k, tag in required.items() if not any(held.get(k, ()))]


def thin_call(call):
    """Does the call have an operand of <= THIN_C channels?  These are the calls whose code path depends on the image's channel
    count: conv ops by x.c, y.c or w_rows, wgrad by big_c or small_c, gan_bias_grad / gan_act_bwd by the tensor they reduce / write."""
    n, a = call.name, call.args
    if n in OPS:
        d = a[0]._obj
        return d.x.c <= THIN_C or d.y.c <= THIN_C or d.w_rows <= THIN_C
    if n == 'gan_conv_wgrad':
        d = a[0]._obj
        return d.big_c <= THIN_C or d.small_c <= THIN_C
    if n == 'gan_bias_grad':
        return a[1]._obj.c <= THIN_C
    if n == 'gan_act_bwd':
        return a[0]._obj.dy.c <= THIN_C
    return False


def missing_required(calls, rows, required):
    """required: [(title, entry point, substring of the label, least number of distinct checked calls)].  A call counts when its
    row was checked (res not None); distinct = different input tensors (x / big / dy pointer), so the two invocations of D count
    twice and a repeated issue of one call once.  Returns the titles not met, with what was found."""
    bad = []
    for title, entry, frag, least in required:
        seen = set()
        for c, r in zip(calls, rows):
            if c.name == entry and frag in c.label and r[4] is not None:
                o = getattr(c.args[0], '_obj', None)
                if isinstance(o, L.GanConvDesc):
                    seen.add((o.x.ptr, o.y.ptr))
                elif isinstance(o, L.GanWgradDesc):
                    seen.add((o.big.ptr, o.small.ptr))
                else:
                    seen.add(id(c))
        if len(seen) < least:
            bad.append(f"{title}: {len(seen)} checked {entry} call(s) labelled '{frag}', {least} required")
    return bad


def pad_channels(named):
    """named: [(name, NHWC device tensor of 8-channel pixels, real channels)] -> the names whose padding channels [real, 8) hold a
    bit that is not zero (-0.0 included): thin-K reads whole 16-byte pixels, so such an element reaches the next layer."""
    bad = []
    for name, t, real in named:
        assert t.shape[-1] == 8 and 0 < real <= 8, (name, tuple(t.shape), real)
        pad = _bits(t[..., real:])
        k = int((pad != 0).sum())
        if k:
            bad.append(f"{name}: {k} non-zero elements in channels [{real}, 8)")
    return bad


# ---- data-parallel step: an exchange that does nothing, the wire buffers, the update of whole networks ---------------------------
SENTINEL = 0x7FA5            # a bf16 NaN no kernel produces: what the wire buffers hold before the compute calls
_WIRE = None                 # the WireAudit of the replay in progress (replay(wire=...))


def identity_sync(step, compress):
    """A GradSync of world 2 for ONE process: pack / unpack are the real kernels, the exchange is the identity (start returns no
    handle, wait does nothing; no process group, no child process, no RCCL).  The "sum over ranks" is this rank's own wire
    contents (own fp32 gradients for compress = False), so the 1/world of the mean is real and visible: every update is half the
    one-GPU update."""
    from gan_amd.ddp import GradSync

    class IdentitySync(GradSync):
        def start(self, i, lo=0, hi=None):
            return None

        def wait(self, handle):
            pass

    s = IdentitySync([n.params.grad for n in step.nets()], compress_bf16=compress, lib=step.ctx.lib)
    s.world, s.active = 2, True
    return s


class WireAudit:
    """The bf16 wire buffers of a data-parallel capture (GradSync.wire, one per network, ParamSet offsets), compared whole and on
    the device around every call that may write them: which elements changed, that none of them lies outside the call's range,
    and that no element changes twice.  fill() plants SENTINEL; coverage() after the last compute call: every element of every
    kernel's and vector's real extent written exactly once, no SENTINEL left inside one."""

    def __init__(self, step, sync):
        self.bufs = [w.view(torch.int16) for w in sync.wire]
        self.sets = [n.params for n in step.nets()]
        self.count = [torch.zeros(b.numel(), dtype=torch.int8, device=b.device) for b in self.bufs]
        self.log = []            # (buffer, lo, hi) of every range a call claimed

    def fill(self):
        for b, c in zip(self.bufs, self.count):
            b.fill_(SENTINEL)
            c.zero_()
        self.log.clear()
        if self.bufs[0].is_cuda:
            torch.cuda.synchronize()

    def owner(self, ptr):
        for i, b in enumerate(self.bufs):
            if b.data_ptr() <= ptr < b.data_ptr() + 2 * b.numel():
                return i, (ptr - b.data_ptr()) // 2
        raise AssertionError(f"wire pointer {ptr:#x} lies in no wire buffer")

    def snapshot(self):
        return [b.clone() for b in self.bufs]

    def written(self, before, i, lo, hi):
        """Gate entries of one call that claimed elements [lo, hi) of buffer i (i None: nothing)."""
        res = {'wire untouched outside its range': 0.0, 'no wire element written twice': 0.0}
        for k, (b0, b1) in enumerate(zip(before, self.bufs)):
            ch = b0 != b1
            if k == i:
                self.log.append((i, lo, hi))
                self.count[k] += ch.to(torch.int8)
                if bool((self.count[k][lo:hi] > 1).any()):
                    res['no wire element written twice'] = math.inf
                ch[lo:hi] = False
            if bool(ch.any()):
                res['wire untouched outside its range'] = math.inf
        return res

    def coverage(self):
        """Failures (strings) of the exactly-once rule over the real extents."""
        bad = []
        for i, (P, b, c) in enumerate(zip(self.sets, self.bufs, self.count)):
            for name, (o, shape) in P.entries.items():
                n = int(np.prod(shape))
                cnt, left = c[o:o + n], int((b[o:o + n] == SENTINEL).sum())
                if left or bool((cnt != 1).any()):
                    bad.append(f"wire {i} {name} [{o}, {o + n}): {int((cnt == 0).sum())} elements never written, "
                               f"{int((cnt > 1).sum())} written twice, {left} still hold the sentinel")
            if bool((c > 1).any()):
                bad.append(f"wire {i}: {int((c > 1).sum())} elements (padding included) written by more than one call")
        return bad


def check_pack_range(call):
    """gan_grad_pack in a data-parallel capture: its range is recorded (WireAudit), nothing outside it may change, and - it costs
    nothing here - the range must equal torch's round-to-nearest-even cast of the fp32 gradients it read."""
    src, dst, n = call.args[:3]
    wa = _WIRE
    i, lo = wa.owner(dst)
    call.plan = f"wire {i} [{lo}, {lo + n})"
    g = wa.sets[i].grad
    assert src == g.data_ptr() + 4 * lo, "gan_grad_pack reads another range than it writes"
    w0 = wa.snapshot()
    yield
    res = wa.written(w0, i, lo, lo + n)
    res['wire = rne(grad)'] = 0.0 if torch.equal(wa.bufs[i][lo:lo + n], g[lo:lo + n].to(torch.bfloat16).view(torch.int16)) else math.inf
    return res


def adam_end_ratios(p0, m0, v0, g, gs, lr_t, p1, m1, v1, b1=0.5, b2=0.999):
    """{item: error / gate} of one Adam step over flat tensors (any device): m and v against fp64 of the stored inputs (g: the stored
    gradient widened to fp32, gs: what the kernel multiplies it by), master against fp64 of the NEW moments the kernel stored, all
    within tests/elementwise_ref.adam_gates."""
    from tests import elementwise_ref as E
    omb1, omb2, eps = (float(c) for c in E.adam_consts(b1, b2))
    p0, m0, v0, g, p1, m1, v1 = (t.double() for t in (p0, m0, v0, g, p1, m1, v1))
    gr = g * gs
    mr, vr = m0 + (gr - m0) * omb1, v0 + (gr * gr - v0) * omb2
    u = m1 * lr_t / (torch.sqrt(v1) + eps)
    pr = p0 - u
    gm, gv, gp = E.adam_gates(m0, v0, g, gs, pr, u)
    return {'adam m': ratio(m1, mr, gm), 'adam v': ratio(v1, vr, gv), 'adam master': ratio(p1, pr, gp)}


def rounding_bias(got, ref, dt=L.BF16):
    """|mean over the elements of sign(ref) * (got - ref) / ulp(ref)| / 0.05.  Round-to-nearest-even leaves an error uniform in +-half
    an ulp: over the n >= 65,536 elements of the smallest kernel a launch writes in the wire format its mean has a standard deviation
    of 0.29 / sqrt(n) <= 0.0012 ulp (the fp32 accumulation error is symmetric too), so 0.05 is forty of them; truncation leaves -0.5.
    The per-element gate (one ulp) cannot tell the two apart."""
    ref = ref.double()
    e = torch.sign(ref) * (got.double() - ref) / ulp(ref, dt)
    nz = ref != 0
    if not bool(torch.isfinite(e).all()):
        return math.inf
    return abs(float(e[nz].mean())) / 0.05 if bool(nz.any()) else 0.0


def wgrad_acc_bound(big, small, big_c, small_c):
    """fp32 accumulation bound of every element of a kernel gradient: ACC * sum|terms|, sum|terms| <= max|big| * sum over positions of
    |small| per small channel (the cheap bound: an exact |big| x |small| pass would double the reference's cost)."""
    sb = float(big[..., :big_c].abs().max()) * small[..., :small_c].abs().sum((0, 1, 2))
    return ACC * sb.expand(16, big_c, small_c).reshape(-1)


class AdamEnd:
    """The update of every network as a whole, after the Adam graphs' calls of a data-parallel step.
    snapshot() before the first of them: master, m, v and the gradient source - the bf16 wire buffer (g = wire / world), the fp32
    gradient buffer (fp32 wire: g = grad * grad_scale) or, on fp16, nothing yet: there g is the buffer gan_grad_unpack leaves, which
    must be bit-equal to wire * 1/world.  check(): m, v, master of every parameter element against fp64 on the device (torch
    float64) within tests/elementwise_ref.adam_gates - u and p from the stored new moments, as the fused-Adam check does - step == 1,
    the gradient source untouched, every NK copy bit-equal to the cast master with zero padding, the kernels' ALIGN padding of
    master / m / v untouched; fp16: loss scale unchanged and the step taken."""

    def __init__(self, step, sync, b1=0.5, b2=0.999):
        self.step, self.sync, self.b1, self.b2 = step, sync, b1, b2
        self.mode = 'wire' if step._wire_adam() else ('unpack' if sync.compress else 'fp32')

    def snapshot(self):
        ctx = self.step.ctx
        self.pre = []
        for i, net in enumerate(self.step.nets()):
            P = net.params
            src = self.sync.wire[i] if self.mode != 'fp32' else P.grad
            self.pre.append((P.master.clone(), P.m.clone(), P.v.clone(), src.clone()))
        self.ls0 = ctx.ls.clone() if ctx.ls is not None else None
        torch.cuda.synchronize()

    def check(self):
        ctx, world = self.step.ctx, self.sync.world
        rows = []
        for i, (net, (p0, m0, v0, src0)) in enumerate(zip(self.step.nets(), self.pre)):
            P = net.params
            res = {}
            src1 = self.sync.wire[i] if self.mode != 'fp32' else P.grad
            if self.mode == 'wire':
                g, gs = src0.float(), 1.0 / world
                res['wire untouched by Adam'] = 0.0 if torch.equal(src0.view(torch.int16), src1.view(torch.int16)) else math.inf
            elif self.mode == 'fp32':
                g, gs = src0, self.sync.grad_scale
                assert gs == 1.0 / world
                res['grad untouched by Adam'] = 0.0 if torch.equal(src0.view(torch.int32), src1.view(torch.int32)) else math.inf
            else:
                g, gs = P.grad.clone(), self.sync.grad_scale * float(self.ls0[1])
                res['unpacked grad = wire * 1/world'] = 0.0 if torch.equal(g.view(torch.int32), (src0.float() * (1.0 / world)).view(torch.int32)) else math.inf
                res['gradient finite'] = 0.0 if bool(torch.isfinite(g).all()) else math.inf
            real = torch.zeros(P.total, dtype=torch.bool, device=p0.device)
            for name, (o, shape) in P.entries.items():
                real[o:o + int(np.prod(shape))] = True
            pad = ~real
            pad[P.vec_start:] = False               # (gan_adam_tf runs over the vectors' padding too: harmless, not gated)
            res['kernel padding of master / m / v untouched'] = 0.0 if all(
                torch.equal(a[pad].view(torch.int32), b[pad].view(torch.int32)) for a, b in ((p0, P.master), (m0, P.m), (v0, P.v))) else math.inf
            res.update(adam_end_ratios(*(t[real] for t in (p0, m0, v0, g)), gs, float(P.lr_t[0]),
                                       *(t[real] for t in (P.master, P.m, P.v)), self.b1, self.b2))
            p1, p0 = P.master[real], p0[real]
            res['step == 1'] = 0.0 if int(P.step[0]) == 1 else math.inf
            nk = 0.0
            for name in P.nat:
                o, shape = P.entries[name]
                A_, B_ = shape[2], shape[3]
                w = P.master[o:o + 16 * A_ * B_].view(16, A_, B_)
                for t, ref, c in ((P.nat[name], w, B_), (P.tr[name], w.transpose(1, 2), A_)):
                    if not torch.equal(_bits(t[..., :c]), _bits(ref.to(t.dtype))) or bool(t[..., c:].any()):
                        nk = math.inf
            res['nat / tr = cast(master), padding zero'] = nk
            if self.ls0 is not None:
                res['loss scale unchanged, step taken'] = 0.0 if (float(ctx.ls[0]) == float(self.ls0[0]) and float(ctx.ls[3]) == 0.0
                                                                  and not torch.equal(p1, p0)) else math.inf
            tag = _nets_of(self.step)[i][0]
            rows.append((f"{tag} whole network ({int(real.sum())} parameters)", 'gan_adam (whole network)', f"{self.mode} g, scale {gs:g}", '', res))
        return rows


def _short(sym):
    m = re.match(r'_Z(?:N\d*)?(\d+)', sym)
    if not m:
        return sym
    n = int(m.group(1))
    return sym[m.end():m.end() + n]


# ---- the option entry points: dSSIM, MS-SSIM, Sobel edge term, DiffAugment, least-squares GAN loss, image pools, learning-rate schedule ------
# Each checker is a thin generator (decode the descriptor / argument list the product code built, read the operands through their
# GanTensor views, yield, read back) around a device-free *_ratios function: (snapshot, descriptor fields, outputs) -> {item: error /
# gate}.  tests/test_cpu_option_audit.py puts the references' own results and planted faults through the same functions.
# No gate is new.  Where a stand-alone gate presumes inputs the step does not give it, the derivation stands next to the gate.
DTN = {L.F32: 'f32', L.BF16: 'bf16', L.F16: 'f16'}
OPTION_ENTRIES = ('gan_dssim', 'gan_msssim', 'gan_edge_l1', 'gan_diffaug_draw', 'gan_diffaug_apply', 'gan_lsq_logits', 'gan_patchgan_losses_lsq',
                  'gan_pool_exchange', 'gan_adam_begin_sched')
EDGE_MARGIN = 1e-5                   # tests/test_gpu_edge.py::general_pair: no contributing Sobel response within this of the kink of |.|
EDGE_SHARE = 0.01                    # ... ::test_general_cases: at most this share of the elements may be excluded (on the reference alone)
EDGE_LOSS_REL = 2048 * 2.0 ** -24    # ... the bound of an fp32 tile partial of non-negative terms, relative to the term
DSSIM_KIND = 'noise'                 # tests/test_gpu_quality.py::SSIM_GATE: an untrained generator's output against a lattice-noise target


def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def _void(p):
    """A ctypes pointer argument / field as an integer address (0 for NULL)."""
    return int(getattr(p, 'value', p) or 0)


def tensor_key(t):
    return (_void(t.ptr), t.n, t.h, t.w, t.c, t.pitch)


class Pixels:
    """Snapshot of the WHOLE pixels a GanTensor view lies in: raw [n, h, w, pitch] of the storage type, and the view's channel offset
    c0 inside a pixel, taken from the pointer (the step's image-side buffers are pitch-aligned allocations whose samples are whole
    pixels apart) - so that the channels beside the view, on both sides, are compared too."""

    def __init__(self, t, dt):
        es = TDT[dt].itemsize
        self.t, self.dt, self.c = t, dt, t.c
        self.c0 = (_void(t.ptr) // es) % t.pitch
        assert self.c0 + t.c <= t.pitch, ("a view that is not inside one pitch-aligned pixel", tensor_key(t))
        self.raw = read(_void(t.ptr) - self.c0 * es, t.n * t.h * t.w * t.pitch, dt).reshape(t.n, t.h, t.w, t.pitch)

    def real(self):
        return self.raw[..., self.c0:self.c0 + self.c]


def pixels_outside(raw0, raw1, c0, c):
    """Gate entry: every stored element of the pixels outside channels [c0, c0 + c) keeps its bits (pad channels, and the channels
    of a neighbouring view)."""
    keep = torch.ones(raw0.shape[-1], dtype=torch.bool)
    keep[c0:c0 + c] = False
    return 0.0 if torch.equal(_bits(raw0[..., keep]), _bits(raw1[..., keep])) else math.inf


def _scale_word(ptr):
    return float(read(ptr, 1)[0]) if ptr else None


def dssim_ratios(a, b, da0, da1, c0, loss0, loss1, f):
    """gan_dssim.  a, b: the stored operands [n,h,w,c]; da0 / da1: whole pixels of da before / after; loss0 / loss1: loss_out before /
    after; f: loss_scale, loss_accumulate, grad_scale, ls (the loss-scale word or None), dtype_da.
    Gates of tests/test_gpu_dssim.py: the gradient max|got - want| / max|want| <= 8 * yardstick + ulp(dtype_da), the yardstick being
    the same reference in float32 against the fp64 one on these very operands; the loss within SSIM_GATE.  da = grad_scale * ls *
    dloss/da; the loss is NOT multiplied by ls.  loss_accumulate: one more fp32 addition, half an ulp32 of the sum, taken as one."""
    from tests import dssim_ref
    from tests.test_gpu_dssim import ULP as DSSIM_ULP
    from tests.test_gpu_quality import SSIM_GATE
    c = a.shape[-1]
    a64, b64 = a.double().numpy(), b.double().numpy()
    loss, g64 = dssim_ref.loss_and_grad(a64, b64)
    _, g32 = dssim_ref.loss_and_grad(a64, b64, torch.float32)
    g64 = g64.numpy()
    top = float(np.abs(g64).max())
    yard = float(np.abs(g32.double().numpy() - g64).max() / top) if top > 0 else 0.0
    k = f['grad_scale'] * (f['ls'] if f['ls'] is not None else 1.0)
    got = da1[..., c0:c0 + c].double().numpy()
    res = {}
    if not np.isfinite(got).all():
        res['da'] = math.inf
    else:
        res['da'] = E_r(float(np.abs(got - k * g64).max()) / (abs(k) * top), 8 * yard + DSSIM_ULP[DTN[f['dtype_da']]])
    acc = int(f['loss_accumulate'])
    want = f['loss_scale'] * loss + (float(loss0) if acc else 0.0)
    res['loss'] = E_r(abs(float(loss1) - want), abs(f['loss_scale']) * SSIM_GATE[DSSIM_KIND] + acc * ulp32(want))
    res['da untouched outside the view'] = pixels_outside(da0, da1, c0, c)
    return res


def E_r(err, gate):
    from tests import elementwise_ref as E
    return E._r(err, gate)


def edge_ratios(a, b, da0, da1, c0, loss0, loss1, f):
    """gan_edge_l1.  Arguments as dssim_ratios; f also holds grad_accumulate.
    Gradient: bit-equal to the header's rounding order on the reference's integer map k (tests/test_gpu_edge.py::expected_grad:
    (float(k) * F) / n [* ls], [float(da before) +], ONE rounding to storage - with grad_accumulate the snapshot of da taken before
    the call), on the elements the reference can decide: no contributing Sobel response within EDGE_MARGIN of 0.  The excluded share
    is a property of the reference alone and must stay <= EDGE_SHARE.
    Loss: loss_out (+)= (float)(sum / (2 n c M)) * loss_scale.  The term within EDGE_LOSS_REL of itself (that test's gate, which covers
    the two roundings of the quotient and the product: 2^-23 against 2^-13); loss_accumulate adds one fp32 addition: half an ulp32
    of the sum, taken as one."""
    from tests import edge_ref
    from tests.test_gpu_edge import bits, expected_grad
    c = a.shape[-1]
    a64, b64 = a.double().numpy(), b.double().numpy()
    k = edge_ref.k_map(a64, b64)
    mask = edge_ref.min_response(a64, b64) >= EDGE_MARGIN
    res = {'excluded share / 1 %': float(1.0 - mask.mean()) / EDGE_SHARE}
    old = da0[..., c0:c0 + c] if f['grad_accumulate'] else None
    want = expected_grad(k, f['grad_scale'], tuple(a.shape), DTN[f['dtype_da']], ls=f['ls'], old=old)
    m = torch.from_numpy(mask)
    got = da1[..., c0:c0 + c].contiguous()
    res['da (bits)'] = 0.0 if torch.equal(bits(got)[m], bits(want)[m]) else math.inf
    acc = int(f['loss_accumulate'])
    term = f['loss_scale'] * edge_ref.loss(a64, b64)
    want_l = term + (float(loss0) if acc else 0.0)
    res['loss'] = E_r(abs(float(loss1) - want_l), EDGE_LOSS_REL * abs(term) + acc * ulp32(want_l))
    res['da untouched outside the view'] = pixels_outside(da0, da1, c0, c)
    return res


MSSSIM_PREMISE = 0.4                 # tests/test_gpu_msssim.py: every factor CS_j, S_{M-1} at least this, the premise of its loss gate


def msssim_ratios(a, b, da0, da1, c0, loss0, loss1, f):
    """gan_msssim.  Arguments as dssim_ratios; f also holds grad_accumulate, scales and power (the descriptor's fp32 factors).
    Reference: tests/msssim_ref.loss_and_grad in float64 on the stored operands; the same function in float32 is the yardstick.
    premise: MSSSIM_PREMISE / the reference's smallest factor - a condition on the INPUTS, computed from the reference alone; under it
      |dMS| <= max_j |dCS_j| / 0.4, which is what makes the loss gate below valid (tests/test_gpu_msssim.py).  Above 1 the row fails:
      the operands are of a kind the gate is not derived for (independent images: factors at the clamp, where pow is ill-conditioned).
    da, grad_accumulate = 0: dssim_ratios' form and tests/test_gpu_msssim.py's gate, max|got - k g64| / (|k| max|g64|) <= 8 * yardstick +
      ulp(dtype_da), k = grad_scale * (the loss-scale word or 1).
    da, grad_accumulate = 1: the kernel forms the fp32 term t = k g as it does when it stores, widens da before exactly, adds in fp32
      and rounds the sum ONCE to dtype_da.  |t - k g64| is bounded by the storing form's gate taken absolutely, |k| max|g64| *
      (8 * yardstick + ulp(dtype_da)) (generous by the one storage rounding of t that this form does not make); the fp32 addition and the
      rounding to storage together stay within one storage ulp of the wanted sum float(da before) + k g64 (half an ulp for round to
      nearest, the other half for a sum that sits on the other side of a binade edge, as K_ULP; at fp32 storage the addition IS the
      rounding).  Per element: |got - wanted| <= |k| max|g64| * (8 * yardstick + ulp(dtype_da)) + ulp_storage(wanted).  No new constant.
    loss: wanted loss_scale * loss (+ loss0); gate |loss_scale| * 2.5 * SSIM_GATE (the 2.5e-5 of tests/test_gpu_msssim_step.py, valid by
      the premise row) + one ulp32 of the sum for the accumulating addition.  The loss is NOT multiplied by the loss-scale word."""
    from tests import msssim_ref
    from tests.test_gpu_dssim import ULP as DSSIM_ULP
    from tests.test_gpu_quality import SSIM_GATE
    c, M = a.shape[-1], int(f['scales'])
    power = tuple(float(p) for p in f['power'])[:M]
    a64, b64 = a.double().numpy(), b.double().numpy()
    loss, g64, _ = msssim_ref.loss_and_grad(a64, b64, M, power)
    _, g32, _ = msssim_ref.loss_and_grad(a64, b64, M, power, dtype=torch.float32)
    fmin = msssim_ref.min_factor(a64, b64, M)
    g64 = g64.numpy()
    top = float(np.abs(g64).max())
    yard = float(np.abs(g32.double().numpy() - g64).max() / top) if top > 0 else 0.0
    k = f['grad_scale'] * (f['ls'] if f['ls'] is not None else 1.0)
    dt = f['dtype_da']
    bound = 8 * yard + DSSIM_ULP[DTN[dt]]
    got = da1[..., c0:c0 + c].double().numpy()
    res = {'premise': MSSSIM_PREMISE / fmin if fmin > 0 else math.inf}
    if not np.isfinite(got).all():
        res['da'] = math.inf
    elif not f['grad_accumulate']:
        res['da'] = E_r(float(np.abs(got - k * g64).max()), abs(k) * top * bound)       # (a gradient that is 0 everywhere: 0 demanded)
    else:
        want = da0[..., c0:c0 + c].double().numpy() + k * g64
        gate = abs(k) * top * bound + ulp(torch.from_numpy(want), dt).numpy()
        res['da'] = float((np.abs(got - want) / gate).max())
    acc = int(f['loss_accumulate'])
    want = f['loss_scale'] * loss + (float(loss0) if acc else 0.0)
    res['loss'] = E_r(abs(float(loss1) - want), abs(f['loss_scale']) * 2.5 * SSIM_GATE[DSSIM_KIND] + acc * ulp32(want))
    res['da untouched outside the view'] = pixels_outside(da0, da1, c0, c)
    return res


def _loss_desc_fields(d):
    return dict(loss_scale=float(d.loss_scale), loss_accumulate=int(d.loss_accumulate), grad_scale=float(d.grad_scale),
                ls=_scale_word(d.scale_state), dtype_da=d.dtype_da, grad_accumulate=int(getattr(d, 'grad_accumulate', 0)))


def _loss_plan(call):
    d = call.args[0]._obj
    return f"{d.a.n}x{d.a.h}x{d.a.w}x{d.a.c} loss x{d.loss_scale:g}{' acc' if d.loss_accumulate else ''} grad x{d.grad_scale:g}" + \
        (' acc' if getattr(d, 'grad_accumulate', 0) else '') + (' ls' if d.scale_state else '')


def _check_image_loss(call, ratios, **more):
    """more: descriptor fields beyond _loss_desc_fields that `ratios` reads from f."""
    d = call.args[0]._obj
    call.plan = OPTION_PLANS[call.name](call)
    assert d.da.ptr, "the audit checks the gradient-carrying form (the step never calls the loss-only one)"
    a, b = Pixels(d.a, d.dtype_a).real().clone(), Pixels(d.b, d.dtype_b).real().clone()
    da0 = Pixels(d.da, d.dtype_da)
    loss0 = float(read(d.loss_out, 1)[0])
    f = dict(_loss_desc_fields(d), **more)
    yield
    da1 = Pixels(d.da, d.dtype_da)
    return ratios(a, b, da0.raw, da1.raw, da0.c0, loss0, float(read(d.loss_out, 1)[0]), f)


def check_dssim(call):
    return (yield from _check_image_loss(call, dssim_ratios))


def check_edge(call):
    return (yield from _check_image_loss(call, edge_ratios))


def check_msssim(call):
    d = call.args[0]._obj
    return (yield from _check_image_loss(call, msssim_ratios, scales=int(d.scales), power=tuple(d.power)[:d.scales]))


AUG_RECORDS = 128                    # gan_amd.diffaug.MAX_RECORDS: the table every DiffAugment object allocates


def diffaug_draw_ratios(table0, counter0, table1, counter1, f):
    """gan_diffaug_draw.  table0 / table1: int32 [records, 8] before / after; counter0 / counter1: the device launch counter;
    f: n, h, w, policy, seed, stream_id.  Bit for bit: records [0, n) = the reference's draws of launch `counter0`, the counter one
    higher, the records past n unchanged."""
    from tests import diffaug_ref as R
    pol = tuple(p for i, p in enumerate(R.POLICIES) if f['policy'] >> i & 1)
    n = f['n']
    ref = R.table(R.draw(f['seed'], int(counter0), f['stream_id'], n, f['h'], f['w'], pol))
    t0, t1 = np.asarray(table0, dtype=np.int32), np.asarray(table1, dtype=np.int32)
    return {'table (bits)': 0.0 if np.array_equal(t1[:n], ref) else math.inf,
            'counter + 1': 0.0 if int(counter1) == int(counter0) + 1 else math.inf,
            'records past n unchanged': 0.0 if np.array_equal(t1[n:], t0[n:]) else math.inf}


def check_diffaug_draw(call):
    table, n, h, w, policy, seed, stream_id, launches = call.args[:8]
    call.plan = OPTION_PLANS['gan_diffaug_draw'](call)
    t0 = read(table, AUG_RECORDS * 8, tdtype=torch.int32).numpy().reshape(AUG_RECORDS, 8)
    c0 = int(read(launches, 1, tdtype=torch.int32)[0])
    yield
    t1 = read(table, AUG_RECORDS * 8, tdtype=torch.int32).numpy().reshape(AUG_RECORDS, 8)
    return diffaug_draw_ratios(t0, c0, t1, int(read(launches, 1, tdtype=torch.int32)[0]),
                               dict(n=n, h=h, w=w, policy=policy, seed=seed, stream_id=stream_id))


def diffaug_apply_ratios(src, dst0, dst1, c0, records, f):
    """gan_diffaug_apply, either direction.  src: the stored source view [n,h,w,c]; dst0 / dst1: whole pixels of dst before / after;
    records: the table as it stands in device memory at the call (diffaug_ref.records); f: group_c, sample0, direction, dtype.
    Gate: fp32 storage 4 fp32 ulps of the largest term of the element's arithmetic (tests/test_gpu_diffaug.py, forward_terms /
    transpose_terms).  16-bit storage: that test gates at one storage ulp of the expected value and PRESUMES inputs whose terms do
    not cancel (_inputs_are_fair), so that the fp32 error stays below the half ulp the rounding leaves free; the step's images do
    cancel, so the fp32 error is counted instead of presumed: K_ULP * ulp_storage(want) + 4 * ulp32(term) - the storage formula
    of this file with the stand-alone fp32 bound as its accumulation term.  A sample whose record makes colour the identity has its
    bits moved: equal, and the fill is +0."""
    from tests import diffaug_ref as R
    dtn = DTN[f['dtype']]
    g, s0, n, c = f['group_c'], f['sample0'], src.shape[0], src.shape[-1]
    x = src.double()
    used = records[s0:s0 + n]
    geo = list(records[:s0]) + [dict(p, brightness=0.0, saturation=1.0) for p in used]
    ones = np.ones(tuple(x.shape))
    if f['direction'] == 0:
        want = R.forward(x, records, g, s0).numpy()
        term = R.forward_terms(x.numpy(), records, g, s0)
        live = R.forward_terms(ones, geo, g, s0) > 0
        moved = np.array([p['brightness'] == 0 and (g == 1 or p['saturation'] == 1) for p in used])
    else:
        want = R.transpose(x.numpy(), records, g, s0)
        term = R.transpose_terms(x.numpy(), records, g, s0)
        live = R.transpose_terms(ones, geo, g, s0) > 0
        moved = np.array([g == 1 or p['saturation'] == 1 for p in used])
    got = dst1[..., c0:c0 + c].double().numpy()
    res = {}
    if not np.isfinite(got).all():
        res['dst'] = math.inf
    else:
        gate = 4 * R.ulp(term, 'f32') + (0.0 if dtn == 'f32' else K_ULP * R.ulp(want, dtn))
        err = np.abs(got - want)
        res['dst'] = float((err[~moved] / gate[~moved]).max()) if (~moved).any() else 0.0
        res['dst where bits move'] = 0.0 if not err[moved].any() else math.inf
    res['fill is +0'] = 0.0 if not (np.signbit(got) | (got != 0))[~live].any() else math.inf
    res['dst untouched outside the view'] = pixels_outside(dst0, dst1, c0, c)
    return res


def check_diffaug_apply(call):
    from tests import diffaug_ref as R
    d = call.args[0]._obj
    call.plan = OPTION_PLANS['gan_diffaug_apply'](call)
    src = Pixels(d.src, d.dtype).real().clone()
    dst0 = Pixels(d.dst, d.dtype)
    nrec = d.sample0 + d.src.n
    records = R.records(read(d.params, nrec * 8, tdtype=torch.int32).numpy().reshape(nrec, 8))
    yield
    dst1 = Pixels(d.dst, d.dtype)
    return diffaug_apply_ratios(src, dst0.raw, dst1.raw, dst0.c0, records,
                                dict(group_c=d.group_c, sample0=d.sample0, direction=d.direction, dtype=d.dtype))


def _strided(ptr, count, pitch, dt):
    """[count, pitch] of the storage type: element i of a gradient row lives at i * pitch (whole pixels: the rows are dlogits buffers)."""
    return read(ptr, count * pitch, dt).reshape(count, pitch) if ptr else None


def lsq_ratios(x, f, loss0, loss1, dx0, dx1):
    """gan_lsq_logits.  x: fp32 numpy [count]; f: target, loss_scale, loss_accumulate, grad_scale, dtype, ls; dx0 / dx1: [count, pitch]
    before / after (None: no gradient asked for).  lsgan_ref.check_lsq with its gates unchanged; loss_accumulate = 1: the same loss
    gate around loss0 + loss_scale * mean, plus the ONE fp32 addition (half an ulp32 of the sum; lsgan_ref.check_accumulate needs the
    unaccumulated loss of the same call, which a replayed step does not have)."""
    from tests import lsgan_ref as R
    ls0 = f['ls'] if f['ls'] is not None else 1.0
    grad = dx1[:, 0] if dx1 is not None else None
    if not f['loss_accumulate']:
        res = R.check_lsq(x, f['target'], f['grad_scale'], ls0, f['dtype'], loss1, grad, f['loss_scale'])
    else:
        ref_l, ref_g = R.lsq_ref(x, f['target'], f['grad_scale'] * ls0)
        want = float(loss0) + f['loss_scale'] * ref_l
        res = {'loss': E_r(abs(float(loss1) - want), abs(f['loss_scale']) * R.loss_gate('gan_lsq_logits', x.size, ref_l) + 0.5 * ulp32(want))}
        if grad is not None:
            res['grad'] = R.grad_ratio(grad, ref_g, f['dtype'])
    if dx1 is not None:
        res['dx untouched beside the elements'] = pixels_outside(dx0, dx1, 0, 1)
    return res


def check_lsq_logits(call):
    from tests import elementwise_ref as E
    x, count, target, loss_scale, acc, loss_out, grad_scale, dt, dx, pitch, ws, ls_ptr = call.args[:12]
    call.plan = OPTION_PLANS['gan_lsq_logits'](call)
    xs = read(x, count).numpy().copy()
    loss0 = float(read(loss_out, 1)[0])
    dx0 = _strided(dx, count, pitch, dt)
    f = dict(target=E.f32c(target), loss_scale=E.f32c(loss_scale), loss_accumulate=int(acc), grad_scale=E.f32c(grad_scale), dtype=dt,
             ls=_scale_word(ls_ptr))
    yield
    return lsq_ratios(xs, f, loss0, float(read(loss_out, 1)[0]), dx0, _strided(dx, count, pitch, dt))


def fused_lsq_ratios(real, fake, f, got, grads0, grads1):
    """gan_patchgan_losses_lsq.  real / fake: fp32 numpy [count]; f: dtype, ls, lam, l1 (the device scalar *l1 before the call);
    got: the fp32 scalars gan, disc, gen_total; grads0 / grads1: {name: [count, pitch]} before / after.  lsgan_ref.check_fused."""
    from tests import lsgan_ref as R
    g = dict(got)
    for k, t in grads1.items():
        g[k] = t[:, 0] if t is not None else None
    res = R.check_fused(real, fake, f['ls'] if f['ls'] is not None else 1.0, f['dtype'], g, lam=f['lam'], l1=f['l1'])
    for k, t in grads1.items():
        if t is not None:
            res[f'{k} untouched beside the elements'] = pixels_outside(grads0[k], t, 0, 1)
    return res


def check_patchgan_lsq(call):
    from tests import elementwise_ref as E
    real, fake, count, dt, g_dfake, d_dreal, d_dfake, pitch, lam, l1, gen_total, gan, disc, ws, ls_ptr = call.args[:15]
    call.plan = OPTION_PLANS['gan_patchgan_losses_lsq'](call)
    r, fk = read(real, count).numpy().copy(), read(fake, count).numpy().copy()
    ptrs = dict(g_dfake=g_dfake, d_dreal=d_dreal, d_dfake=d_dfake)
    g0 = {k: _strided(p, count, pitch, dt) for k, p in ptrs.items()}
    f = dict(dtype=dt, ls=_scale_word(ls_ptr), lam=E.f32c(lam), l1=float(read(l1, 1)[0]) if l1 else 0.0)
    yield
    got = dict(gan=float(read(gan, 1)[0]), disc=float(read(disc, 1)[0]), gen_total=float(read(gen_total, 1)[0]) if gen_total else None)
    return fused_lsq_ratios(r, fk, f, got, g0, {k: _strided(p, count, pitch, dt) for k, p in ptrs.items()})


def pool_ratios(src, pool0, state0, dst0, dst1, c0, pool1, state1, f):
    """gan_pool_exchange.  src: the stored current images [n,h,w,c]; pool0 / pool1: the pool [capacity,h,w,c] before / after; state0 /
    state1: the three int32 state words; dst0 / dst1: whole pixels of dst; f: seed, stream_id.  Bits are moved: dst, pool contents
    and state equal pool_ref.query of the snapshot, the block ticket is back at 0, nothing beside dst's channels changes."""
    from tests import pool_ref as R
    c = src.shape[-1]
    out, pool, (stored, launches), trace = R.query(_bits(src).numpy(), _bits(pool0).numpy(), (int(state0[0]), int(state0[1])),
                                                  f['seed'], f['stream_id'])
    return {'dst (bits)': 0.0 if np.array_equal(_bits(dst1[..., c0:c0 + c]).numpy(), out) else math.inf,
            'pool (bits)': 0.0 if np.array_equal(_bits(pool1).numpy(), pool) else math.inf,
            'state': 0.0 if [int(v) for v in state1] == [stored, launches, 0] else math.inf,
            'dst untouched outside the view': pixels_outside(dst0, dst1, c0, c)}, trace


def check_pool_exchange(call):
    d = call.args[0]._obj
    call.plan = OPTION_PLANS['gan_pool_exchange'](call)
    src = Pixels(d.src, d.dtype).real().clone()
    shape = (d.capacity, d.src.h, d.src.w, d.src.c)
    pool0 = read(d.pool, int(np.prod(shape)), d.dtype).reshape(shape)
    state0 = read(d.state, 3, tdtype=torch.int32).tolist()
    dst0 = Pixels(d.dst, d.dtype)
    yield
    dst1 = Pixels(d.dst, d.dtype)
    res, trace = pool_ratios(src, pool0, state0, dst0.raw, dst1.raw, dst0.c0, read(d.pool, int(np.prod(shape)), d.dtype).reshape(shape),
                             read(d.state, 3, tdtype=torch.int32).tolist(), dict(seed=d.seed, stream_id=d.stream_id))
    call.trace = trace
    return res


def adam_begin_sched_ratios(step0, lr_t0, lr_now0, skip, step1, lr_t1, lr_now1, f):
    """gan_adam_begin_sched.  step / lr_t / lr_now before and after (np.float32 scalars, lr_now None where the call passes NULL); skip:
    the loss scale's non-finite flag at the call; f: lr, end_factor, decay_start, decay_end, beta1, beta2.  A skipped step keeps all
    three, bit for bit; otherwise t = step0 + 1 is stored and both rates are within lr_schedule_ref.GATE_ULPS of the reference."""
    from tests import lr_schedule_ref as S
    same = lambda a, b: 0.0 if (a is None and b is None) or np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32) else math.inf
    if skip:
        return {'step kept': 0.0 if int(step1) == int(step0) else math.inf, 'lr_t kept': same(lr_t0, lr_t1), 'lr_now kept': same(lr_now0, lr_now1)}
    t = int(step0) + 1
    res = {'step + 1': 0.0 if int(step1) == t else math.inf}
    for k, v in S.check(f['lr'], f['end_factor'], f['decay_start'], f['decay_end'], f['beta1'], f['beta2'], t, lr_t1, lr_now1).items():
        res[k] = v / S.GATE_ULPS
    return res


def check_adam_begin_sched(call):
    step, lr_t, lr_now, s, b1, b2, ls_ptr = call.args[:7]
    s = s._obj
    call.plan = OPTION_PLANS['gan_adam_begin_sched'](call)
    rd = lambda: (int(read(step, 1, tdtype=torch.int32)[0]), read(lr_t, 1).numpy()[0], read(lr_now, 1).numpy()[0] if lr_now else None)
    before = rd()
    skip = bool(ls_ptr) and float(read(ls_ptr, 4)[3]) != 0.0
    yield
    return adam_begin_sched_ratios(*before, skip, *rd(), dict(lr=s.lr, end_factor=s.end_factor, decay_start=s.decay_start,
                                                               decay_end=s.decay_end, beta1=b1, beta2=b2))


def _aug_plan(call):
    d = call.args[0]._obj
    return f"{'backward' if d.direction else 'forward'} {d.src.n}x{d.src.h}x{d.src.w}x{d.src.c} group {d.group_c} sample0 {d.sample0}"


def _pool_plan(call):
    d = call.args[0]._obj
    return f"{d.src.n}x{d.src.h}x{d.src.w}x{d.src.c} capacity {d.capacity} stream {d.stream_id}"


def _sched_plan(call):
    s = call.args[3]._obj
    return f"decay [{s.decay_start}, {s.decay_end}) to x{s.end_factor:g}"


# plan strings from the descriptor / argument list alone (plan_of)
OPTION_PLANS = {
    'gan_dssim': _loss_plan, 'gan_msssim': lambda c: _loss_plan(c) + f" M{c.args[0]._obj.scales}", 'gan_edge_l1': _loss_plan,
    'gan_diffaug_apply': _aug_plan, 'gan_pool_exchange': _pool_plan,
    'gan_adam_begin_sched': _sched_plan,
    'gan_diffaug_draw': lambda c: f"{c.args[1]} records {c.args[2]}x{c.args[3]} policy {c.args[4]:#x} stream {c.args[6]}",
    'gan_lsq_logits': lambda c: f"count {c.args[1]} target {c.args[2]:g} loss x{c.args[3]:g}{' acc' if c.args[4] else ''} grad x{c.args[6]:g}"
                                + (' ls' if c.args[11] else ''),
    'gan_patchgan_losses_lsq': lambda c: f"count {c.args[2]} lambda {c.args[8]:g}" + (' ls' if c.args[14] else ''),
}
CHECKERS.update(gan_dssim=check_dssim, gan_msssim=check_msssim, gan_edge_l1=check_edge, gan_diffaug_draw=check_diffaug_draw, gan_diffaug_apply=check_diffaug_apply,
                gan_lsq_logits=check_lsq_logits, gan_patchgan_losses_lsq=check_patchgan_lsq, gan_pool_exchange=check_pool_exchange,
                gan_adam_begin_sched=check_adam_begin_sched)


# ---- which calls an option audit checks, and how the rest earns AS_ONE_GPU ----------------------------------------------------------
def _span(ptr, elems, es):
    return (_void(ptr), _void(ptr) + elems * es)


def _tensor_span(t, es):
    rows = t.n * t.h * t.w
    return _span(t.ptr, (rows - 1) * t.pitch + t.c if rows else 0, es)


def option_regions(step):
    """Address ranges of the buffers only an option creates: aug_raw and aug_dgen of a DiffAugment step; with image pools the pooled
    third (samples B .. 2B-1) of every forward buffer of both discriminators' three-invocation calls."""
    reg = []
    rng = lambda t: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
    if getattr(step, 'diffaug', None) is not None:
        reg += [rng(step.aug_raw.t), rng(step.aug_dgen.t)]
    if getattr(step, 'pools', None):
        B = step.B
        for d in (step.dx, step.dy):
            for buf in [d.xin, d.logits] + list(d.y.values()) + list(d.a.values()):
                reg.append(rng(buf.t[B:2 * B]))
    return reg


def option_call(regions):
    """Predicate of replay(check=...): the option entry points, and every conv / dgrad / wgrad call with an operand in `regions`."""
    def hit(t, dt):
        a, b = _tensor_span(t, TDT[dt].itemsize)
        return any(a < hi and lo < b for lo, hi in regions)

    def check(call):
        if call.name in OPTION_ENTRIES:
            return True
        if call.name in OPS:
            d = call.args[0]._obj
            return hit(d.x, d.dtype) or hit(d.y, L.F32 if d.y_f32 else d.dtype)
        if call.name == 'gan_conv_wgrad':
            d = call.args[0]._obj
            return hit(d.big, d.dtype) or hit(d.small, d.dtype)
        return False
    return check


OPTION_MAP = {'gan_lsq_logits': 'gan_bce_logits', 'gan_patchgan_losses_lsq': 'gan_patchgan_losses', 'gan_adam_begin_sched': 'gan_adam_begin',
              'gan_dssim': 'gan_l1', 'gan_msssim': 'gan_l1'}       # an option entry point that stands in the place of a plain one, argument for argument
OPTION_STRUCK = ('gan_edge_l1', 'gan_diffaug_draw', 'gan_diffaug_apply', 'gan_pool_exchange')       # ... that the plain step has no call for
ANY = 'checked'              # the key of a call the audit checks itself: its plan class need not be the plain step's
# gan_msssim takes one of two places, and the caller says which (same_as_plain(msssim=...), the step's generator_loss): 'msssim' - it
# stands where gan_l1 stood (OPTION_MAP, as gan_dssim); 'msssim_l1' - gan_l1 stays and gan_msssim is an extra call directly behind it
# (struck); None - the step has no MS-SSIM loss and must not record the entry point at all.
MSSSIM_PLACES = (None, 'msssim', 'msssim_l1')


def same_as_plain(option, plain, replaced_copy=None, msssim=None):
    """The rule by which the unchecked calls of an option step carry AS_ONE_GPU.  option / plain: [(entry point, key)] in recorded
    order; key = the plan class of a conv / wgrad call (call_class), None for every other entry point, ANY for a call the audit
    checks.  Strike OPTION_STRUCK from the option list, map the entry points of OPTION_MAP back (tests/test_gpu_lsgan.py::
    test_launch_lists; gan_dssim stands where gan_l1 stood), strike from the plain list the one gan_copy_view that
    gan_diffaug_apply replaces (its index: replaced_copy): the two sequences must then be equal, entry for entry.
    msssim (MSSSIM_PLACES): the place gan_msssim takes.  Striking and mapping alone cannot see a second gan_msssim behind gan_l1 or
    one that has changed places with the (struck) edge term, so with either place there is exactly one such call, no gan_edge_l1 in
    front of it, and for 'msssim_l1' the call directly in front of it is gan_l1; without a place there is none.
    -> the differences as strings (empty: the rule holds)."""
    assert msssim in MSSSIM_PLACES, msssim
    bad = []
    at = [i for i, (n, _) in enumerate(option) if n == 'gan_msssim']
    if len(at) != (msssim is not None):
        bad.append(f"{len(at)} gan_msssim calls at {at} in a step with generator loss {msssim or 'l1 / dssim'}")
    for i in at:
        if any(n == 'gan_edge_l1' for n, _ in option[:i]):
            bad.append(f"position {i}: gan_msssim behind the edge term")
        if msssim == 'msssim_l1' and (i == 0 or option[i - 1][0] != 'gan_l1'):
            bad.append(f"position {i}: gan_msssim of 'msssim_l1' behind {option[i - 1][0] if i else 'nothing'}, not gan_l1")
    struck = OPTION_STRUCK + (('gan_msssim',) if msssim == 'msssim_l1' else ())
    a = [(OPTION_MAP.get(n, n), k) for n, k in option if n not in struck]
    b = list(plain)
    if replaced_copy is not None:
        assert b[replaced_copy][0] == 'gan_copy_view', b[replaced_copy]
        del b[replaced_copy]
    if len(a) != len(b):
        bad.append(f"{len(a)} calls left of the option step, {len(b)} of the plain one")
    for i, ((n1, k1), (n2, k2)) in enumerate(zip(a, b)):
        if n1 != n2 or (k1 != ANY and k1 != k2):
            bad.append(f"position {i}: option step {n1} {k1}, plain step {n2} {k2}")
            if len(bad) >= 12:
                break
    return bad


def sequence_of(calls, check=None):
    """[(entry point, key)] of recorded calls for same_as_plain: check = the audit's predicate (None: the plain step, every class kept)."""
    return [(c.name, ANY if check is not None and check(c) else call_class(c)) for c in calls]


def issue(calls, stream=None):
    """The recorded calls re-issued one by one, in recorded order, on one stream, unchecked (the serial order a captured graph's
    dependency edges must be equivalent to)."""
    st = (stream or torch.cuda.current_stream()).cuda_stream
    for c in calls:
        rc = c.fn(*c.args[:-1], st)
        if rc:
            L.check(rc, f"{c.name} ({c.label})")
    torch.cuda.synchronize()


# ---- the option-carrying step, built as captured_step builds the plain one -----------------------------------------------------------
POOL_CAPACITY = 3
AUG_LAUNCH0 = 5              # the DiffAugment launch counter at the known start (not 0: the counter must be READ)
AUG_FILL = 0x5A5A5A5A        # what every table record holds before the draw
SCHED_STEP0 = 2              # the step counters of a scheduled step at the known start: update index 2 of STEP_SCHEDULE runs at lr / 2


def lattice(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, tuple(shape), generator=g).float() / 127.5 - 1.0


def pool_launches(batch, capacity, seed, stream_id, want):
    """The smallest launch counter at which a full pool's query decides `want` ('swap' / 'keep') for its first image."""
    from tests import pool_ref
    for k in range(1, 256):
        if pool_ref.decisions(batch, capacity, seed, stream_id, capacity, k)[0][0][0] == want:
            return k
    raise AssertionError(want)


class OptionStart:
    """Puts an option step at its known start: reset_step (unchanged), then every tensor of DiffAugment.tensors(), every tensor of
    each ImagePool.tensors() - full pools of lattice images, pool_y at a launch counter where its first image is swapped, pool_x
    where it is kept, so that the two exchanges of a step take both branches - the mask_draws counters, lr_now and the step counters
    of a scheduled step, the loss-scale state, and the lattice inputs."""

    def __init__(self, step, saved, replay_, inputs, ls0):
        self.step, self.saved, self.replay, self.inputs, self.ls0 = step, saved, replay_, inputs, ls0

    def __call__(self):
        st = self.step
        reset_step(st, self.saved)
        for net in st.nets():
            P = net.params
            if P.lr_schedule is not None:
                P.step.fill_(SCHED_STEP0)
                P.lr_now.fill_(float(P.lr_schedule.lr))
        for call in vars(st).values():
            if hasattr(call, 'mask_draws'):
                call.mask_draws.zero_()
        aug = getattr(st, 'diffaug', None)
        if aug is not None:
            launches, table = aug.tensors()
            launches.fill_(AUG_LAUNCH0)
            table.fill_(AUG_FILL)
        for i, pool in enumerate(getattr(st, 'pools', None) or ()):
            state, storage = pool.tensors()
            storage.copy_(lattice(storage.shape, 31 + i).to(storage.dtype))
            k = pool_launches(st.B, pool.capacity, pool.seed, pool.stream_id, ('swap', 'keep')[i])
            state.copy_(torch.tensor([pool.capacity, k, 0], dtype=torch.int32))
        if self.ls0 is not None:
            st.ctx.ls.copy_(self.ls0)
        for t, src in zip(self.replay.inputs, self.inputs):
            t.copy_(src)
        torch.cuda.synchronize()


def option_step(model, dtype, channels, batch, monkeypatch, size=256, generator_loss='l1', edge_weight=0.0, diffaug=None, gan_loss='bce',
                lr_schedule=None, pools=None, msssim_alpha=0.84):
    """captured_step with the option keywords and `channels`: recorder first, then build, capture, reset.  diffaug: the policies
    (a comma-separated string) or None; lr_schedule: (decay_start, decay_end, end_factor) or None; pools: the capacity or None;
    msssim_alpha: the mixing weight of generator_loss 'msssim_l1' (the product's default).
    -> (step, labelled calls, the captured replay, the OptionStart that was just run)."""
    import gc
    from gan_amd.diffaug import DiffAugment
    from gan_amd.nets import Ctx, LrSchedule, workspace_mb_for
    from gan_amd.pool import STREAM_X, STREAM_Y, ImagePool
    from gan_amd.steps import CycleGANStep, Pix2PixStep
    gc.collect()                                  # (graphs of the previous case: see captured_step)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    rec = Recorder(monkeypatch)
    rec.hook_capture(monkeypatch)
    ctx = Ctx('cuda:0', dtype, workspace_mb=workspace_mb_for(batch, size, channels, calls=3 if pools else 2))
    ls0 = ctx.ls.clone() if ctx.ls is not None else None
    sched = LrSchedule(2e-4, lr_schedule[2], lr_schedule[0], lr_schedule[1]) if lr_schedule else None
    if model == 'pix2pix':
        assert pools is None and generator_loss in ('l1', 'dssim', 'msssim', 'msssim_l1'), (pools, generator_loss)
        aug = DiffAugment(ctx, diffaug, seed=123) if diffaug else None
        st = Pix2PixStep(ctx, batch, size, channels, lam=100.0, seed=123, generator_loss=generator_loss, gan_loss=gan_loss,
                         lr_schedule=sched, diffaug=aug, edge_weight=edge_weight, msssim_alpha=msssim_alpha)
    else:
        assert generator_loss == 'l1' and not edge_weight and diffaug is None
        pl = (ImagePool(ctx, size, channels, pools, 123, STREAM_Y), ImagePool(ctx, size, channels, pools, 123, STREAM_X)) if pools else None
        st = CycleGANStep(ctx, batch, size, channels, lam=10.0, seed=123, gan_loss=gan_loss, lr_schedule=sched, pools=pl)
    saved = [(n.params.master.clone(), {k: t.clone() for k, t in n.params.state.items()}) for n in st.nets()]
    replay_ = st.capture(training=True)
    torch.cuda.synchronize()
    calls = rec.calls
    assert calls, "nothing recorded inside the capture body"
    label_calls(calls, st)
    inputs = [lattice(t.shape, 7 + batch + 100 * i).to(t.device) for i, t in enumerate(replay_.inputs)]
    start = OptionStart(st, saved, replay_, inputs, ls0)
    start()
    return st, calls, replay_, start


NEAR_SEED = 977              # of the lattice noise near_target adds


def near_target(step, start, amp):
    """Give a Pix2Pix option step a target near its generator's own output: the operands gan_msssim's loss gate is derived for
    (tests/test_gpu_msssim.py: a = clip(b + amp * U); an untrained generator against an independent lattice image has its factors at the
    clamp).  Pix2Pix's G reads only the un-augmented input x, and start() resets the weights, the norm state and the dropout
    counters, so G's output at the known start is reproducible and does not depend on the target: start(), one replay, read G's
    stored output, target = clip(gen + amp * lattice noise, -1, 1) rounded to the 8-bit lattice of the inputs, in start.inputs (so
    that every later start() restores it), start() again.  Whether the premise holds on the result is the checker's 'premise' row."""
    start()
    start.replay(*start.replay.inputs)
    torch.cuda.synchronize()
    gen = step.g.output_f32().double().cpu()
    tar = torch.clamp(gen + amp * lattice(gen.shape, NEAR_SEED).double(), -1.0, 1.0)
    tar = torch.round((tar + 1.0) * 127.5) / 127.5 - 1.0
    assert tuple(start.inputs[1].shape) == tuple(tar.shape), (tuple(start.inputs[1].shape), tuple(tar.shape))
    start.inputs[1] = tar.float().to(start.inputs[1].device)
    start()


# ---- the captured one-GPU step at channels = 1: what tests/test_gpu_launch_audit.py and tests/test_gpu_wide_audit.py replay ----------
def reset_step(step, saved):
    for net, (P, state) in zip(step.nets(), saved):
        ps = net.params
        ps.master.copy_(P)
        ps.prepare()
        # non-zero moments: the fused-Adam checks then see the carried beta * m_old / beta2 * v_old terms too, and the blocks a
        # launch may skip where the gradient is zero (wgrad.dead_taps) must still apply them
        g = torch.Generator(device='cpu').manual_seed(11)
        ps.m.copy_(1e-4 * torch.randn(ps.m.shape, generator=g))
        ps.v.copy_(1e-8 * torch.rand(ps.v.shape, generator=g) + 1e-10)
        ps.step.zero_(); ps.grad.zero_()
        for k, t in ps.state.items():
            t.copy_(state[k])


def captured_step(model, dtype, size, batch, monkeypatch):
    """Build the step, capture it as bench.py does with every library call of the capture body recorded, then put it at the known
    start: initial weights, step 0, small random moments (reset_step), inputs on the normalize() lattice (base_gan.py:56-61).
    -> (step, labelled calls, the captured replay: the caller keeps it alive while it re-issues the calls)."""
    import gc
    from gan_amd.nets import Ctx, workspace_mb_for
    from gan_amd.steps import CycleGANStep, Pix2PixStep
    # the graphs and events of the previous case must be gone before this one captures: destroying them inside a capture (a cyclic
    # garbage collection run at an allocation) aborts the process
    gc.collect()
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    rec = Recorder(monkeypatch)                   # before the step object: its op lists hold the bound entry points
    rec.hook_capture(monkeypatch)
    ctx = Ctx('cuda:0', dtype, workspace_mb=workspace_mb_for(batch, size))
    if model == 'pix2pix':
        st = Pix2PixStep(ctx, batch, size, 1, lam=100.0, seed=123)
    else:
        st = CycleGANStep(ctx, batch, size, 1, lam=10.0, seed=123)
    saved = [(n.params.master.clone(), {k: t.clone() for k, t in n.params.state.items()}) for n in st.nets()]
    replay_ = st.capture(training=True)           # what bench.py captures
    torch.cuda.synchronize()
    calls = rec.calls
    assert calls, "nothing recorded inside the capture body"
    label_calls(calls, st)
    reset_step(st, saved)
    g = torch.Generator().manual_seed(7 + batch)
    for t in replay_.inputs:
        t.copy_((torch.randint(0, 256, tuple(t.shape), generator=g).float() / 127.5 - 1.0).to(t.device))
    torch.cuda.synchronize()
    return st, calls, replay_


def report(title, rows, t0, t1, t2):
    """Print the table, the worst error / gate per entry point and the times of one case."""
    print('\n' + table(rows, title))
    worst = worst_per_entry(rows)
    print(f"[{title}] worst error/gate per entry point: " + ', '.join(f"{k[4:]} {v:.3f}" for k, v in sorted(worst.items())))
    print(f"[{title}] {len(rows)} calls ({sum(r[4] is not None for r in rows)} checked); "
          f"build + capture {t1 - t0:.1f} s, audit {t2 - t1:.1f} s")


AS_ONE_GPU = 'as in the one-GPU step'
TIMES = []                   # (seconds, label, entry point) of every call of the last replays: where a case's time goes


def replay(calls, stream=None, check=None, wire=None):
    """Re-issue the recorded calls in order on one stream, each checked against its reference.  Returns rows
    (label, entry point, plan, kernels, {item: error/gate}) - None for allowlisted entry points.
    check: a predicate of a call - a call it rejects is issued unchecked and its row's plan reads AS_ONE_GPU (its entry point must
    still have a checker or an ALLOWLIST entry).  wire: the WireAudit of a data-parallel capture - gan_grad_pack then has its range
    recorded (check_pack_range), whatever the predicate says, and every wgrad launch is held to the wire buffers."""
    global _WIRE
    lib = L.load()
    stream = stream or torch.cuda.current_stream()
    st = stream.cuda_stream
    rows = []
    _WIRE = wire
    for c in calls:
        chk = CHECKERS.get(c.name)
        if chk is None and c.name not in ALLOWLIST:
            _WIRE = None
            raise AssertionError(f"{c.name} ({c.label}) has neither a reference in tests/launch_audit.py nor an ALLOWLIST entry")
        if wire is not None and c.name == 'gan_grad_pack':
            chk = check_pack_range
        elif chk is not None and check is not None and not check(c):
            chk = None
        torch.cuda.synchronize()
        t_call = time.time()
        c.plan = ''
        gen = chk(c) if chk is not None else None
        if gen is not None:
            try:
                next(gen)                                       # snapshot
            except BaseException:
                _WIRE = None
                raise
            assert c.name == 'gan_grad_pack' or c.plan == plan_of(c), (c.name, c.plan, plan_of(c))
        elif c.name in CHECKERS:
            c.plan = AS_ONE_GPU
        L.check(lib.gan_set_option(b'diag.launch_log', 1), "launch log")
        rc = c.fn(*c.args[:-1], st)
        torch.cuda.synchronize()
        syms = [_short(s) for s in L.launch_log()]
        L.check(lib.gan_set_option(b'diag.launch_log', 0), "launch log")
        if rc:
            L.check(rc, f"{c.name} ({c.label})")
        res = None
        if gen is not None:
            try:
                next(gen)
            except StopIteration as e:
                res = e.value
        rows.append((c.label, c.name, c.plan, ','.join(dict.fromkeys(syms)), res))
        TIMES.append((time.time() - t_call, c.label, c.name))
    _WIRE = None
    return rows


def table(rows, title=''):
    lines = [f"== launch audit {title}: {len(rows)} calls"]
    for lab, name, plan, ks, res in rows:
        if res is None:
            lines.append(f"  {lab[:44]:44s} {name[4:]:22s} {plan if plan == AS_ONE_GPU else 'allowlisted'}")
            continue
        worst = max(res.items(), key=lambda kv: kv[1]) if res else ('-', 0.0)
        lines.append(f"  {lab[:44]:44s} {name[4:]:22s} {plan:50s} {ks[:70]:70s} {worst[0]} {worst[1]:.3f}")
    return '\n'.join(lines)


def failures(rows):
    return [(lab, name, plan, k, v) for lab, name, plan, ks, res in rows if res for k, v in res.items() if not v <= 1.0]


def worst_per_item(rows, name):
    """{item: worst error / gate} over the rows of one entry point."""
    w = {}
    for lab, nm, plan, ks, res in rows:
        if res and nm == name:
            for k, v in res.items():
                w[k] = max(w.get(k, 0.0), v)
    return w


def worst_per_entry(rows):
    w = {}
    for lab, name, plan, ks, res in rows:
        if res:
            v = max(res.values())
            w[name] = max(w.get(name, 0.0), v)
    return w
