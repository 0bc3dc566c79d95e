"""The option-carrying training steps per launch against fp64 (tests/launch_audit.py): dSSIM, MS-SSIM alone and mixed
with L1, the Sobel edge term, DiffAugment, the least-squares GAN loss, the learning-rate schedule and CycleGAN's image pools, in the
captured, laned step, at f32 / bf16 / f16 and at channels 1 and 3.  Every case is at 256x256 (for MS-SSIM's five scales the smallest
size the U-Net admits: 176 is the minimum side); batch 2 for Pix2Pix (the smallest at which no BatchNorm layer sees one value per
channel), 1 for CycleGAN.  An MS-SSIM case runs on a target near the generator's own output (launch_audit.near_target, amplitude
NEAR_AMP): the loss gate of gan_msssim is derived for factors of at least 0.4, which an untrained generator against an independent
lattice image does not give; the checker's 'premise' row holds the inputs to it, from the reference alone.

Per case:
  a. the audit: replay(check=option_call(...)) checks the calls of the nine option entry points and every conv / dgrad / wgrad call
     with an operand in a buffer only the option creates (aug_raw, aug_dgen, the pooled third of D's batch); the rest is issued
     unchecked and carries AS_ONE_GPU, which it earns against the same step built without the options in the same test
     (launch_audit.same_as_plain); every option entry point the case was built for is among the checked rows the expected number of times;
  b. the wiring, from the recorded descriptors' pointers and scalars;
  c. the captured graph against the serial order: one graph launch and one unchecked one-stream re-issue of the recorded calls from
     the same start leave the same bits in the losses, every network's grad / master / m / v / step, every image-side buffer, the
     DiffAugment table and counter, the pools and the MS-SSIM workspace (2 M + 1 launches on the side lane beside D's forward, gan_l1
     in front and gan_edge_l1 behind on the same g.dgen) - the one-stream audit cannot see a missing dependency edge between lanes;
  d. the pad channels of every image-side buffer (aug_raw and aug_dgen among them) are bit-zero before the first and after the last call;
  e. f16: the loss-scale state after the replay is that of a finite, applied step."""
import gc
import time

import numpy as np
import pytest
import torch

from tests import launch_audit as A
from tests.lr_schedule_ref import STEP_SCHEDULE
from tests.test_gpu_rgb_audit import image_buffers

pytestmark = pytest.mark.gpu

ALL = 'translation,cutout,brightness,saturation'
W_EDGE = 0.25
SCHED = (STEP_SCHEDULE[0], STEP_SCHEDULE[1], STEP_SCHEDULE[2])        # (decay_start, decay_end, end_factor)
MSSSIM = ('msssim', 'msssim_l1')
NEAR_AMP = 0.1               # tests/test_gpu_msssim.py::AMPS[0].  Were the reference's smallest factor under 0.4 on a case: 0.05, then 0.025
CASES = [
    ('pix2pix', 'bf16', 1, dict(generator_loss='dssim', edge_weight=W_EDGE, diffaug=ALL, gan_loss='lsgan', lr_schedule=SCHED)),
    ('pix2pix', 'f16', 1, dict(generator_loss='dssim', edge_weight=W_EDGE)),
    ('pix2pix', 'f16', 3, dict(edge_weight=W_EDGE, diffaug=ALL)),
    ('pix2pix', 'bf16', 3, dict(generator_loss='dssim', edge_weight=W_EDGE, diffaug=ALL)),
    ('pix2pix', 'f32', 3, dict(edge_weight=W_EDGE, diffaug=ALL)),
    ('cyclegan', 'bf16', 1, dict(pools=A.POOL_CAPACITY, gan_loss='lsgan', lr_schedule=SCHED)),
    ('cyclegan', 'f16', 3, dict(pools=A.POOL_CAPACITY)),
    ('pix2pix', 'bf16', 1, dict(generator_loss='msssim', edge_weight=W_EDGE, diffaug=ALL, gan_loss='lsgan', lr_schedule=SCHED)),
    ('pix2pix', 'f16', 1, dict(generator_loss='msssim')),                     # the storing form under a loss-scale word
    ('pix2pix', 'f16', 3, dict(generator_loss='msssim_l1', edge_weight=W_EDGE)),           # the product's default alpha, 0.84
    ('pix2pix', 'f32', 3, dict(generator_loss='msssim_l1', msssim_alpha=0.5, diffaug=ALL)),
]


def case_id(case):
    model, dtype, ch, opts = case
    tags = [('dssim', opts.get('generator_loss') == 'dssim'), ('msssim', opts.get('generator_loss') == 'msssim'),
            ('msssim_l1', opts.get('generator_loss') == 'msssim_l1'), ('alpha', opts.get('msssim_alpha')), ('edge', opts.get('edge_weight')), ('diffaug', opts.get('diffaug')),
            ('lsgan', opts.get('gan_loss') == 'lsgan'), ('sched', opts.get('lr_schedule')), ('pools', opts.get('pools'))]
    return f"{model}-{dtype}-ch{ch}-" + '+'.join(t for t, on in tags if on)


def expected_counts(model, opts):
    """{option entry point: checked calls per training step} of a case."""
    nets = 2 if model == 'pix2pix' else 4
    n = {}
    if opts.get('generator_loss') == 'dssim':
        n['gan_dssim'] = 1
    if opts.get('generator_loss') in MSSSIM:
        n['gan_msssim'] = 1
    if opts.get('edge_weight'):
        n['gan_edge_l1'] = 1
    if opts.get('diffaug'):
        n['gan_diffaug_draw'], n['gan_diffaug_apply'] = 1, 4
    if opts.get('gan_loss') == 'lsgan':
        n['gan_patchgan_losses_lsq' if model == 'pix2pix' else 'gan_lsq_logits'] = 1 if model == 'pix2pix' else 6
    if opts.get('lr_schedule'):
        n['gan_adam_begin_sched'] = nets
    if opts.get('pools'):
        n['gan_pool_exchange'] = 2
    return n


def kept(st):
    """A copy of everything the graph-against-serial comparison holds bit-equal."""
    out = {'losses': st.losses}
    for tag, net in A._nets_of(st):
        for k in ('grad', 'master', 'm', 'v', 'step'):
            out[f"{tag}.{k}"] = getattr(net.params, k)
    for name, t, _ in image_buffers(st):
        out[name] = t
    if getattr(st, 'diffaug', None) is not None:
        out['aug_raw'] = st.aug_raw.t
        out['diffaug.launches'], out['diffaug.table'] = st.diffaug.tensors()
    for i, pool in enumerate(getattr(st, 'pools', None) or ()):
        out[f'pool{i}.state'], out[f'pool{i}.storage'] = pool.tensors()
    if hasattr(st, 'msssim_ws'):
        out['msssim_ws'] = st.msssim_ws
    if st.ctx.ls is not None:
        out['loss scale'] = st.ctx.ls
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def pix2pix_wiring(st, calls, dtype, opts):
    """Failures (strings) of item b for a Pix2Pix step."""
    B, C, g, d = st.B, st.C, st.g, st.d
    key, at = A.tensor_key, lambda name: [i for i, c in enumerate(calls) if c.name == name]
    aug = st.diffaug
    raw = st.aug_raw if aug is not None else d.xin
    ls_ptr = st.ctx.ls_ptr or 0
    bad = []
    if (ls_ptr != 0) != (dtype == 'f16'):
        bad.append(f"loss-scale state {ls_ptr:#x} at {dtype}")
    want = dict(a=key(g.out_view()), b=key(raw.view(C, C, 0, B)), da=key(g.dgen.view(0, C)), loss_out=st.losses.data_ptr() + 8, scale_state=ls_ptr)
    kind = opts.get('generator_loss', 'l1')
    f32 = lambda v: float(np.float32(v))
    if kind in MSSSIM:
        # gan_msssim alone, or directly behind gan_l1 and accumulating into its loss word and gradient; the scalars as the fp32
        # values the step's own double products (steps.py: loss_scale * al, grad_scale * (1.0 - al), ...) round to
        al = st.msssim_alpha if kind == 'msssim_l1' else 1.0
        if kind == 'msssim_l1' and al != opts.get('msssim_alpha', 0.84):
            bad.append(f"msssim_alpha {al}")
        (i,) = at('gan_msssim')
        s = calls[i].args[0]._obj
        got = dict(a=key(s.a), b=key(s.b), da=key(s.da), loss_out=A._void(s.loss_out), scale_state=A._void(s.scale_state))
        if got != want:
            bad.append(f"gan_msssim: {got}, expected {want}")
        acc = int(kind == 'msssim_l1')
        sc = (s.loss_scale, s.loss_accumulate, s.grad_scale, s.grad_accumulate)
        if sc != ((1.0, 0, f32(st.lam), 0) if not acc else (f32(1.0 * al), 1, f32(st.lam * al), 1)):
            bad.append(f"gan_msssim scalars (loss scale, accumulate, grad scale, accumulate) {sc} at alpha {al}")
        if (A._void(s.workspace), s.workspace_bytes) != (st.msssim_ws.data_ptr(), st.msssim_ws.numel() * 4):
            bad.append(f"gan_msssim workspace {A._void(s.workspace):#x} + {s.workspace_bytes}")
        if s.scales != 5 or list(s.power) != list(A.L.msssim_power(5)) or A._void(s.per_image):
            bad.append(f"gan_msssim scales {s.scales} power {list(s.power)} per_image {A._void(s.per_image):#x}")
        if (s.dtype_a, s.dtype_b, s.dtype_da) != (st.ctx.dt,) * 3:
            bad.append(f"gan_msssim dtypes {(s.dtype_a, s.dtype_b, s.dtype_da)}")
        l1 = at('gan_l1')
        if not acc:
            if l1:
                bad.append(f"'msssim' records gan_l1 at {l1}")
        elif l1 != [i - 1]:
            bad.append(f"'msssim_l1': gan_l1 at {l1}, gan_msssim at {i}")
        else:
            a_ = calls[i - 1].args
            got = dict(a=key(a_[1]._obj), b=key(a_[2]._obj), da=key(a_[7]._obj), loss_out=A._void(a_[5]), scale_state=A._void(a_[9]))
            if got != want:
                bad.append(f"gan_l1 of 'msssim_l1': {got}, expected {want}")
            sc = (f32(a_[3]), a_[4], f32(a_[6]))
            if sc != (f32(1.0 * (1.0 - al)), 0, f32(st.lam * (1.0 - al))):
                bad.append(f"gan_l1 scalars of 'msssim_l1' (loss scale, accumulate, grad scale) {sc} at alpha {al}")
    elif kind == 'dssim':
        (i,) = at('gan_dssim')
        s = calls[i].args[0]._obj
        got = dict(a=key(s.a), b=key(s.b), da=key(s.da), loss_out=A._void(s.loss_out), scale_state=A._void(s.scale_state))
        sec = (s.loss_scale, s.loss_accumulate, s.grad_scale)
    else:
        (i,) = at('gan_l1')
        a_ = calls[i].args
        got = dict(a=key(a_[1]._obj), b=key(a_[2]._obj), da=key(a_[7]._obj), loss_out=A._void(a_[5]), scale_state=A._void(a_[9]))
        sec = (a_[3], a_[4], a_[6])
    if kind not in MSSSIM:
        if got != want:
            bad.append(f"secondary loss: {got}, expected {want}")
        if sec != (1.0, 0, np.float32(st.lam)):
            bad.append(f"secondary loss scalars (loss scale, accumulate, grad scale) {sec}")
    if opts.get('edge_weight'):
        (j,) = at('gan_edge_l1')
        e = calls[j].args[0]._obj
        got = dict(a=key(e.a), b=key(e.b), da=key(e.da), loss_out=A._void(e.loss_out), scale_state=A._void(e.scale_state))
        if got != want:
            bad.append(f"edge term: {got}, expected {want}")
        w = st.edge_weight
        if (e.loss_accumulate, e.grad_accumulate, e.loss_scale, e.grad_scale) != (1, 1, np.float32(w), np.float32(st.lam * w)):
            bad.append(f"edge term scalars {(e.loss_accumulate, e.grad_accumulate, e.loss_scale, e.grad_scale)}")
        if not j > i:                     # (i: the secondary loss - with an MS-SSIM loss the gan_msssim call, behind its gan_l1)
            bad.append(f"edge term recorded at {j}, the secondary loss at {i}")
    elif at('gan_edge_l1'):
        bad.append(f"a step without an edge weight records gan_edge_l1 at {at('gan_edge_l1')}")
    if aug is None:
        return bad
    (k,) = at('gan_diffaug_draw')
    dr = calls[k].args
    if (dr[0], dr[1], dr[2], dr[3], dr[4], dr[5], dr[6], dr[7]) != (aug.table.data_ptr(), 2 * B, st.S, st.S, aug.mask, aug.seed, aug.stream_id,
                                                                  aug.launches.data_ptr()):
        bad.append(f"draw arguments {dr[:8]}")
    ap = at('gan_diffaug_apply')
    desc = lambda i_: calls[i_].args[0]._obj
    got = {(key(desc(i_).src), key(desc(i_).dst), desc(i_).group_c, desc(i_).sample0, desc(i_).direction): i_ for i_ in ap}
    back = (key(st.aug_dgen.view(0, C)), key(g.dgen2.view(0, C)), C, B, 1)
    want = {(key(raw.view(0, 2 * C, 0, B)), key(d.xin.view(0, 2 * C, 0, B)), C, 0, 0),
            (key(raw.view(0, C, B, B)), key(d.xin.view(0, C, B, B)), C, B, 0),
            (key(g.out_view()), key(d.xin.view(C, C, B, B)), C, B, 0), back}
    if set(got) != want or len(ap) != 4:
        bad.append(f"apply calls {sorted(got)}, expected {sorted(want)}")
    if any(A._void(desc(i_).params) != aug.table.data_ptr() or desc(i_).dtype != st.ctx.dt for i_ in ap):
        bad.append("an apply call reads another table or dtype")
    if not k < min(ap):
        bad.append("an apply call is recorded before the draw")
    dx = [i_ for i_ in at('gan_conv2d_dgrad') if key(calls[i_].args[0]._obj.y) == key(st.aug_dgen.view(0, C))]
    wk = st.D.params.nat['down0.kernel']
    if len(dx) != 1:
        bad.append(f"{len(dx)} dgrad calls write aug_dgen")
    else:
        dd = calls[dx[0]].args[0]._obj
        if A._void(dd.w) != wk.data_ptr() + C * wk.shape[2] * wk.element_size() or dd.w_rows != 2 * C or 'D.down0' not in calls[dx[0]].label:
            bad.append(f"D.down0's dx dgrad: w {A._void(dd.w):#x} rows {dd.w_rows} label {calls[dx[0]].label!r}")
        if back in got and not dx[0] < got[back]:
            bad.append("the transpose is recorded before D.down0's dx dgrad")
    return bad


def cyclegan_wiring(st, calls, dtype, opts):
    from gan_amd.pool import STREAM_X, STREAM_Y
    B, C = st.B, st.C
    key = A.tensor_key
    if not opts.get('pools'):
        return []
    got = set()
    for c in calls:
        if c.name == 'gan_pool_exchange':
            p = c.args[0]._obj
            got.add((key(p.src), key(p.dst), A._void(p.pool), A._void(p.state), p.capacity, p.stream_id, p.seed, p.dtype))
    py, px = st.pools
    want = {(key(st.fy.out_view()), key(st.dy.xin.view(0, C, B, B)), py.storage.data_ptr(), py.state.data_ptr(), py.capacity, STREAM_Y, py.seed, st.ctx.dt),
            (key(st.fx.out_view()), key(st.dx.xin.view(0, C, B, B)), px.storage.data_ptr(), px.state.data_ptr(), px.capacity, STREAM_X, px.seed, st.ctx.dt)}
    return [] if got == want else [f"pool exchanges {sorted(got)}, expected {sorted(want)}"]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_option_step_per_launch_against_fp64(case, monkeypatch):
    model, dtype, ch, opts = case
    batch = 2 if model == 'pix2pix' else 1
    title = f"options {case_id(case)} 256x256 B={batch}"
    t0 = time.time()
    # the same step without the options: its (entry point, plan class) sequence is what the unchecked calls must repeat
    pst, pcalls, preplay, _ = A.option_step(model, dtype, ch, batch, monkeypatch)
    plain = A.sequence_of(pcalls)
    replaced = None
    if opts.get('diffaug'):
        slot = A.tensor_key(pst.d.xin.view(ch, ch, batch, batch))
        (replaced,) = [i for i, c in enumerate(pcalls) if c.name == 'gan_copy_view' and A.tensor_key(c.args[2]._obj) == slot]
    assert not set(n for n, _ in plain) & set(A.OPTION_ENTRIES)
    del pst, pcalls, preplay
    gc.collect()
    st, calls, replay_, start = A.option_step(model, dtype, ch, batch, monkeypatch, **opts)
    ctx = st.ctx
    msssim = opts.get('generator_loss') if opts.get('generator_loss') in MSSSIM else None
    if msssim:                  # before anything is compared: the target near G's own output, part of the known start from here on
        A.near_target(st, start, NEAR_AMP)
    check = A.option_call(A.option_regions(st))
    bad = A.same_as_plain(A.sequence_of(calls, check), plain, replaced, msssim=msssim)
    assert not bad, "the unchecked calls are not those of the plain step:\n" + '\n'.join(bad)
    # b. wiring
    bad = (pix2pix_wiring if model == 'pix2pix' else cyclegan_wiring)(st, calls, dtype, opts)
    assert not bad, "wiring:\n" + '\n'.join(bad)
    # c. the captured graph against the serial order
    replay_(*replay_.inputs)
    graph = kept(st)
    assert np.isfinite(graph['losses'].cpu().numpy()).all()
    start()
    A.issue(calls)
    serial = kept(st)
    differ = [k for k in graph if A.bit_equal(serial[k], graph[k]) != 0.0]
    print(f"\n[{title}] graph against serial order: {len(graph)} tensors compared, " + (f"DIFFERENT: {differ}" if differ else "all bit-equal"))
    assert not differ, f"the captured graph and the serial order leave different bits in {differ}"
    del graph, serial
    # a. + d. the audit, pad channels before the first and after the last call
    start()
    bufs = image_buffers(st) + ([('aug_raw', st.aug_raw.t, 2 * ch)] if opts.get('diffaug') else [])
    assert {'g.dgen', 'g.dgen2', 'd.xin', 'd.dxin'} <= {b[0] for b in bufs} or model == 'cyclegan', [b[0] for b in bufs]
    before = A.pad_channels(bufs)
    if ctx.ls is not None:
        ls0 = ctx.ls.clone()
        masters = [n.params.master.clone() for n in st.nets()]
    steps0 = [int(n.params.step[0]) for n in st.nets()]
    t1 = time.time()
    del A.TIMES[:]
    rows = A.replay(calls, check=check)
    t2 = time.time()
    after = A.pad_channels(bufs)
    A.report(title, rows, t0, t1, t2)
    print(f"[{title}] reference + audit time {t2 - t1:.1f} s; slowest calls: " +
          ', '.join(f"{lab} ({nm[4:]}) {sec:.2f} s" for sec, lab, nm in sorted(A.TIMES, reverse=True)[:4]))
    print(f"[{title}] pad channels bit-zero before the first call: {not before}, after the last: {not after}")
    # exactly the calls of the predicate carry a ratio; every other call with a checker reads AS_ONE_GPU
    for c, r in zip(calls, rows):
        assert (r[4] is not None) == check(c), (r[0], c.name)
        assert r[4] is not None or c.name in A.ALLOWLIST or r[2] == A.AS_ONE_GPU, (r[0], c.name)
    want = expected_counts(model, opts)
    seen = {n: sum(1 for r in rows if r[1] == n and r[4]) for n in A.OPTION_ENTRIES}
    assert seen == {n: want.get(n, 0) for n in A.OPTION_ENTRIES}, f"checked option calls {seen}, expected {want}"
    convs = [r for c, r in zip(calls, rows) if r[4] is not None and c.name not in A.OPTION_ENTRIES]
    if opts.get('diffaug'):
        assert [r[1] for r in convs] == ['gan_conv2d_dgrad'] and 'D.down0' in convs[0][0], [r[:2] for r in convs]
    if opts.get('pools'):
        fwd = [r for r in convs if r[1] == 'gan_conv2d_fwd']
        assert len(fwd) >= 10 and any(r[1] == 'gan_conv_wgrad' for r in convs), [r[:2] for r in convs]
        traces = [c.trace[0][0] for c in calls if c.name == 'gan_pool_exchange']
        assert sorted(traces) == ['keep', 'swap'], traces
    if not opts.get('diffaug') and not opts.get('pools'):
        assert not convs
    if msssim:
        (ms,) = [r[4] for r in rows if r[1] == 'gan_msssim']
        print(f"[{title}] gan_msssim at amplitude {NEAR_AMP}: smallest factor of the reference {A.MSSSIM_PREMISE / ms['premise']:.3f}; error / gate " +
              ', '.join(f"{k} {v:.3f}" for k, v in ms.items()))
        assert set(ms) == {'premise', 'da', 'loss', 'da untouched outside the view'}
    assert not before and not after, f"pad channels: before the first call {before}, after the last {after}"
    bad = A.failures(rows)
    assert not bad, "calls outside their gates:\n" + '\n'.join(f"  {b}" for b in bad[:40])
    assert np.isfinite(st.losses.cpu().numpy()).all()
    for net, s0 in zip(st.nets(), steps0):
        assert int(net.params.step[0]) == s0 + 1
    if opts.get('lr_schedule'):
        ds, de, ef = opts['lr_schedule']
        assert steps0 == [A.SCHED_STEP0] * len(steps0)
        assert all(st.current_lr(i) == float(np.float32(np.float32(st.lr) * 0.5)) for i in range(len(steps0)))
    # e. f16: a finite, applied step (tests/test_gpu_wide_audit.py)
    if dtype == 'f16':
        ls1 = ctx.ls.cpu()
        print(f"[{title}] loss-scale state before {ls0.tolist()} after {ls1.tolist()}")
        assert float(ls1[0]) == float(ls0[0]) and float(ls1[1]) == float(ls0[1]) and float(ls1[3]) == 0.0
        assert float(ls1[2]) == float(ls0[2]) + 1.0
        for net, p0 in zip(st.nets(), masters):
            assert bool(torch.isfinite(net.params.master).all()) and not torch.equal(net.params.master, p0)
    else:
        assert ctx.ls is None
