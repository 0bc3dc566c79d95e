"""Every launch of the data-parallel training step that the one-GPU audit does not already cover, per element against fp64
(tests/launch_audit.py), in ONE process: the gradient exchange is launch_audit.identity_sync - world 2, real pack / unpack kernels,
an exchange that does nothing - so the "sum over ranks" is this rank's own wire contents and Adam's 1/world halves every update.

Per case: the data-parallel step is captured (recorded per graph) and a one-GPU step of the same model, dtype and batch beside it,
whose (entry point, plan string) pairs come from the host queries alone (it is never replayed).  Replay order, as the schedule's
replayer runs its graphs on the data they depend on: the compute graphs' calls in capture order - bucketed G1..G4 with their
gan_grad_pack launches inside, phased one graph per phase with the eager gan_grad_pack of the networks a phase completes behind
it - then (fp16, bf16 wire without wire Adam) the eager gan_grad_unpack calls, then the Adam graphs' calls in capture order.  (The
product replays an Adam graph as soon as its bucket has landed, beside the later compute graphs, which read none of the weights it
rewrites; issuing them afterwards changes no value.)  The wire buffers hold a NaN sentinel before the compute calls.
Checked: every gan_conv_wgrad (dw_wire launches against the wire gate, the wire buffers whole), every gan_bias_grad, every
gan_grad_pack's range, every call whose (entry point, plan string) the one-GPU capture does not hold; the rest is issued
unchecked and printed "as in the one-GPU step".  After the compute calls: every element of every real extent of the wire buffers
written exactly once.  After the Adam calls: launch_audit.AdamEnd.  The case's wgrad plan strings must be those of
tests/test_cpu_launch_audit.py's table (DDP_CASES, whose batches its sweep chose)."""
import gc
import time

import numpy as np
import pytest
import torch

from tests import launch_audit as A
from tests.test_cpu_launch_audit import DDP_CASES, ddp_wgrad_plan_strings
from tests.test_gpu_launch_audit import _reset

pytestmark = pytest.mark.gpu

# what each case of DDP_CASES sets on the step / the exchange: (compress, attributes of the step)
SETUP = {
    'pix2pix-bf16-bucketed-wire-direct': (True, {}),
    'pix2pix-bf16-bucketed-wire-pack': (True, {'ddp_wire_direct': False}),
    'pix2pix-bf16-bucketed-fp32-wire': (False, {}),
    'pix2pix-f16-phased': (True, {}),
    'cyclegan-bf16-phased-wire': (True, {}),
    'pix2pix-bf16-phased-wire': (True, {'ddp_buckets': False}),
}
CASES = [(name, b) for name, (_, _, _, bs) in DDP_CASES.items() for b in bs]


def _build(model, ctx, batch):
    from gan_amd.steps import CycleGANStep, Pix2PixStep
    if model == 'pix2pix':
        return Pix2PixStep(ctx, batch, 256, 1, lam=100.0, seed=123)
    return CycleGANStep(ctx, batch, 256, 1, lam=10.0, seed=123)


@pytest.mark.parametrize("name,batch", CASES, ids=[f"{n}-B{b}" for n, b in CASES])
def test_every_launch_of_the_data_parallel_step_against_fp64(name, batch, monkeypatch):
    from gan_amd.nets import Ctx, workspace_mb_for
    model, dtype, tab, _ = DDP_CASES[name]
    compress, attrs = SETUP[name]
    gc.collect()                                  # (graphs of the previous case: see test_gpu_launch_audit.py)
    torch.cuda.synchronize()
    t0 = time.time()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    rec = A.Recorder(monkeypatch)
    rec.hook_capture(monkeypatch)
    # the one-GPU step of the same model, dtype and batch: captured for its plan strings, never replayed
    one = _build(model, Ctx('cuda:0', dtype, workspace_mb=workspace_mb_for(batch, 256)), batch)
    one.capture(training=True)
    torch.cuda.synchronize()
    n_one = len(rec.calls)
    known = {(c.name, A.plan_of(c)) for c in rec.calls}
    assert any(nm == 'gan_conv2d_fwd' for nm, _ in known)
    # the data-parallel step
    st = _build(model, Ctx('cuda:0', dtype, workspace_mb=workspace_mb_for(batch, 256)), batch)
    for k, v in attrs.items():
        setattr(st, k, v)
    sync = st.sync = A.identity_sync(st, compress)
    assert sync.world == 2 and sync.active and sync.grad_scale == (1.0 if compress else 0.5)
    saved = [(n.params.master.clone(), {k: t.clone() for k, t in n.params.state.items()}) for n in st.nets()]
    g0 = len(rec.graph_starts)
    replay = st.capture(training=True)
    torch.cuda.synchronize()
    starts = rec.graph_starts[g0:] + [len(rec.calls)]
    graphs = [rec.calls[a:b] for a, b in zip(starts[:-1], starts[1:])]
    bucketed = hasattr(st, 'buckets')
    assert bucketed == (model == 'pix2pix' and dtype == 'bf16' and attrs.get('ddp_buckets', True))
    if bucketed:                                  # G1..G4 | A0..A2 (G's segments), A3 (D)
        assert len(graphs) == 8
        compute, adam = sum(graphs[:4], []), sum(graphs[4:], [])
    else:                                         # a graph per phase, each followed by the pack of what it completes | unpack, Adam
        phases = st.ddp_phases()
        n_adam = 1 if dtype == 'f16' else len(st.nets())
        assert len(graphs) == len(phases) + n_adam
        compute, adam = [], []
        for (pid, done), gcalls in zip(phases, graphs):
            compute += gcalls
            for i in done:
                k0 = len(rec.calls)
                with rec.recording():
                    sync.pack(i)
                compute += rec.calls[k0:]
        if not st._wire_adam():
            for i in range(len(st.nets())):
                k0 = len(rec.calls)
                with rec.recording():
                    sync.unpack(i)
                adam += rec.calls[k0:]
        adam += sum(graphs[len(phases):], [])
    torch.cuda.synchronize()
    assert compute and adam and not any(c.name.startswith('gan_adam') for c in compute)
    assert not any(c.name in ('gan_conv_wgrad', 'gan_grad_pack') for c in adam)
    A.label_calls(compute + adam, st)
    _reset(st, saved)                             # initial weights, step 0, small NON-ZERO moments: they stay
    g = torch.Generator().manual_seed(7 + batch)
    for t in replay.inputs:
        t.copy_((torch.randint(0, 256, tuple(t.shape), generator=g).float() / 127.5 - 1.0).to(t.device))
    wa = A.WireAudit(st, sync) if compress else None
    if wa is not None:
        wa.fill()
    torch.cuda.synchronize()
    t1 = time.time()
    del A.TIMES[:]

    def check(c):
        return c.name in ('gan_conv_wgrad', 'gan_bias_grad') or (c.name, A.plan_of(c)) not in known
    rows = A.replay(compute, check=check, wire=wa)
    t2 = time.time()
    cover = wa.coverage() if wa is not None else []
    end = A.AdamEnd(st, sync)
    end.snapshot()
    rows += A.replay(adam, check=check)
    rows += end.check()
    t3 = time.time()
    title = f"{name} 256x256 B={batch}"
    print('\n' + A.table(rows, title))
    worst = A.worst_per_entry(rows)
    print(f"[{title}] worst error/gate per entry point: " + ', '.join(f"{k[4:]} {v:.3f}" for k, v in sorted(worst.items())))
    for nm in ('gan_conv_wgrad', 'gan_grad_pack', 'gan_adam (whole network)'):
        if A.worst_per_item(rows, nm):
            print(f"[{title}] {nm[4:]}: " + ', '.join(f"{k} {v:.3f}" for k, v in A.worst_per_item(rows, nm).items()))
    print(f"[{title}] slowest calls: " + ', '.join(f"{lab} {sec:.2f} s" for sec, lab, _ in sorted(A.TIMES, reverse=True)[:3]))
    checked = sum(r[4] is not None for r in rows)
    same = sum(r[2] == A.AS_ONE_GPU for r in rows)
    print(f"[{title}] {len(compute) + len(adam)} calls issued, {checked} checked, {same} as in the one-GPU step "
          f"({n_one} calls, {len(known)} plans), {len(rows) - checked - same} allowlisted; build + 2 captures {t1 - t0:.1f} s, "
          f"compute calls {t2 - t1:.1f} s, Adam calls + end check {t3 - t2:.1f} s")
    wg = [r for r in rows if r[1] == 'gan_conv_wgrad']
    assert wg and all(r[4] is not None for r in wg)
    seen = {r[2] for r in wg}
    want = ddp_wgrad_plan_strings(model, dtype, tab, batch)
    assert seen == want, f"wgrad plans differ from the table: only recorded {sorted(seen - want)}, only in the table {sorted(want - seen)}"
    direct = [r for r in wg if r[2].endswith(' wire')]
    assert bool(direct) == (tab == 'direct')
    if wa is not None:
        packs = [r for r in rows if r[1] == 'gan_grad_pack']
        assert packs and all(r[4] is not None for r in packs)
        assert not cover, "wire coverage:\n" + '\n'.join(cover)
    bad = A.failures(rows)
    assert not bad, "calls outside their gates:\n" + '\n'.join(f"  {b}" for b in bad[:40])
    assert np.isfinite(st.losses.cpu().numpy()).all()
