"""Every library call of the captured training step, at the shapes and with the descriptors the step builds itself, checked on
its own against an fp64 reference of the values it read (tests/launch_audit.py): per-element gates near one output ulp instead of
the step-level cosine / agreement gates of test_gpu_golden_full.py, and every kernel / fusion the planner picks for these batch
sizes - the partial batches of an epoch included (gan_amd/data.py keeps the last one; Pix2Pix._step_for captures a step per batch
size) - is reached, for steps built at channels = 1.  AUDIT_CASES is the batch list; tests/test_cpu_launch_audit.py asserts on the
host planners alone that it reaches every plan class of B = 1..16 at 256x256 and B = 1..8 at 512x512.  At channels = 3 the
image-side layers leave the one-kernel thin-N form for conv_thin_n_kernel + conv_thin_col2im_kernel, which no case here launches:
tests/test_gpu_rgb_audit.py audits the launches that depend on the channel count."""
import gc
import time

import numpy as np
import pytest
import torch

from tests import launch_audit as A
from tests.test_cpu_launch_audit import AUDITED

pytestmark = pytest.mark.gpu

# (model, dtype, size, batch).  The 16-bit batches are tests/test_cpu_launch_audit.py::AUDITED, which that test checks against the
# plan classes of B = 1..16 at 256x256 (1..8 at 512x512).  Pix2Pix 256: B = 16 is the object bench.py times (GanAdamFuse, lanes, the
# alternate wgrad lane), B = 1 the CLI default, B = 3, 5, 9 the partial batches the planner sweep named (D's stride-1 conv on tap-shared
# split-K tiles without fused statistics; on 256x256 tiles at 9) and B = 8 the two classes no other of them reaches.  512: B = 3, 5
# named by the sweep, B = 1, 6 for the rest.  CycleGAN: B = 4 (BASELINE config 3) and the smallest set of others that covers every
# class (1, 9, 15).  Trade-off: covering every class costs about 11 minutes of fp64 reference on 16 CPUs, not the 6 first budgeted;
# the reference is the cost (the GPU work of a case is under a second).
AUDIT_CASES = [(m, 'bf16', s, b) for (m, s), bs in AUDITED.items() for b in bs] + [
    ('pix2pix', 'f16', 256, 16),      # loss scaling, the unfused Adam path
    ('pix2pix', 'f32', 256, 2),       # exact-MFMA kernels
]


def _reset(step, saved):
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


@pytest.mark.parametrize("model,dtype,size,batch", AUDIT_CASES, ids=[f"{m}-{d}-{s}-B{b}" for m, d, s, b in AUDIT_CASES])
def test_every_launch_of_the_captured_step_against_fp64(model, dtype, size, batch, monkeypatch):
    from gan_amd.nets import Ctx, workspace_mb_for
    from gan_amd.steps import CycleGANStep, Pix2PixStep
    # the graphs and events of the previous case must be gone before this one captures: destroying them inside a capture (a cyclic
    # garbage collection run at an allocation) aborts the process
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.time()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    rec = A.Recorder(monkeypatch)                 # before the step object: its op lists hold the bound entry points
    rec.hook_capture(monkeypatch)
    ctx = Ctx('cuda:0', dtype, workspace_mb=workspace_mb_for(batch, size))
    if model == 'pix2pix':
        st = Pix2PixStep(ctx, batch, size, 1, lam=100.0, seed=123)
    else:
        st = CycleGANStep(ctx, batch, size, 1, lam=10.0, seed=123)
    saved = [(n.params.master.clone(), {k: t.clone() for k, t in n.params.state.items()}) for n in st.nets()]
    replay = st.capture(training=True)            # what bench.py captures
    torch.cuda.synchronize()
    calls = rec.calls
    assert calls, "nothing recorded inside the capture body"
    A.label_calls(calls, st)
    # known start: initial weights, step 0, small random moments (_reset); inputs on the normalize() lattice (base_gan.py:56-61)
    _reset(st, saved)
    g = torch.Generator().manual_seed(7 + batch)
    for t in replay.inputs:
        t.copy_((torch.randint(0, 256, tuple(t.shape), generator=g).float() / 127.5 - 1.0).to(t.device))
    torch.cuda.synchronize()
    t1 = time.time()
    rows = A.replay(calls)
    t2 = time.time()
    title = f"{model} {dtype} {size}x{size} B={batch}"
    print('\n' + A.table(rows, title))
    worst = A.worst_per_entry(rows)
    print(f"[{title}] worst error/gate per entry point: " + ', '.join(f"{k[4:]} {v:.3f}" for k, v in sorted(worst.items())))
    print(f"[{title}] {len(rows)} calls ({sum(r[4] is not None for r in rows)} checked); "
          f"build + capture {t1 - t0:.1f} s, audit {t2 - t1:.1f} s")
    assert any(r[4] is not None for r in rows if r[1] == 'gan_conv_wgrad')
    bad = A.failures(rows)
    assert not bad, "calls outside their gates:\n" + '\n'.join(f"  {b}" for b in bad[:40])
    assert np.isfinite(st.losses.cpu().numpy()).all()
