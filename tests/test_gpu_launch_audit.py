"""Every library call of the captured training step, at the shapes and with the descriptors the step builds itself, checked on
its own against an fp64 reference of the values it read (tests/launch_audit.py): per-element gates near one output ulp instead of
the step-level cosine / agreement gates of test_gpu_golden_full.py, and every kernel / fusion the planner picks for these batch
sizes - the partial batches of an epoch included (gan_amd/data.py keeps the last one; Pix2Pix._step_for captures a step per batch
size) - is reached, for steps built at channels = 1.  AUDIT_CASES is the batch list; tests/test_cpu_launch_audit.py asserts on the
host planners alone that it reaches every plan class of B = 1..16 at 256x256 and B = 1..8 at 512x512 at 16-bit storage (Pix2Pix at
both sizes, CycleGAN at 256x256).  fp32 beyond the one case here, CycleGAN at 512x512 and the larger batches (to 64 at 256x256, 16 at
512x512) are tests/test_gpu_wide_audit.py's: it replays the same captured steps (launch_audit.captured_step) and checks the launches
of the plan classes that no case here reaches, per dtype family.  At channels = 3 the
image-side layers leave the one-kernel thin-N form for conv_thin_n_kernel + conv_thin_col2im_kernel, which no case here launches:
tests/test_gpu_rgb_audit.py audits the launches that depend on the channel count.  Every step here is built without options:
the launches of gan_dssim, gan_msssim, gan_edge_l1, gan_diffaug_draw / gan_diffaug_apply, gan_lsq_logits / gan_patchgan_losses_lsq,
gan_pool_exchange and gan_adam_begin_sched inside the option-carrying captured steps are tests/test_gpu_option_audit.py's (their
device-free compare functions: tests/test_cpu_option_audit.py)."""
import time

import numpy as np
import pytest

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


_reset = A.reset_step             # (tests/test_gpu_rgb_audit.py and tests/test_gpu_ddp_audit.py build their own steps and reset them with it)


@pytest.mark.parametrize("model,dtype,size,batch", AUDIT_CASES, ids=[f"{m}-{d}-{s}-B{b}" for m, d, s, b in AUDIT_CASES])
def test_every_launch_of_the_captured_step_against_fp64(model, dtype, size, batch, monkeypatch):
    t0 = time.time()
    st, calls, replay = A.captured_step(model, dtype, size, batch, monkeypatch)      # (shared with tests/test_gpu_wide_audit.py)
    t1 = time.time()
    rows = A.replay(calls)
    t2 = time.time()
    A.report(f"{model} {dtype} {size}x{size} B={batch}", rows, t0, t1, t2)
    assert any(r[4] is not None for r in rows if r[1] == 'gan_conv_wgrad')
    bad = A.failures(rows)
    assert not bad, "calls outside their gates:\n" + '\n'.join(f"  {b}" for b in bad[:40])
    assert np.isfinite(st.losses.cpu().numpy()).all()
