"""The launch audit (tests/launch_audit.py) beyond the sweep of tests/test_gpu_launch_audit.py: fp32, CycleGAN at 512x512 and the
batches above B = 16 (256x256) / 8 (512x512).  The steps are built, captured, reset and fed as there (launch_audit.captured_step);
checkers and gates are the same, unchanged.  tests/test_cpu_launch_audit.py holds the tables (WIDE_SWEEP, WIDE_FULL, WIDE_CLASS) and
asserts on the host planners that these cases, with the one-GPU audit's, reach every (dtype family, plan class) of the wide sweeps.

Full audits (WIDE_FULL): every launch of CycleGAN 256x256 B = 1 at f16 - the loss-scaled InstanceNorm chain, gan_grads_check and
gan_loss_scale_update in the capture, the scale state after the replay - and at fp32.

Class audits (WIDE_CLASS): only the conv / wgrad calls whose class no earlier case of the dtype family has audited are checked
(launch_audit.outside_classes), which keeps the fp64 reference to a handful of launches even at 512x512 B = 9 or 256x256 B = 49.
Every unchecked conv / wgrad call must be of a class the host table gives an earlier case, the classes the case was added for must
be among its checked rows (launch_audit.missing_classes), and the classes the case recorded must be the host table's for its batch,
no more and no fewer - so the table cannot credit a batch with a class its step does not launch."""
import time

import numpy as np
import pytest
import torch

from tests import launch_audit as A
from tests.test_cpu_launch_audit import (FAMILY, WIDE_FULL, wide_audited, wide_class_cases, wide_classes, wide_earlier,
                                         wide_new_classes)

pytestmark = pytest.mark.gpu

ID = "{0}-{1}-{2}-B{3}".format


def recorded_classes(calls):
    return {k for k in map(A.call_class, calls) if k is not None}


def table_failures(case, calls):
    """The classes the captured step recorded against the host table of its batch (both directions)."""
    rec, tab = recorded_classes(calls), wide_classes(*case[:3], case[3])
    return [f"recorded, not in the host table: {k}" for k in sorted(rec - set(tab), key=str)] + \
        [f"in the host table ({tab[k]}), not recorded: {k}" for k in sorted(set(tab) - rec, key=str)]


@pytest.mark.parametrize("model,dtype,size,batch", WIDE_FULL, ids=[ID(*c) for c in WIDE_FULL])
def test_every_launch_of_the_cyclegan_step_against_fp64(model, dtype, size, batch, monkeypatch):
    t0 = time.time()
    st, calls, replay = A.captured_step(model, dtype, size, batch, monkeypatch)
    ctx = st.ctx
    names = {c.name for c in calls}
    if dtype == 'f16':
        assert ctx.ls is not None and {'gan_grads_check', 'gan_loss_scale_update'} <= names, sorted(names)
        ls0 = ctx.ls.clone()
        masters = [n.params.master.clone() for n in st.nets()]
    else:
        assert ctx.ls is None and not {'gan_grads_check', 'gan_loss_scale_update'} & names
    t1 = time.time()
    rows = A.replay(calls)
    t2 = time.time()
    A.report(f"wide, full: {model} {dtype} {size}x{size} B={batch}", rows, t0, t1, t2)
    # every recorded entry point has a checker or an ALLOWLIST entry (replay raises otherwise); every call with a checker was checked
    assert all(r[4] is not None for c, r in zip(calls, rows) if c.name in A.CHECKERS)
    assert all(c.name in A.ALLOWLIST for c, r in zip(calls, rows) if r[4] is None)
    assert any(r[1] == 'gan_conv_wgrad' for r in rows) and any(r[1].startswith('gan_norm_act_bwd') for r in rows)
    bad = table_failures((model, dtype, size, batch), calls)
    assert not bad, "plan classes:\n" + '\n'.join(bad)
    bad = A.failures(rows)
    assert not bad, "calls outside their gates:\n" + '\n'.join(f"  {b}" for b in bad[:40])
    assert np.isfinite(st.losses.cpu().numpy()).all()
    if dtype == 'f16':
        # a finite, applied step: the scale kept, one more finite step counted, the flag clear, every network one step on
        ls1 = ctx.ls.cpu()
        print(f"loss-scale state before {ls0.tolist()} after {ls1.tolist()}")
        assert float(ls1[0]) == float(ls0[0]) and float(ls1[1]) == float(ls0[1]) and float(ls1[3]) == 0.0
        assert float(ls1[2]) == float(ls0[2]) + 1.0
        for net, p0 in zip(st.nets(), masters):
            P = net.params
            assert int(P.step[0]) == 1 and bool(torch.isfinite(P.master).all()) and not torch.equal(P.master, p0)


CLASS_CASES = wide_class_cases()


@pytest.mark.parametrize("model,dtype,size,batch", CLASS_CASES, ids=[ID(*c) for c in CLASS_CASES])
def test_launches_of_unaudited_plan_classes_against_fp64(model, dtype, size, batch, monkeypatch):
    case = (model, dtype, size, batch)
    family = FAMILY[dtype]
    audited = wide_audited(wide_earlier() + CLASS_CASES[:CLASS_CASES.index(case)], family)
    new = wide_new_classes(case)
    assert new and not set(new) & audited
    t0 = time.time()
    st, calls, replay = A.captured_step(model, dtype, size, batch, monkeypatch)
    t1 = time.time()
    del A.TIMES[:]
    rows = A.replay(calls, check=A.outside_classes(audited))
    t2 = time.time()
    title = f"wide, classes: {model} {dtype} {size}x{size} B={batch}"
    A.report(title, rows, t0, t1, t2)
    print(f"[{title}] added for: " + '; '.join(f"{tag} {k}" for k, tag in sorted(new.items(), key=str)))
    print(f"[{title}] slowest calls: " + ', '.join(f"{lab} {sec:.2f} s" for sec, lab, _ in sorted(A.TIMES, reverse=True)[:3]))
    # the step launches the classes of the host table for this batch, no more and no fewer
    bad = table_failures(case, calls)
    assert not bad, "plan classes:\n" + '\n'.join(bad)
    # every unchecked conv / wgrad call is of a class an earlier case of the family audited; every checked one is not
    for c, r in zip(calls, rows):
        k = A.call_class(c)
        if k is not None:
            assert (r[4] is None) == (k in audited), (r[0], c.name, k)
            assert r[4] is not None or r[2] == A.AS_ONE_GPU
        else:
            assert r[4] is None
    # what the case was added for is among the checked rows
    miss = A.missing_classes(calls, rows, new)
    assert not miss, "classes this case was added for, not checked:\n" + '\n'.join(miss)
    assert {A.call_class(c) for c, r in zip(calls, rows) if r[4] is not None} == set(new)
    bad = A.failures(rows)
    assert not bad, "calls outside their gates:\n" + '\n'.join(f"  {b}" for b in bad[:40])
    assert np.isfinite(st.losses.cpu().numpy()).all()
