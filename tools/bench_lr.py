#!/usr/bin/env python3
"""The captured training step with a learning-rate schedule beside the constant rate: Pix2Pix bf16 256^2 at
--p2p-batch and CycleGAN bf16 256^2 at --cyc-batch, same seeds and inputs; the schedule exchanges one single-thread launch per network
(gan_adam_begin -> gan_adam_begin_sched) and nothing else.

    python tools/bench_lr.py [--min-seconds 1.0] [--repeats 2] [--configs off,on] [--tree DIR] [--parent-json FILE ...] [--from-json FILE] [--out FILE]

Every point: warm-up, then HIP events around as many back-to-back replays as fill --min-seconds (tools/bench_infer.py's `timed`),
the configurations interleaved, --repeats windows each.  'on' is a schedule in its decaying part from the first update (0 .. 2^30, so
the rate hardly moves during the measurement).  --configs off touches nothing this feature added, so the same script measures the parent
commit: --tree names the checkout to import gan_amd from (default: this one).  --parent-json: the output of such a run; it is merged
in (several files: pooled) with the parent's own run-to-run spread next to the differences; --from-json FILE merges into an earlier output of this
tool instead of measuring (parent runs taken before AND after this commit's).  Prints one JSON object; --out also saves it
(profiles/bench_lr.json).  Reported, not gated."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summarise(res, parent):
    """Differences of the medians against the parent's 'off' windows, with the parent's spread (max - min) beside them."""
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
    res['parent'] = {k: parent[k] for k in ('tree', 'pix2pix', 'cyclegan') if k in parent}
    out = res['summary'] = {}
    for model in ('pix2pix', 'cyclegan'):
        p = parent[model]['off_ms']
        s = out[model] = {'parent_off_median_ms': med(p), 'parent_spread_ms': max(p) - min(p),
                          'parent_spread_percent': 100.0 * (max(p) - min(p)) / med(p)}
        for kind in ('off', 'on'):
            if kind + '_ms' in res[model]:
                m = med(res[model][kind + '_ms'])
                s[kind + '_median_ms'] = m
                s[kind + '_vs_parent_percent'] = 100.0 * (m - med(p)) / med(p)
        if 'on_median_ms' in s and 'off_median_ms' in s:
            s['on_vs_off_percent'] = 100.0 * (s['on_median_ms'] - s['off_median_ms']) / s['off_median_ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--configs', default='off,on')
    ap.add_argument('--p2p-batch', type=int, default=16)
    ap.add_argument('--cyc-batch', type=int, default=1)
    ap.add_argument('--tree', default=HERE)
    ap.add_argument('--parent-json', nargs='+', default=None)
    ap.add_argument('--from-json', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.from_json:                   # an earlier output of this tool: nothing is measured, --parent-json is merged into it
        res = json.loads(open(a.from_json).read())
        finish(a, res)
        return
    root = os.path.abspath(a.tree)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'tools'))
    import torch
    from bench_infer import timed
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep, Pix2PixStep
    configs = [c for c in a.configs.split(',') if c]
    assert configs and set(configs) <= {'off', 'on'}, a.configs
    assert torch.cuda.is_available(), "bench_lr.py needs an MI355X"
    res = {'tool': 'bench_lr', 'tree': 'this checkout' if root == HERE else 'the checkout given by --tree', 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
           'dtype': 'bf16', 'size': 256, 'unit': 'ms per replayed step'}
    for model, B in (('pix2pix', a.p2p_batch), ('cyclegan', a.cyc_batch)):
        ctx = Ctx('cuda:0', 'bf16')
        x, y = (torch.rand(B, 256, 256, 1, device=ctx.device) * 2 - 1 for _ in range(2))
        point = res[model] = {'batch': B}
        for kind in configs * a.repeats:
            kw = {}
            if kind == 'on':
                from gan_amd.nets import LrSchedule
                kw['lr_schedule'] = LrSchedule(2e-4, 0.0, 0, 1 << 30)
            if model == 'pix2pix':
                st = Pix2PixStep(ctx, B, 256, 1, lam=100.0, seed=123, **kw)
            else:
                st = CycleGANStep(ctx, B, 256, 1, lam=10.0, seed=123, **kw)
            replay = st.capture(training=True)
            ms, n = timed(lambda: replay(x, y), a.min_seconds)
            point.setdefault(kind + '_ms', []).append(ms)
            point.setdefault(kind + '_losses', []).append([float(v) for v in st.losses[:4].cpu()])
            if kind == 'on':
                point['on_current_lr'] = st.current_lr()
            del st, replay
            torch.cuda.empty_cache()
        del ctx
    finish(a, res)


def finish(a, res):
    if a.parent_json:
        runs = [json.loads(open(p).read()) for p in a.parent_json]       # (several runs, e.g. one before and one after: pooled)
        parent = {'tree': runs[0]['tree']}
        for model in ('pix2pix', 'cyclegan'):
            parent[model] = {'batch': runs[0][model]['batch'], 'off_ms': [ms for r in runs for ms in r[model]['off_ms']]}
        summarise(res, parent)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
