#!/usr/bin/env python3
"""The captured CycleGAN step with image history pools beside the step without: bf16 256^2 at --batches,
same seeds and inputs.  With pools each discriminator call grows from two invocations to three and each chain gains one launch
(gan_pool_exchange).

    python tools/bench_pool.py [--min-seconds 1.0] [--repeats 3] [--configs off,on,parts] [--batches 1,4] [--tree DIR]
                               [--parent-json FILE ...] [--from-json FILE] [--out FILE]

Every point: warm-up, then HIP events around as many back-to-back replays as fill --min-seconds (tools/bench_infer.py's `timed`), the
configurations interleaved, --repeats windows each.
  off    pools=None (the argument is not passed at all: the same script measures the parent commit with --configs off --tree DIR)
  on     pools of 50, filled before the measurement
  parts  what `on` adds, each piece alone as a captured graph of 20 repetitions: the discriminator forward of three invocations
         against two (the same launches, larger), and gan_pool_exchange at B = 1, 4, 16 on a full pool of 50
--parent-json: the output of --configs off runs of the parent (several files: pooled); merged in with the parent's own run-to-run
spread next to the differences.  --from-json FILE merges into an earlier output of this tool instead of measuring.  Prints one JSON
object; --out also saves it (profiles/bench_pool.json).  Reported, not gated."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH_US = 3.0          # the project's measured cost of one more launch on a chain
REPS = 20                # repetitions inside one captured graph of a part: the graph launch itself is amortised


def med(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def summarise(res, parent):
    out = res['summary'] = {}
    for key, point in res['steps'].items():
        s = out[key] = {}
        if parent is not None and key in parent:
            p = parent[key]
            s.update(parent_off_median_ms=med(p), parent_windows=len(p), parent_spread_ms=max(p) - min(p),
                     parent_spread_percent=100.0 * (max(p) - min(p)) / med(p))
        if 'off_ms' in point:
            s['off_median_ms'] = med(point['off_ms'])
            if 'parent_off_median_ms' in s:
                s['off_vs_parent_ms'] = s['off_median_ms'] - s['parent_off_median_ms']
                s['off_within_parent_spread'] = bool(min(p) <= s['off_median_ms'] <= max(p))
        if 'on_ms' in point and 'off_ms' in point:
            s['on_median_ms'] = med(point['on_ms'])
            s['on_minus_off_us'] = 1e3 * (s['on_median_ms'] - s['off_median_ms'])
            s['on_vs_off_percent'] = 100.0 * (s['on_median_ms'] - s['off_median_ms']) / s['off_median_ms']
        parts = res.get('parts', {}).get(key)
        if parts and 'on_minus_off_us' in s:
            # per chain: the larger discriminator forward + the exchange + one launch; the two chains run on two lanes, so the step
            # pays between one chain's sum (perfect overlap) and both (none)
            chain = parts['disc_forward_3_minus_2_us'] + parts['exchange_us'] + LAUNCH_US
            s.update(added_per_chain_us=chain, added_both_chains_us=2 * chain,
                     measured_over_both_chains=s['on_minus_off_us'] / (2 * chain))


def parts_of(torch, timed, min_s, B):
    """The pieces `on` adds, alone: microseconds per repetition."""
    from gan_amd.nets import Ctx, DiscriminatorNet
    ctx = Ctx('cuda:0', 'bf16', lanes=False)
    net = DiscriminatorNet(ctx, 1, False, 'instancenorm')
    out = {}

    def graph_us(fn):
        fn()
        torch.cuda.synchronize()
        g = ctx.capture_graph(lambda: [fn() for _ in range(REPS)])
        ms, _ = timed(g.replay, min_s)
        return 1e3 * ms / REPS
    for calls in (2, 3):
        dc = net.new_call(B, 256, calls=calls, param_calls=2)
        dc.xin.t.uniform_(-1, 1)
        out[f'disc_forward_{calls}_us'] = graph_us(dc.forward)
        del dc
    out['disc_forward_3_minus_2_us'] = out['disc_forward_3_us'] - out['disc_forward_2_us']
    del net, ctx
    out['exchange_us'] = parts_of_exchange(torch, timed, min_s, B)
    out['exchange_bytes_moved_at_most'] = 3 * B * 256 * 256 * 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--configs', default='off,on,parts')
    ap.add_argument('--batches', default='1,4')
    ap.add_argument('--tree', default=HERE)
    ap.add_argument('--parent-json', nargs='+', default=None)
    ap.add_argument('--from-json', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.from_json:
        finish(a, json.loads(open(a.from_json).read()))
        return
    root = os.path.abspath(a.tree)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'tools'))
    import torch
    from bench_infer import timed
    from gan_amd.nets import Ctx
    from gan_amd.steps import CycleGANStep
    configs = [c for c in a.configs.split(',') if c]
    assert configs and set(configs) <= {'off', 'on', 'parts'}, a.configs
    assert torch.cuda.is_available(), "bench_pool.py needs an MI355X"
    res = {'tool': 'bench_pool', 'tree': 'this checkout' if root == HERE else 'the checkout given by --tree', 'min_seconds': a.min_seconds,
           'device': torch.cuda.get_device_name(0), 'model': 'cyclegan', 'dtype': 'bf16', 'size': 256, 'unit': 'ms per replayed step',
           'launch_us': LAUNCH_US, 'steps': {}, 'parts': {}}
    for B in [int(b) for b in a.batches.split(',')]:
        key = f'batch{B}'
        ctx = Ctx('cuda:0', 'bf16')
        x, y = (torch.rand(B, 256, 256, 1, device=ctx.device) * 2 - 1 for _ in range(2))
        point = res['steps'][key] = {'batch': B}
        for kind in [c for c in configs if c != 'parts'] * a.repeats:
            kw = {}
            if kind == 'on':
                from gan_amd.pool import ImagePool
                kw['pools'] = tuple(ImagePool(ctx, 256, 1, 50, 123, sid) for sid in (32, 33))
            st = CycleGANStep(ctx, B, 256, 1, lam=10.0, seed=123, **kw)
            replay = st.capture(training=True)
            if kind == 'on':
                for _ in range(-(-50 // B)):        # fill the pools: the measured steps swap and keep
                    replay(x, y)
                torch.cuda.synchronize()
                assert all(p.state[0].item() == 50 for p in kw['pools'])
            ms, n = timed(lambda: replay(x, y), a.min_seconds)
            point.setdefault(kind + '_ms', []).append(ms)
            del st, replay, kw
            torch.cuda.empty_cache()
        del ctx
        if 'parts' in configs:
            res['parts'][key] = parts_of(torch, timed, min(a.min_seconds, 0.3), B)
    if 'parts' in configs:
        res['exchange_alone_us'] = {f'batch{B}': parts_of_exchange(torch, timed, min(a.min_seconds, 0.3), B) for B in (1, 4, 16)}
    finish(a, res)


def parts_of_exchange(torch, timed, min_s, B):
    from gan_amd import _lib as L
    from gan_amd.nets import Ctx
    from gan_amd.pool import ImagePool
    ctx = Ctx('cuda:0', 'bf16', lanes=False)
    pool = ImagePool(ctx, 256, 1, 50, 123, 32)
    pool.state[0] = 50
    src = torch.empty(B, 256, 256, 8, dtype=ctx.tdtype, device=ctx.device).uniform_(-1, 1)
    dst = torch.zeros_like(src)
    view = lambda t: L.GanTensor(t.data_ptr(), B, 256, 256, 1, 8)
    fn = lambda: pool.exchange(view(src), view(dst))
    fn()
    torch.cuda.synchronize()
    g = ctx.capture_graph(lambda: [fn() for _ in range(REPS)])
    ms, _ = timed(g.replay, min_s)
    return 1e3 * ms / REPS


def finish(a, res):
    parent = None
    if a.parent_json:
        runs = [json.loads(open(p).read()) for p in a.parent_json]
        parent = {}
        for r in runs:
            for key, point in r['steps'].items():
                parent.setdefault(key, []).extend(point['off_ms'])
        res['parent'] = {'tree': runs[0]['tree'], 'off_ms': parent}
    summarise(res, parent)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
