#!/usr/bin/env python3
"""The Sobel edge term: gan_edge_l1 beside the two secondary losses it joins, and the captured Pix2Pix step
with and without --edge-weight.

    python tools/bench_edge.py [--min-seconds 1.0] [--repeats 3] [--configs kernels,step] [--out FILE]

kernels  on the step's layout (bf16, pitch 8, one channel, the target at channel offset 1 of D's input): 256^2 batch 16.  gan_edge_l1
         (both launches, loss and gradient accumulating into da), gan_l1 and gan_dssim on the same views, each alone as a captured
         graph of REPS repetitions (the graph launch is amortised), HIP events around as many replays as fill --min-seconds;
         --repeats alternating rounds, medians.
step     the captured step at 256^2 bf16 batch 16, edge_weight 0 against 0.25, interleaved, --repeats windows each.
Prints one JSON object; --out also saves it (profiles/bench_edge.json).  Reported, not gated."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
W = 0.25


def med(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def kernels(torch, timed, min_s, repeats):
    import ctypes as C
    from gan_amd import _lib as L
    from gan_amd.nets import Buf, Ctx
    ctx = Ctx('cuda:0', 'bf16', lanes=False)
    lib = ctx.lib
    S, B, c, lam = 256, 16, 1, 100.0
    gen, xin, dgen = Buf(ctx, B, S, S, 8), Buf(ctx, 2 * B, S, S, 8), Buf(ctx, B, S, S, 8)
    for b in (gen, xin):
        b.t.uniform_(-1, 1)
    a, t, da = gen.view(0, c), xin.view(c, c, 0, B), dgen.view(0, c)
    loss = torch.zeros(4, device=ctx.device)
    ws_l1 = torch.zeros(4096, device=ctx.device)
    ws_d = torch.zeros(lib.gan_dssim_workspace_bytes(B, S, S, c) // 4, device=ctx.device)
    ws_e = torch.zeros(lib.gan_edge_workspace_bytes(B, S, S, c) // 4, device=ctx.device)
    dssim = L.GanDssimDesc(ctx.dt, ctx.dt, a, t, 1.0, 0, loss.data_ptr(), lam, ctx.dt, da, ws_d.data_ptr(), ws_d.numel() * 4, None)
    edge = L.GanEdgeDesc(ctx.dt, ctx.dt, a, t, W, 1, loss.data_ptr(), lam * W, ctx.dt, da, ws_e.data_ptr(), ws_e.numel() * 4, None, 1)
    edge_set = L.GanEdgeDesc(ctx.dt, ctx.dt, a, t, W, 0, loss.data_ptr(), lam * W, ctx.dt, da, ws_e.data_ptr(), ws_e.numel() * 4, None, 0)
    ops = {
        'gan_l1_us': lambda: L.check(lib.gan_l1(ctx.dt, C.byref(a), C.byref(t), 1.0, 0, loss.data_ptr(), lam, C.byref(da), ws_l1.data_ptr(),
                                                None, ctx.stream()), "l1"),
        'gan_dssim_us': lambda: L.check(lib.gan_dssim(C.byref(dssim), ctx.stream()), "dssim"),
        'gan_edge_l1_accumulate_us': lambda: L.check(lib.gan_edge_l1(C.byref(edge), ctx.stream()), "edge_l1"),
        'gan_edge_l1_set_us': lambda: L.check(lib.gan_edge_l1(C.byref(edge_set), ctx.stream()), "edge_l1"),
    }
    graphs = {}
    for k, fn in ops.items():
        fn()
        torch.cuda.synchronize()
        graphs[k] = ctx.capture_graph(lambda fn=fn: [fn() for _ in range(REPS)])
    runs = {k: [] for k in ops}
    for _ in range(repeats):                      # alternating: every op once per round
        for k, g in graphs.items():
            ms, _ = timed(g.replay, min_s)
            runs[k].append(1e3 * ms / REPS)
    pixels = B * S * S
    p = {'size': S, 'batch': B, 'channels': c, 'dtype': 'bf16', 'pitch': 8, 'runs_us': runs}
    p.update({k: med(v) for k, v in runs.items()})
    # what the launch has to move: a is one aligned 16-byte pixel (one load), the target and da are read / written by elements, and
    # every line they touch is a line of 16-byte pixels: a, b once and da read + written
    p['bytes_used'] = pixels * c * 2 * 4
    p['bytes_of_lines_touched'] = pixels * 16 * 4
    us = p['gan_edge_l1_accumulate_us']
    p['used_gb_per_s'] = p['bytes_used'] / us * 1e-3
    p['lines_gb_per_s'] = p['bytes_of_lines_touched'] / us * 1e-3
    p['edge_over_l1'] = us / p['gan_l1_us']
    p['edge_over_dssim'] = us / p['gan_dssim_us']
    return {f'{S}x{S}_batch{B}_c{c}': p}


def step(torch, timed, min_s, repeats):
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    B, S = 16, 256
    ctx = Ctx('cuda:0', 'bf16')
    x, y = (torch.rand(B, S, S, 1, device=ctx.device) * 2 - 1 for _ in range(2))
    point = {'batch': B, 'size': S, 'dtype': 'bf16', 'edge_weight': W, 'unit': 'ms per replayed step'}
    for kind in ['off', 'on'] * repeats:
        st = Pix2PixStep(ctx, B, S, 1, seed=123, edge_weight=W if kind == 'on' else 0.0)
        replay = st.capture(training=True)
        ms, _ = timed(lambda: replay(x, y), min_s)
        point.setdefault(kind + '_ms', []).append(ms)
        del st, replay
        torch.cuda.empty_cache()
    off, on = med(point['off_ms']), med(point['on_ms'])
    point.update(off_median_ms=off, on_median_ms=on, on_minus_off_us=1e3 * (on - off), on_vs_off_percent=100.0 * (on - off) / off,
                 off_spread_percent=100.0 * (max(point['off_ms']) - min(point['off_ms'])) / off,
                 off_images_per_s=1e3 * B / off, on_images_per_s=1e3 * B / on)
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--configs', default='kernels,step')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, 'tools'))
    import torch
    from bench_infer import timed
    configs = [c for c in a.configs.split(',') if c]
    assert configs and set(configs) <= {'kernels', 'step'}, a.configs
    assert torch.cuda.is_available(), "bench_edge.py needs an MI355X"
    res = {'tool': 'bench_edge', 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0), 'reps_per_graph': REPS}
    if 'kernels' in configs:
        res['kernels_us_per_call'] = kernels(torch, timed, a.min_seconds, a.repeats)
    if 'step' in configs:
        res['step'] = step(torch, timed, a.min_seconds, a.repeats)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
