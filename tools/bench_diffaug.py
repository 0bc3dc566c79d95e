#!/usr/bin/env python3
"""Differentiable augmentation: its launches beside the copy they replace, and the captured Pix2Pix step
with and without the option.

    python tools/bench_diffaug.py [--min-seconds 1.0] [--repeats 3] [--configs kernels,step] [--out FILE]

kernels  on the step's layout (bf16, pitch 8): 256^2 batch 16 and 64 with c = 1, 512^2 batch 8 with c = 3.  gan_diffaug_apply forward
         and backward on the generated channels' views (g.out -> D's input at channel offset c; D's input gradient -> g.dgen2), the
         forward on the real half (c = 2 * channels, two images per sample), each beside gan_copy_view on the same views, and
         gan_diffaug_draw of 2 * batch records.  Every piece alone as a captured graph of REPS repetitions (the graph launch is
         amortised), HIP events around as many replays as fill --min-seconds; all four policies drawn by the library itself.
step     the captured step at 256^2 bf16 batch 16, diffaug=None against all four policies, interleaved, --repeats windows each.
Prints one JSON object; --out also saves it (profiles/bench_diffaug.json).  Reported, not gated."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
ALL = 'translation,cutout,brightness,saturation'


def med(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def kernels(torch, timed, min_s):
    import ctypes as C
    from gan_amd import _lib as L
    from gan_amd.diffaug import DiffAugment
    from gan_amd.nets import Buf, Ctx
    ctx = Ctx('cuda:0', 'bf16', lanes=False)
    out = {}

    def graph_us(fn):
        fn()
        torch.cuda.synchronize()
        g = ctx.capture_graph(lambda: [fn() for _ in range(REPS)])
        ms, _ = timed(g.replay, min_s)
        return 1e3 * ms / REPS

    for S, B, c in ((256, 16, 1), (256, 64, 1), (512, 8, 3)):
        aug = DiffAugment(ctx, ALL, seed=123)
        aug.draw(2 * B, S, S)
        gen, xin, raw = Buf(ctx, B, S, S, 8), Buf(ctx, 2 * B, S, S, 8), Buf(ctx, 2 * B, S, S, 8)
        for b in (gen, raw):
            b.t.uniform_(-1, 1)
        copy = lambda s_, d_: L.check(ctx.lib.gan_copy_view(ctx.dt, C.byref(s_), C.byref(d_), ctx.stream()), "copy_view")
        gv, fv = gen.view(0, c), xin.view(c, c, B, B)                       # the generated channels: g.out -> D(fake)'s slot
        rv, xv = raw.view(0, 2 * c, 0, B), xin.view(0, 2 * c, 0, B)         # the real half: [input | target]
        p = out[f'{S}x{S}_batch{B}_c{c}'] = {
            'generated_bytes_read_and_written': 2 * B * S * S * c * 2,
            'copy_view_generated_us': graph_us(lambda: copy(gv, fv)),
            'apply_forward_generated_us': graph_us(lambda: aug.apply(gv, fv, c, B)),
            'apply_backward_generated_us': graph_us(lambda: aug.apply(raw.view(0, c, 0, B), gv, c, B, backward=True)),
            'copy_view_real_half_us': graph_us(lambda: copy(rv, xv)),
            'apply_forward_real_half_us': graph_us(lambda: aug.apply(rv, xv, c, 0)),
            'draw_us': graph_us(lambda: aug.draw(2 * B, S, S)),
        }
        for k in ('apply_forward_generated', 'apply_backward_generated'):
            p[k + '_over_copy'] = p[k + '_us'] / p['copy_view_generated_us']
        p['apply_forward_real_half_over_copy'] = p['apply_forward_real_half_us'] / p['copy_view_real_half_us']
        del aug, gen, xin, raw
        torch.cuda.empty_cache()
    return out


def step(torch, timed, min_s, repeats):
    from gan_amd.diffaug import DiffAugment
    from gan_amd.nets import Ctx
    from gan_amd.steps import Pix2PixStep
    B, S = 16, 256
    ctx = Ctx('cuda:0', 'bf16')
    x, y = (torch.rand(B, S, S, 1, device=ctx.device) * 2 - 1 for _ in range(2))
    point = {'batch': B, 'size': S, 'dtype': 'bf16', 'unit': 'ms per replayed step'}
    for kind in ['off', 'on'] * repeats:
        kw = {'diffaug': DiffAugment(ctx, ALL, seed=123)} if kind == 'on' else {}
        st = Pix2PixStep(ctx, B, S, 1, seed=123, **kw)
        replay = st.capture(training=True)
        ms, _ = timed(lambda: replay(x, y), min_s)
        point.setdefault(kind + '_ms', []).append(ms)
        del st, replay, kw
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
    assert torch.cuda.is_available(), "bench_diffaug.py needs an MI355X"
    res = {'tool': 'bench_diffaug', 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0), 'reps_per_graph': REPS}
    if 'kernels' in configs:
        res['kernels_us_per_launch'] = kernels(torch, timed, a.min_seconds)
    if 'step' in configs:
        res['step'] = step(torch, timed, a.min_seconds, a.repeats)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
