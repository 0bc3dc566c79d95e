#!/usr/bin/env python3
"""Cost of tiled inference: what the two launches around the forward - gan_tile_gather_u8 before it,
gan_tile_blend after it - add to the forward they wrap, and what the same work costs on the host.

    python tools/bench_tiled.py [--min-seconds 1.0] [--repeats 3] [--out profiles/bench_tiled.json]

One 512 x 640 single-channel image in bf16, at tiles of 256 with overlap 64 (3 x 3 tiles) and tiles of 512 with overlap 128
(1 x 2).  Per point, with the weights folded beforehand:
  (a) forward_us : the eval forward alone on the nt tiles already in the call's input buffer;
  (b) tiled_us   : GeneratorModel.infer_tiled end to end (gather, the same forward, blend; the uint8 image is on the device);
  (c) host_us    : the host-side alternative - numpy cut of the normalised image, infer (upload + pack + forward + unpack), .cpu(),
                   numpy weighted sum - wall clock, since it ends in a device-to-host copy.
(a) and (b): HIP events around as many back-to-back calls as fill --min-seconds (tools/bench_infer.py's `timed`), alternating,
--repeats times each; the median is reported beside every repeat.  overhead = (b - a) / a.  `bytes` are what the two launches move
by the shapes: the gather writes nt * S * S * c real elements into the pitch-8 buffer (one 16-byte slot per pixel) and reads
nt * S * S * c bytes; the blend reads the nt * S * S 16-byte slots and writes H * W * c * 4.  Prints one JSON object; --out also
saves it.  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_infer import timed  # noqa: E402
from gan_amd import data as D  # noqa: E402
from gan_amd.base_gan import GeneratorModel  # noqa: E402
from gan_amd.nets import Ctx, GeneratorNet, workspace_mb_for  # noqa: E402
from gan_amd.tiling import tile_origins  # noqa: E402

H, W, CH = 512, 640, 1
POINTS = [(256, 64), (512, 128)]          # tile, overlap


def host_weights(L_, S, V):
    """float32 [n, L_]: hat weight of tile k at coordinate p over the sum of the hats that cover p."""
    org = tile_origins(L_, S, V)
    hat = np.zeros((len(org), L_), np.float32)
    i = np.arange(S)
    for k, o in enumerate(org):
        hat[k, o:o + S] = np.minimum(i + 1, S - i)
    return org, hat / hat.sum(axis=0, keepdims=True)


def host_tiled(model, img_u8, S, V):
    """The host-side alternative: cut and blend in numpy, the tiles through `infer` as one batch."""
    (oys, wy), (oxs, wx) = host_weights(H, S, V), host_weights(W, S, V)
    x = D.normalize(img_u8.astype(np.float32))
    tiles = np.stack([x[oy:oy + S, ox:ox + S] for oy in oys for ox in oxs])
    out = model.infer(tiles, fold=False).cpu().numpy()
    image = np.zeros((H, W, CH), np.float32)
    t = 0
    for ky, oy in enumerate(oys):
        for kx, ox in enumerate(oxs):
            image[oy:oy + S, ox:ox + S] += (wy[ky, oy:oy + S, None] * wx[kx, None, ox:ox + S])[..., None] * out[t]
            t += 1
    return image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tiled.py needs an MI355X"
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=workspace_mb_for(9, 512))
    model = GeneratorModel(GeneratorNet(ctx, CH, 'batchnorm', seed=1))
    model.fold()
    img = np.random.default_rng(0).integers(0, 256, (H, W, CH), dtype=np.uint8)
    src = torch.from_numpy(img).to(ctx.device)
    res = {'tool': 'bench_tiled', 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0), 'image': [H, W, CH],
           'dtype': 'bf16', 'points': []}
    for S, V in POINTS:
        nt = len(tile_origins(H, S, V)) * len(tile_origins(W, S, V))
        call = model.eval_call(nt, S)
        tiled = lambda: model.infer_tiled(src, tile=S, overlap=V, fold=False)
        ref = torch.from_numpy(host_tiled(model, img, S, V)).to(ctx.device)
        diff = float((tiled() - ref).abs().max())          # the two routes predict the same image (bf16 network, fp32 blends)
        fwd, til = [], []
        for _ in range(a.repeats):
            fwd.append(timed(lambda: call.infer(fold=False), a.min_seconds)[0] * 1e3)
            til.append(timed(tiled, a.min_seconds)[0] * 1e3)
        host_tiled(model, img, S, V)
        torch.cuda.synchronize()
        reps, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < a.min_seconds:
            host_tiled(model, img, S, V)
            reps += 1
        host_us = (time.perf_counter() - t0) / reps * 1e6
        fa, tb = statistics.median(fwd), statistics.median(til)
        slots = nt * S * S * 16
        res['points'].append(dict(tile=S, overlap=V, tiles=nt, forward_us=fa, tiled_us=tb, overhead=(tb - fa) / fa,
                                  forward_us_repeats=fwd, tiled_us_repeats=til, host_us=host_us, host_calls=reps,
                                  host_over_tiled=host_us / tb, max_abs_diff_tiled_vs_host=diff,
                                  bytes=dict(gather_read=nt * S * S * CH, gather_written_real=nt * S * S * CH * 2,
                                             gather_slots_touched=slots, blend_read=slots, blend_written=H * W * CH * 4)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
