#!/usr/bin/env python3
"""Bit record of the loss entry points: every case runs on seeded inputs and its return code, loss word(s), gradient bytes and
workspace partials go to an .npz (an array of more than 64 KiB as the SHA-256 of its bytes); two records (two builds, one process
each - GAN_AMD_LIB selects the library) must be equal byte for byte.
  python tools/loss_bits.py run OUT.npz            every case (needs the GPU)
  python tools/loss_bits.py reject OUT.npz         the rejected calls only: they return before any launch (no GPU needed)
  python tools/loss_bits.py compare A.npz B.npz [OUT.json]     one row per case; exit status 1 unless all are equal"""
import ctypes as C, hashlib, itertools, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

REC = {}


def compare(pa, pb, out=None):
    a, b = np.load(pa), np.load(pb)
    rows = [{'case': k, 'equal': bool(k in a and k in b and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
                                      and a[k].tobytes() == b[k].tobytes())} for k in sorted(set(a.files) | set(b.files))]
    res = {'a': pa, 'b': pb, 'cases': len(rows), 'equal': sum(r['equal'] for r in rows), 'rows': rows}
    if out:
        json.dump(res, open(out, 'w'), indent=1)
    print(f"{res['equal']} of {res['cases']} arrays equal" + ''.join(f"\n  differs: {r['case']}" for r in rows if not r['equal']))
    return 0 if res['equal'] == res['cases'] else 1


if sys.argv[1] == 'compare':
    sys.exit(compare(*sys.argv[2:5]))

import torch
from gan_amd import _lib as L
lib = L.load()
TD = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16}
NAME = {L.F32: 'f32', L.BF16: 'bf16', L.F16: 'f16'}
PAIRS = ((lib.gan_dssim, L.GanDssimDesc, 11, 'dssim'), (lib.gan_edge_l1, L.GanEdgeDesc, 3, 'edge'),      # (.., smallest edge, tag)
         (lib.gan_image_quality, L.GanQualityDesc, 11, 'image_quality'))


def pair_desc(cls, a, b, da, ws, ws_bytes, out, dts=(0, 0, 0), acc=0, ls=None, grad_acc=0):
    if cls is L.GanQualityDesc:
        return cls(dts[0], dts[1], a, b, out, ws, ws_bytes)
    tail = (grad_acc,) if cls is L.GanEdgeDesc else ()
    return cls(dts[0], dts[1], a, b, 0.5, acc, out, 100.0, dts[2], da, ws, ws_bytes, ls, *tail)


def rejects():
    """One rejected call per entry point (five per descriptor entry point) on dummy host pointers: nothing is launched."""
    p = C.addressof(C.create_string_buffer(64))
    T = lambda n, h, w, c: L.GanTensor(p, n, h, w, c, 8)
    for fn in ('gan_bce_logits', 'gan_lsq_logits'):
        REC[f'reject {fn} count 0'] = getattr(lib, fn)(p, 0, 1.0, 1.0, 0, p, 1.0, L.F32, p, 8, p, None, None)
    for fn in ('gan_patchgan_losses', 'gan_patchgan_losses_lsq'):
        REC[f'reject {fn} count 0'] = getattr(lib, fn)(p, p, 0, L.F32, p, p, p, 8, 100.0, p, p, p, p, p, None, None)
    REC['reject gan_l1 shape'] = lib.gan_l1(L.F32, C.byref(T(1, 4, 4, 1)), C.byref(T(1, 4, 5, 1)), 1.0, 0, p, 1.0, None, p, None, None)
    for fn, cls, lo, tag in PAIRS:
        need = getattr(lib, f'gan_{tag}_workspace_bytes')(1, 16, 16, 1)
        good = lambda **kw: pair_desc(cls, T(1, 16, 16, 1), T(1, 16, 16, 1), T(1, 16, 16, 1), p, need, p, **kw)
        d = good(); d.struct_size += 4
        REC[f'reject {tag} struct_size'] = fn(C.byref(d), None)
        d = good(); d.b = T(1, 16, 17, 1)
        REC[f'reject {tag} shapes'] = fn(C.byref(d), None)
        d = good(); d.a = d.b = T(1, 16, 16, 2)
        REC[f'reject {tag} c=2'] = fn(C.byref(d), None)
        d = good(); d.a = d.b = T(1, 16, lo - 1, 1)
        if cls is not L.GanQualityDesc:
            d.da = d.a
        REC[f'reject {tag} small edge'] = fn(C.byref(d), None)
        d = good(); d.workspace_bytes = need - 1
        REC[f'reject {tag} workspace'] = fn(C.byref(d), None)


def raw(t):
    b = t.contiguous().view(torch.uint8).cpu().numpy()
    return b if b.nbytes <= 65536 else np.frombuffer(hashlib.sha256(b.tobytes()).digest(), np.uint8)


def image(shape, pitch, dt, seed, like=None):
    """[n, h, w, pitch] of dtype dt, the pad channels 0.25; -> (tensor, GanTensor with c real channels)"""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    t = torch.full((n, h, w, pitch), 0.25)
    t[..., :c] = torch.rand((n, h, w, c), generator=g) * 2 - 1 if like is None else like[..., :c].float().cpu()
    t = t.to(TD[dt]).cuda()
    return t, L.GanTensor(t.data_ptr(), n, h, w, c, pitch)


def run():
    dev, st = 'cuda', None
    word = lambda v=1.5, n=1: torch.full((n,), v, device=dev)
    scale = lambda on: torch.tensor([1024.0, 1 / 1024.0, 0.0, 0.0], device=dev) if on else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    for fn, counts in (('gan_bce_logits', (1, 255, 257, 262147)), ('gan_lsq_logits', (1, 255, 257, 262147))):
        for count, dt, ls, acc, grad in itertools.product(counts, TD, (0, 1), (0, 1), (0, 1)):
            x = (torch.randn(count, generator=torch.Generator().manual_seed(count)) * 3).cuda()
            loss, ws, s = word(), word(0.0, 1024), scale(ls)
            dx = torch.full((count, 8), 0.25, dtype=TD[dt], device=dev) if grad else None
            rc = getattr(lib, fn)(x.data_ptr(), count, 1.0 - acc, 0.5, acc, loss.data_ptr(), 0.5, dt, ptr(dx), 8, ws.data_ptr(), ptr(s), st)
            key = f'{fn} {count} {NAME[dt]} ls{ls} acc{acc} dx{grad}'
            REC[key + ' rc'], REC[key + ' loss'], REC[key + ' ws'] = rc, raw(loss), raw(ws)
            if grad:
                REC[key + ' dx'] = raw(dx)
    for fn in ('gan_patchgan_losses', 'gan_patchgan_losses_lsq'):
        for count, dt, ls, null, l1 in itertools.product((1, 257, 65541), TD, (0, 1), (None, 0, 1, 2), (0, 1)):
            g = torch.Generator().manual_seed(count)
            r, f = (torch.randn(count, generator=g) * 3).cuda(), (torch.randn(count, generator=g) * 3).cuda()
            maps = [None if k == null else torch.full((count, 8), 0.25, dtype=TD[dt], device=dev) for k in range(3)]
            out, ws, s, l1w = word(1.5, 3), word(0.0, 768), scale(ls), word(0.37) if l1 else None
            rc = getattr(lib, fn)(r.data_ptr(), f.data_ptr(), count, dt, *[ptr(m) for m in maps], 8, 100.0, ptr(l1w), out.data_ptr(),
                                  out.data_ptr() + 4, out.data_ptr() + 8, ws.data_ptr(), ptr(s), st)
            key = f'{fn} {count} {NAME[dt]} ls{ls} null{null} l1{l1}'
            REC[key + ' rc'], REC[key + ' losses'], REC[key + ' ws'] = rc, raw(out), raw(ws)
            for k, m in enumerate(maps):
                if m is not None:
                    REC[key + f' grad{k}'] = raw(m)
    for (shape, pa, pb), dt, ls, acc, grad in itertools.product((((1, 3, 5, 1), 8, 8), ((3, 256, 256, 3), 8, 8), ((2, 9, 7, 3), 8, 4)),
                                                              TD, (0, 1), (0, 1), (0, 1)):
        (a, ta), (b, tb), (da, tda) = image(shape, pa, dt, 1), image(shape, pb, dt, 2), image(shape, 8, dt, 3)
        loss, ws, s = word(), word(0.0, 2048), scale(ls)
        rc = lib.gan_l1(dt, C.byref(ta), C.byref(tb), 0.5, acc, loss.data_ptr(), 100.0, C.byref(tda) if grad else None, ws.data_ptr(), ptr(s), st)
        key = f'gan_l1 {shape} pitch {pa}/{pb} {NAME[dt]} ls{ls} acc{acc} da{grad}'
        REC[key + ' rc'], REC[key + ' loss'], REC[key + ' ws'], REC[key + ' da'] = rc, raw(loss), raw(ws), raw(da)
    F, B, H = L.F32, L.BF16, L.F16
    cases = [(0, (1, 11, 11, 1), (F, F, F), (8, 8)), (0, (2, 43, 75, 3), (F, F, F), (8, 8)), (0, (2, 43, 75, 3), (B, F, B), (8, 8)),
             (0, (2, 43, 75, 3), (H, H, H), (8, 4)), (1, (1, 3, 3, 1), (F, F, F), (3, 3)), (1, (2, 33, 65, 3), (B, B, B), (8, 8)),
             (1, (2, 33, 65, 3), (H, F, H), (8, 3)), (1, (2, 33, 65, 3), (F, F, F), (3, 4)), (2, (1, 11, 11, 1), (F, F, F), (8, 8)),
             (2, (3, 43, 75, 3), (F, F, F), (8, 8)), (2, (3, 43, 75, 3), (B, F, B), (8, 3))]
    for (which, shape, dts, pitch), same, ls, acc, grad, gacc in itertools.product(cases, (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        fn, cls, _, tag = PAIRS[which]
        if (gacc and (which != 1 or not grad)) or (which == 2 and (ls or acc or grad)):
            continue                                    # grad_accumulate: gan_edge_l1 with da only; the metric has none of the options
        a, ta = image(shape, pitch[0], dts[0], 4)
        b, tb = image(shape, pitch[1], dts[1], 5, like=a if same else None)
        da, tda = image(shape, 8, dts[2], 6)
        need = getattr(lib, f'gan_{tag}_workspace_bytes')(*shape)
        ws, s, out = word(0.0, need // 4), scale(ls), word(1.5, 4 * shape[0])
        d = pair_desc(cls, ta, tb, tda if grad else L.GanTensor(), ws.data_ptr(), need, out.data_ptr(), dts, acc, ptr(s), gacc)
        key = f'{tag} {shape} {"/".join(NAME[t] for t in dts)} pitch {pitch} same{same} ls{ls} acc{acc} da{grad} gacc{gacc}'
        REC[key + ' rc'], REC[key + ' out'], REC[key + ' ws'], REC[key + ' da'] = fn(C.byref(d), st), raw(out), raw(ws), raw(da)
    torch.cuda.synchronize()


rejects()
if sys.argv[1] == 'run':
    run()
np.savez(sys.argv[2], **{k: np.asarray(v) for k, v in REC.items()})
print(f"{len(REC)} arrays -> {sys.argv[2]} ({L.LIB_PATH})")
