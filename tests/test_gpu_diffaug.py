"""gan_diffaug_apply and gan_diffaug_draw on the GPU through the C ABI, against the float64 reference of
tests/diffaug_ref.py.  The parameter tables of the apply tests are GIVEN (hand-made records that reach every branch); the draw
tests compare the device table with the reference's restatement of the header's bit layout.

Gates.  Where colour is the identity the kernel moves bits: bit-equal.  Otherwise a handful of fp32 operations and one rounding:
fp32 storage within 4 fp32 ulps of the largest term of the element's arithmetic; 16-bit storage within one ulp of the storage type
at the expected value's magnitude.  The second gate presumes that the fp32 error (<= 4 ulp32 of the largest term = term * 2^-21)
stays below the half ulp that the rounding leaves free, i.e. |expected| >= term * 2^(m - 19) for m mantissa bits - false only
where the terms cancel almost completely (on images in [-1, 1] with s = 0.37 about one element in 10^4 does, e.g. 0.37 * 27/192 -
10/192).  The 16-bit inputs of the colour tables therefore cannot cancel: every image is of one sign with magnitudes 1 + k / 128 in
[1, 1.5], so that with |brightness| <= 0.5 and s in [0, 2] forward |y| >= (5 - 3) / 3 - 1/2 = 1/6 and backward |dx| >= 1/2 while no
term exceeds 3; `_inputs_are_fair` asserts the premise on the reference alone.  The table whose colour is neutral (bits move),
and all fp32 cases (their gate is relative to the largest term), take mixed-sign images on [-1, 1] with zeros."""
import ctypes as C

import numpy as np
import pytest
import torch

from gan_amd import _lib as L
from tests import diffaug_ref as R

pytestmark = pytest.mark.gpu

DT = {'f32': (L.F32, torch.float32, torch.int32), 'bf16': (L.BF16, torch.bfloat16, torch.int16), 'f16': (L.F16, torch.float16, torch.int16)}
SHAPES = [(16, 24), (17, 33), (8, 8)]
GROUPS = [(1, 1), (1, 2), (3, 3), (3, 6)]                 # (group_c, c)
BATCHES = [(1, 0), (1, 2), (3, 0), (3, 2)]                # (n, sample0)
GUARD = 64                                                # elements of NaN in front of and behind every buffer


def tables(h, w):
    """Three tables of five records.  0: colour neutral (bits move); 1, 2: s in {0, 1, 2, 0.37} x brightness in {0, +-0.5}.
    Geometry: t = (+-T, +-T), mixed signs, (0, 0) and one-pixel shifts; a cut at every corner, in the interior, over the whole image."""
    Tx, Ty = (w + 4) // 8, (h + 4) // 8
    cw, ch = w // 2, h // 2
    geo = [dict(tx=Tx, ty=Ty, cut_x0=0, cut_y0=0, cut_w=cw, cut_h=ch),                    # top left
           dict(tx=-Tx, ty=-Ty, cut_x0=w - cw, cut_y0=h - ch, cut_w=cw, cut_h=ch),        # bottom right
           dict(tx=0, ty=0, cut_x0=1, cut_y0=2, cut_w=cw, cut_h=ch),                      # interior
           dict(tx=Tx, ty=-Ty, cut_x0=w - cw, cut_y0=0, cut_w=cw, cut_h=ch),              # top right
           dict(tx=-Tx, ty=Ty, cut_x0=0, cut_y0=h - ch, cut_w=cw, cut_h=ch),              # bottom left
           dict(tx=1, ty=0, cut_x0=0, cut_y0=0, cut_w=w, cut_h=h),                        # everything cut
           dict(tx=0, ty=-1, cut_x0=0, cut_y0=0, cut_w=0, cut_h=0)]                       # no cut
    f32 = lambda v: float(np.float32(v))
    col1 = [(0.0, 0.5), (1.0, -0.5), (2.0, 0.0), (f32(0.37), 0.5), (1.0, 0.5)]
    col2 = [(2.0, -0.5), (f32(0.37), 0.0), (0.0, 0.0), (f32(0.37), -0.5), (2.0, 0.5)]
    t0 = [dict(R.NEUTRAL, **geo[i]) for i in range(5)]
    t1 = [dict(geo[i], saturation=s, brightness=b) for i, (s, b) in enumerate(col1)]
    t2 = [dict(geo[i], saturation=s, brightness=b) for i, (s, b) in zip((5, 6, 1, 3, 2), col2)]
    return [t0, t1, t2]


def test_the_tables_cover_what_they_must():
    for h, w in SHAPES:
        Tx, Ty = (w + 4) // 8, (h + 4) // 8
        recs = [p for t in tables(h, w) for p in t]
        ts = {(p['tx'], p['ty']) for p in recs}
        assert {(Tx, Ty), (-Tx, -Ty), (Tx, -Ty), (-Tx, Ty), (0, 0)} <= ts
        corners = {(p['cut_x0'] == 0, p['cut_y0'] == 0, p['cut_x0'] + p['cut_w'] == w, p['cut_y0'] + p['cut_h'] == h) for p in recs if p['cut_w']}
        assert {(True, True, False, False), (False, False, True, True), (False, True, True, False), (True, False, False, True),
                (False, False, False, False), (True, True, True, True)} <= corners
        assert {round(p['saturation'], 2) for p in recs} == {0.0, 1.0, 2.0, 0.37} and {p['brightness'] for p in recs} == {0.0, 0.5, -0.5}


class Views:
    """src and dst of one case in NaN-guarded buffers: n x h x w pixels of `pitch` elements, the view's c channels at an offset."""

    def __init__(self, dtype, n, h, w, c, spitch, dpitch, soff, doff, seed, one_sign=False):
        self.dt, self.td, self.ti = DT[dtype]
        self.dtype, self.shape = dtype, (n, h, w, c)
        rng = np.random.default_rng(seed)
        if dtype == 'f32':
            self.x = rng.uniform(-1, 1, (n, h, w, c)).astype(np.float32).astype(np.float64)
        elif one_sign:        # (module docstring) one sign per sample, magnitudes in [1, 1.5] on a grid both 16-bit types hold
            self.x = (1 + rng.integers(0, 65, (n, h, w, c)) / 128) * rng.choice([-1.0, 1.0], (n, 1, 1, 1))
        else:
            self.x = rng.integers(-64, 65, (n, h, w, c)).astype(np.float64) / 64
        self.geom = {'src': (spitch, soff), 'dst': (dpitch, doff)}
        self.src = self._buffer(spitch, float('nan'))
        self._real(self.src, spitch, soff)[:] = torch.from_numpy(self.x).to(self.td).cuda()
        self.dst0 = self._buffer(dpitch, float('nan'))
        self.dst0.view(self.ti)[1::2] = 0x4321 if dtype != 'f32' else 0x43214321        # (a second sentinel pattern: not every bit set alike)
        self.dst = self.dst0.clone()
        self.es = self.src.element_size()

    def _buffer(self, pitch, fill):
        n, h, w, _ = self.shape
        return torch.full((2 * GUARD + n * h * w * pitch,), fill, dtype=self.td, device='cuda')

    def _real(self, buf, pitch, off):
        n, h, w, c = self.shape
        return buf[GUARD:GUARD + n * h * w * pitch].view(n, h, w, pitch)[..., off:off + c]

    def tensor(self, which, buf=None):
        pitch, off = self.geom[which]
        n, h, w, c = self.shape
        buf = buf if buf is not None else getattr(self, which)
        return L.GanTensor(buf.data_ptr() + (GUARD + off) * self.es, n, h, w, c, pitch)

    def desc(self, table, group_c, sample0, direction, src=None, dst=None):
        return L.GanDiffAugDesc(self.dt, self.tensor('src', src), self.tensor('dst', dst), group_c, sample0, table.data_ptr(), direction)

    def run(self, table, group_c, sample0, direction, src=None, dst=None):
        d = self.desc(table, group_c, sample0, direction, src, dst)
        L.check(L.load().gan_diffaug_apply(C.byref(d), torch.cuda.current_stream().cuda_stream), "diffaug_apply")

    def result(self, buf=None):
        """(the view's values as float64 numpy, True where every element outside the view kept its bits)."""
        buf = buf if buf is not None else self.dst
        pitch, off = self.geom['dst']
        n, h, w, c = self.shape
        got = self._real(buf, pitch, off).double().cpu().numpy()
        a, b = buf.view(self.ti).clone(), self.dst0.view(self.ti).clone()
        for t in (a, b):
            t[GUARD:GUARD + n * h * w * pitch].view(n, h, w, pitch)[..., off:off + c] = 0
        return got, bool((a == b).all())

    def bits(self, buf=None):
        return (buf if buf is not None else self.dst).view(self.ti).clone()


def _inputs_are_fair(want, term, dtype):
    """See the module docstring: asserted on the reference alone."""
    m = R.MANTISSA[dtype]
    small = (want != 0) & (np.abs(want) < term * 2.0 ** (m - 19))
    assert not small.any(), (dtype, np.abs(want[small]).min())


def _check(got, want, term, dtype, moved, what):
    if moved:
        td = DT[dtype][1]
        wb = torch.from_numpy(want + 0.0).to(td)                    # (the stored inputs themselves, or the fill: +0, where the
                                                                    # reference's product with the mask gives -0 for a negative input)
        gb = torch.from_numpy(got).to(td)
        assert (gb.view(DT[dtype][2]) == wb.view(DT[dtype][2])).all(), what
        return 0.0
    err = np.abs(got - want)
    if dtype == 'f32':
        gate = 4 * R.ulp(term, 'f32')
    else:
        _inputs_are_fair(want, term, dtype)
        gate = R.ulp(want, dtype)
    worst = float((err / gate).max())
    print(f"{what}: worst error {worst:.3f} of the gate")
    assert (err <= gate).all(), (what, worst)
    return worst


def _layouts(dtype, c):
    """(src pitch, dst pitch, src channel offset, dst channel offset): dense; the step's pitch 8 (one 16-byte load per pixel in the
    16-bit types); pitch 8 with channel offsets on both sides (element loads, unaligned views); fp32 pitch 4 (16-byte loads)."""
    out = [(c, c, 0, 0), (8, 8, 0, 8 - c)]
    if c < 8:
        out.append((8, 8, 1, 0))
    if dtype == 'f32' and c <= 4:
        out.append((4, 8, 0, 1))
    return out


@pytest.mark.parametrize('dtype', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('h,w', SHAPES)
def test_apply_forward_and_backward_against_the_reference(dtype, h, w):
    tabs = tables(h, w)
    dev = [torch.from_numpy(R.table(t)).cuda() for t in tabs]
    worst = 0.0
    for gi, (group_c, c) in enumerate(GROUPS):
        for n, sample0 in BATCHES:
            for li, (sp, dp, so, do) in enumerate(_layouts(dtype, c)):
                for ti, (tab, dtab) in enumerate(zip(tabs, dev)):
                    v = Views(dtype, n, h, w, c, sp, dp, so, do, seed=1000 * gi + 10 * n + li, one_sign=ti > 0)
                    x = torch.from_numpy(v.x)
                    what = f"{dtype} {h}x{w} g{group_c} c{c} n{n} s0={sample0} layout {(sp, dp, so, do)} table {ti}"
                    used = tab[sample0:sample0 + n]
                    # forward
                    v.dst.copy_(v.dst0)
                    v.run(dtab, group_c, sample0, 0)
                    got, kept = v.result()
                    assert kept, what + ": forward wrote outside the view's real channels"
                    want = R.forward(x, tab, group_c, sample0).numpy()
                    moved = all(p['brightness'] == 0 and (group_c == 1 or p['saturation'] == 1) for p in used)
                    worst = max(worst, _check(got, want, R.forward_terms(v.x, tab, group_c, sample0), dtype, moved, what + " forward"))
                    # backward: the same data as the upstream gradient
                    v.dst.copy_(v.dst0)
                    v.run(dtab, group_c, sample0, 1)
                    got, kept = v.result()
                    assert kept, what + ": backward wrote outside the view's real channels"
                    want = R.transpose(v.x, tab, group_c, sample0)
                    moved = all(group_c == 1 or p['saturation'] == 1 for p in used)
                    worst = max(worst, _check(got, want, R.transpose_terms(v.x, tab, group_c, sample0), dtype, moved, what + " backward"))
    print(f"{dtype} {h}x{w}: worst error over all cases {worst:.3f} of the gate")


def test_adjoint_identity_on_the_gpu_results_fp32():
    h, w, n, c, group_c = 17, 33, 3, 6, 3
    for ti, tab in enumerate(tables(h, w)[1:]):
        dtab = torch.from_numpy(R.table(tab)).cuda()
        vx, vy = Views('f32', n, h, w, c, 8, 8, 0, 2, seed=5), Views('f32', n, h, w, c, 8, 8, 0, 2, seed=6)
        vx.run(dtab, group_c, 2, 0)
        tx = vx.result()[0]
        zero = vx.src.clone()
        vx._real(zero, 8, 0)[:] = 0
        vx.dst.copy_(vx.dst0)
        vx.run(dtab, group_c, 2, 0, src=zero)
        t0 = vx.result()[0]                                          # T 0: the brightness offset
        vy.run(dtab, group_c, 2, 1)
        tty = vy.result()[0]
        lhs, rhs = ((tx - t0) * vy.x).sum(), (vx.x * tty).sum()
        print(f"table {ti + 1}: <Tx, y> = {lhs:.9g}, <x, T'y> = {rhs:.9g}")
        assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


@pytest.mark.parametrize('dtype', ['f32', 'bf16', 'f16'])
def test_pads_determinism_refusals_and_capture(dtype):
    h, w, n, c, group_c, sample0 = 17, 33, 3, 3, 3, 2
    tab = tables(h, w)[1]
    dtab = torch.from_numpy(R.table(tab)).cuda()
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    for direction in (0, 1):
        v = Views(dtype, n, h, w, c, 8, 8, 0, 5, seed=11)
        v.run(dtab, group_c, sample0, direction)
        first = v.bits()
        v.dst.copy_(v.dst0)
        v.run(dtab, group_c, sample0, direction)
        assert (v.bits() == first).all()                             # two calls, the same bits
        clean = torch.zeros_like(v.src)                              # the same images without a NaN anywhere in or around the source
        v._real(clean, 8, 0)[:] = v._real(v.src, 8, 0)
        v.dst.copy_(v.dst0)
        v.run(dtab, group_c, sample0, direction, src=clean)
        assert (v.bits() == first).all()                             # NaN in the pad channels and around the buffer changed nothing
        # refused descriptors write nothing
        v.dst.copy_(v.dst0)
        for field, bad in (('group_c', 2), ('direction', 2), ('sample0', -1), ('dtype', 7), ('params', None), ('struct_size', 8)):
            d = v.desc(dtab, group_c, sample0, direction)
            setattr(d, field, bad)
            assert lib.gan_diffaug_apply(C.byref(d), st) == L.E_ARG, field
        d = v.desc(dtab, group_c, sample0, direction)
        d.dst.pitch = 2
        assert lib.gan_diffaug_apply(C.byref(d), st) == L.E_ARG
        d = v.desc(dtab, group_c, sample0, direction)
        d.src.h = h + 1
        assert lib.gan_diffaug_apply(C.byref(d), st) == L.E_ARG
        torch.cuda.synchronize()
        assert (v.bits() == v.bits(v.dst0)).all()
        # a captured call replays the eager bits
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side):
                v.run(dtab, group_c, sample0, direction)
        torch.cuda.current_stream().wait_stream(side)
        v.dst.copy_(v.dst0)
        gr.replay()
        torch.cuda.synchronize()
        assert (v.bits() == first).all()


# ---- gan_diffaug_draw ---------------------------------------------------------------------------------------------------------------
def _draw(tab, n, h, w, policy, seed, sid, launches):
    L.check(L.load().gan_diffaug_draw(tab.data_ptr(), n, h, w, policy, seed, sid, launches.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "diffaug_draw")


def test_draw_equals_the_reference_and_advances_its_counter():
    n, h, w, seed, sid = 7, 17, 33, 123, 48
    tab = torch.full((n + 1, 8), -1, dtype=torch.int32, device='cuda')
    launches = torch.zeros(1, dtype=torch.int32, device='cuda')
    for k in range(3):
        _draw(tab, n, h, w, 15, seed, sid, launches)
        assert int(launches.item()) == k + 1
        assert (tab[:n].cpu().numpy() == R.table(R.draw(seed, k, sid, n, h, w, R.POLICIES))).all(), k
        assert (tab[n] == -1).all()                                  # nothing behind the n records
    # under graph replay the counter advances by one per replay and the table is the reference's of that launch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            _draw(tab, n, h, w, 15, seed, sid, launches)
    torch.cuda.current_stream().wait_stream(side)
    assert int(launches.item()) == 3                                 # (the capture itself launched nothing)
    for k in (3, 4):
        gr.replay()
        torch.cuda.synchronize()
        assert int(launches.item()) == k + 1
        assert (tab[:n].cpu().numpy() == R.table(R.draw(seed, k, sid, n, h, w, R.POLICIES))).all(), k


def test_draw_policies_streams_and_the_full_table():
    n, h, w, seed = 128, 256, 256, 99
    tab = torch.zeros((n, 8), dtype=torch.int32, device='cuda')
    for mask in (0, 1, 2, 4, 8, 5, 10):
        pol = tuple(p for i, p in enumerate(R.POLICIES) if mask >> i & 1)
        launches = torch.zeros(1, dtype=torch.int32, device='cuda')
        _draw(tab, n, h, w, mask, seed, 48, launches)
        got = R.records(tab.cpu().numpy())
        assert got == R.draw(seed, 0, 48, n, h, w, pol), mask
        for key, on in (('tx', 1), ('ty', 1), ('cut_w', 2), ('cut_h', 2), ('cut_x0', 2), ('cut_y0', 2), ('brightness', 4), ('saturation', 8)):
            if not mask & on:                                        # a policy that is off: its neutral value in every record
                assert all(p[key] == R.NEUTRAL[key] for p in got), (mask, key)
    launches = torch.zeros(1, dtype=torch.int32, device='cuda')
    _draw(tab, n, h, w, 15, seed, 48, launches)
    a = tab.clone()
    launches.zero_()
    _draw(tab, n, h, w, 15, seed, 49, launches)
    assert not (a == tab).all(dim=1).any()                            # another stream id: no record repeats
