// Image preprocessing of the resident uint8 images (include/gan_amd.h: gan_preprocess_u8): CLAHE, an
// integer Gaussian blur and a 3 x 3 sharpening filter over REGIONS of a packed buffer, in place.
//
// The CLAHE blend is the one place where these bytes could differ from the numpy restatement (gan_amd/preprocess.py) by a fused
// multiply-add, so this file is compiled with contraction OFF: the pragma below, and -ffp-contract=off on the file's Makefile rule.
// (HIP's __fmul_rn / __fadd_rn are plain `*` / `+` inside inline functions and do not stop the compiler from fusing them.)
#pragma clang fp contract(off)
#include <cmath>

#include "common.h"

// reflect-101 of an index into [0, n); the clamp only ever moves indices of tile parts that lie outside the region (unused values)
__device__ __forceinline__ int pre_reflect(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}
__device__ __forceinline__ int pre_floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

struct PreRegionDev {
  long long off;      // byte offset of the region in the buffer
  long long scratch;  // byte offset of its dense copy in the scratch area
  int pitch, h, w;    // bytes between rows; rows; pixels per row
  int spitch;         // bytes between rows of the dense copy (w * c rounded up to 4)
  int tw, th, limit;  // CLAHE: tile size of the padded region, clip limit in counts
  float scale, inv_tw, inv_th;  // CLAHE: float(255 / area), 1.0f / tw, 1.0f / th - computed once on the host
};
struct PreArgs {
  uint8_t* buf;      // the packed images
  uint8_t* lut;      // workspace: [region][channel][tile row][tile column][256]
  uint8_t* scratch;  // workspace: the dense copies
  int c, grid;
  int r, to_buf;     // stencils: blur radius; 0 = buffer -> scratch, 1 = scratch -> buffer
  int q[6];          // blur taps q[0 .. r]
  PreRegionDev g[GAN_PREPROCESS_MAX_REGIONS];
};

// ---- CLAHE, tile tables ---------------------------------------------------------------------------------------------------------
// One workgroup per (tile, channel, region).  The histogram is privatised per wave (four copies in LDS): a constant tile - thermal
// frames have large flat areas - serialises the 64 lanes of a wave on one counter, not the 256 lanes of the workgroup.  Padded
// pixels are read through the reflect index, never outside the region.  Clip sum by a tree in LDS, the residual rule in closed
// form per bin, a 256-wide Hillis-Steele scan, 256 bytes out.
__global__ __launch_bounds__(256) void pre_lut_kernel(const PreArgs a) {
  __shared__ unsigned s_hist[4][256];
  __shared__ unsigned s_scan[256];
  const PreRegionDev& g = a.g[blockIdx.z];
  const int tid = threadIdx.x, wave = tid >> 6, ch = blockIdx.y;
  const int ty = blockIdx.x / a.grid, tx = blockIdx.x - ty * a.grid;
#pragma unroll
  for (int k = 0; k < 4; ++k) s_hist[k][tid] = 0;
  __syncthreads();
  const int area = g.tw * g.th;
  const uint8_t* __restrict__ base = a.buf + g.off + ch;
  for (int i = tid; i < area; i += 256) {
    const int py = i / g.tw, px = i - py * g.tw;
    const int gy = pre_reflect(ty * g.th + py, g.h), gx = pre_reflect(tx * g.tw + px, g.w);
    atomicAdd(&s_hist[wave][base[(long long)gy * g.pitch + gx * a.c]], 1u);
  }
  __syncthreads();
  unsigned h = s_hist[0][tid] + s_hist[1][tid] + s_hist[2][tid] + s_hist[3][tid];
  const unsigned lim = (unsigned)g.limit;
  s_scan[tid] = h > lim ? h - lim : 0u;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) s_scan[tid] += s_scan[tid + s];
    __syncthreads();
  }
  const unsigned clipped = s_scan[0];
  __syncthreads();
  const unsigned batch = clipped >> 8, residual = clipped & 255u;
  h = min(h, lim) + batch;
  if (residual) {
    const unsigned step = max(256u / residual, 1u);
    if (tid % step == 0 && tid / step < residual) ++h;
  }
  s_scan[tid] = h;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned t = tid >= d ? s_scan[tid - d] : 0u;
    __syncthreads();
    s_scan[tid] += t;
    __syncthreads();
  }
  const float f = rintf((float)s_scan[tid] * g.scale);
  a.lut[(((long long)blockIdx.z * a.c + ch) * a.grid * a.grid + blockIdx.x) * 256 + tid] = (uint8_t)fminf(fmaxf(f, 0.f), 255.f);
}

// ---- CLAHE, apply ---------------------------------------------------------------------------------------------------------------
// The rows whose upper table row is k - 1 (ty1 = floor(y / th - 0.5), before the clamp) form interval k = 0 .. grid of about th rows;
// a workgroup owns PRE_APPLY_ROWS candidate rows of one interval of one region and keeps those of them whose own fp32 ty1 says so
// (the candidates overshoot the interval by a row on either side, so no rounding of y * inv_th can lose a row).  All of its rows
// need the same two table rows: they are staged in LDS, 2 * c * grid * 256 bytes, when that is at most PRE_LUT_LDS; a larger
// set (grid 32 with three channels: 48 KiB) is read from the workspace instead.  A lane handles four consecutive bytes of a
// row, as one 32-bit load and store where the address allows.  In place: a byte depends on its own old value and the tables only.
constexpr int PRE_LUT_LDS = 32768, PRE_APPLY_ROWS = 16;

template <int C>
__global__ __launch_bounds__(256) void pre_apply_kernel(const PreArgs a, const int nsub, const int staged) {
  extern __shared__ uint4 s_lut4[];
  const PreRegionDev& g = a.g[blockIdx.y];
  const int tid = threadIdx.x, grid = a.grid;
  const int k = blockIdx.x / nsub, sub = blockIdx.x - k * nsub;
  const int first = pre_floordiv((2 * k - 1) * g.th, 2) - 1;
  const int ylo = max(first + sub * PRE_APPLY_ROWS, 0), yhi = min(min(first + (sub + 1) * PRE_APPLY_ROWS, first + g.th + 3), g.h);
  if (ylo >= yhi) return;          // (the whole workgroup)
  const int ty1 = max(k - 1, 0), ty2 = min(k, grid - 1);
  const uint8_t* lutg = a.lut + (long long)blockIdx.y * C * grid * grid * 256;
  const int rowb = grid * 256;     // bytes of one table row
  if (staged) {
    const int vec = rowb / 16;
    for (int i = tid; i < 2 * C * vec; i += 256) {
      const int j = i / (C * vec), rem = i - j * C * vec, ch = rem / vec, v = rem - ch * vec;
      s_lut4[i] = *(const uint4*)(lutg + ((long long)(ch * grid + (j ? ty2 : ty1)) * grid) * 256 + 16 * v);
    }
    __syncthreads();
  }
  const uint8_t* L1[C];
  const uint8_t* L2[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    L1[ch] = staged ? (const uint8_t*)s_lut4 + ch * rowb : lutg + (long long)(ch * grid + ty1) * rowb;
    L2[ch] = staged ? (const uint8_t*)s_lut4 + (C + ch) * rowb : lutg + (long long)(ch * grid + ty2) * rowb;
  }
  const int nb = g.w * C;
  for (int y = ylo; y < yhi; ++y) {
    const float tyf = (float)y * g.inv_th - 0.5f, tyfl = floorf(tyf);
    if ((int)tyfl != k - 1) continue;
    const float ya = tyf - tyfl, ya1 = 1.0f - ya;
    uint8_t* row = a.buf + g.off + (long long)y * g.pitch;
    const bool aligned = (((uintptr_t)row) & 3) == 0;
    for (int b0 = tid * 4; b0 < nb; b0 += 1024) {
      const bool whole = aligned && b0 + 4 <= nb;
      uint32_t word = 0;
      if (whole) {
        word = *(const uint32_t*)(row + b0);
      } else {
        for (int e = 0; e < 4; ++e)
          if (b0 + e < nb) word |= (uint32_t)row[b0 + e] << (8 * e);
      }
      uint32_t res = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int b = min(b0 + e, nb - 1), x = b / C, ch = b - x * C;
        const uint32_t v = (word >> (8 * e)) & 255u;
        const float txf = (float)x * g.inv_tw - 0.5f, txfl = floorf(txf);
        const float xa = txf - txfl, xa1 = 1.0f - xa;
        const int tx1 = max((int)txfl, 0), tx2 = min((int)txfl + 1, grid - 1);
        const uint8_t* p1 = L1[0];
        const uint8_t* p2 = L2[0];
#pragma unroll
        for (int cc = 1; cc < C; ++cc)
          if (ch == cc) { p1 = L1[cc]; p2 = L2[cc]; }
        const float l11 = (float)p1[tx1 * 256 + v], l12 = (float)p1[tx2 * 256 + v];
        const float l21 = (float)p2[tx1 * 256 + v], l22 = (float)p2[tx2 * 256 + v];
        const float top = l11 * xa1 + l12 * xa, bot = l21 * xa1 + l22 * xa;
        const float o = rintf(top * ya1 + bot * ya);
        res |= (uint32_t)fminf(fmaxf(o, 0.f), 255.f) << (8 * e);
      }
      if (whole) {
        *(uint32_t*)(row + b0) = res;
      } else {
        for (int e = 0; e < 4; ++e)
          if (b0 + e < nb) row[b0 + e] = (uint8_t)(res >> (8 * e));
      }
    }
  }
}

// ---- stencils: copy, blur, sharpen ------------------------------------------------------------------------------------------------
// Out of place between a region and its dense copy in the scratch area.  A workgroup owns PRE_TH rows x PRE_TW byte columns of the
// output and stages them with a halo of r rows and r * c byte columns in LDS; the halo is the reflect-101 of the REGION (the source
// index of every staged byte is reflected in pixel coordinates), not of the tile.  Blur: a horizontal pass over every staged row
// into 16-bit sums, then the vertical pass.  A lane produces four consecutive bytes, stored as one 32-bit word where the address
// allows.  MODE 0 copies (r = 0): the first pass of a chain with a single stencil stage, so that the result lands in the region.
constexpr int PRE_TH = 32, PRE_TW = 128, PRE_RMAX = 5;
constexpr int PRE_LH = PRE_TH + 2 * PRE_RMAX, PRE_LW = PRE_TW + 2 * PRE_RMAX * 3;
enum { PRE_COPY = 0, PRE_BLUR = 1, PRE_SHARPEN = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void pre_stencil_kernel(const PreArgs a) {
  __shared__ uint8_t s_in[PRE_LH][PRE_LW + 2];
  __shared__ uint16_t s_h[MODE == PRE_BLUR ? PRE_LH : 1][PRE_TW];
  const PreRegionDev& g = a.g[blockIdx.z];
  const int tid = threadIdx.x, c = a.c, nb = g.w * c;
  const int by0 = blockIdx.y * PRE_TH, bx0 = blockIdx.x * PRE_TW;
  if (by0 >= g.h || bx0 >= nb) return;          // (the whole workgroup)
  const uint8_t* __restrict__ src = a.to_buf ? a.scratch + g.scratch : a.buf + g.off;
  uint8_t* __restrict__ dst = a.to_buf ? a.buf + g.off : a.scratch + g.scratch;
  const int sp = a.to_buf ? g.spitch : g.pitch, dp = a.to_buf ? g.pitch : g.spitch;
  const int r = MODE == PRE_BLUR ? a.r : MODE == PRE_SHARPEN ? 1 : 0, rc = r * c;
  const int lh = PRE_TH + 2 * r, lw = PRE_TW + 2 * rc;
  int q[PRE_RMAX + 1];
#pragma unroll
  for (int j = 0; j <= PRE_RMAX; ++j) q[j] = a.q[j];
  for (int i = tid; i < lh * lw; i += 256) {
    const int ly = i / lw, lx = i - ly * lw;
    const int gy = pre_reflect(by0 - r + ly, g.h);
    const int vb = bx0 - rc + lx, vx = pre_floordiv(vb, c), ch = vb - vx * c;
    s_in[ly][lx] = src[(long long)gy * sp + pre_reflect(vx, g.w) * c + ch];
  }
  __syncthreads();
  if (MODE == PRE_BLUR) {
    for (int i = tid; i < lh * PRE_TW; i += 256) {
      const int ly = i / PRE_TW, x = i - ly * PRE_TW;
      int t = q[0] * s_in[ly][x + rc];
#pragma unroll
      for (int j = 1; j <= PRE_RMAX; ++j)
        if (j <= r) t += q[j] * (s_in[ly][x + rc - j * c] + s_in[ly][x + rc + j * c]);
      s_h[ly][x] = (uint16_t)t;            // <= 256 * 255
    }
    __syncthreads();
  }
  const int cx = (tid & 31) * 4, ry = tid >> 5;
#pragma unroll
  for (int j = 0; j < PRE_TH / 8; ++j) {
    const int oy = ry + 8 * j, gy = by0 + oy;
    if (gy >= g.h) continue;
    uint32_t res = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = cx + e;
      int o;
      if (MODE == PRE_BLUR) {
        int u = q[0] * s_h[oy + r][x];
#pragma unroll
        for (int t = 1; t <= PRE_RMAX; ++t)
          if (t <= r) u += q[t] * (s_h[oy + r - t][x] + s_h[oy + r + t][x]);
        o = (u + 32768) >> 16;
      } else if (MODE == PRE_SHARPEN) {
        o = 5 * s_in[oy + 1][x + rc] - s_in[oy][x + rc] - s_in[oy + 2][x + rc] - s_in[oy + 1][x] - s_in[oy + 1][x + 2 * rc];
        o = min(max(o, 0), 255);
      } else {
        o = s_in[oy][x];
      }
      res |= (uint32_t)o << (8 * e);
    }
    uint8_t* out = dst + (long long)gy * dp + bx0 + cx;
    if (bx0 + cx + 4 <= nb && (((uintptr_t)out) & 3) == 0) {
      *(uint32_t*)out = res;
    } else {
      for (int e = 0; e < 4; ++e)
        if (bx0 + cx + e < nb) out[e] = (uint8_t)(res >> (8 * e));
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static int pre_blur_radius(double sigma) { return ((int)nearbyint(6.0 * sigma + 1.0) | 1) / 2; }

// taps q[0 .. r] of the blur: q_i = rint(256 w_i) for i > 0, the centre takes what is left of 256 (float64, as gan_amd/preprocess.py)
static void pre_blur_taps(double sigma, int r, int* q) {
  double w[PRE_RMAX + 1], side = 0.0;
  for (int i = 0; i <= r; ++i) {
    w[i] = exp(-(double)(i * i) / (2.0 * sigma * sigma));
    if (i) side += w[i];
  }
  const double sum = w[0] + 2.0 * side;
  int rest = 256;
  for (int i = 1; i <= r; ++i) {
    q[i] = (int)nearbyint(256.0 * (w[i] / sum));
    rest -= 2 * q[i];
  }
  q[0] = rest;
}

static inline size_t pre_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// Everything gan_preprocess_u8 checks except the buffers themselves; -> 0 or the error, *need = workspace bytes.
static int pre_validate(const GanPreprocessDesc* d, size_t* need) {
  if (!d || d->struct_size != sizeof(GanPreprocessDesc)) return GAN_E_ARG;
  if (!d->regions || d->n < 1 || (d->c != 1 && d->c != 3)) return GAN_E_ARG;
  const uint32_t all = GAN_PRE_CLAHE | GAN_PRE_BLUR | GAN_PRE_SHARPEN;
  if (!d->stages || (d->stages & ~all)) return GAN_E_ARG;
  int r = 0;
  if (d->stages & GAN_PRE_CLAHE) {
    if (d->grid < 1 || d->grid > 32 || !(d->clip >= 0.f) || !std::isfinite(d->clip)) return GAN_E_ARG;
  }
  if (d->stages & GAN_PRE_BLUR) {
    if (!(d->sigma > 0.f) || !(d->sigma <= 1.5f)) return GAN_E_ARG;
    r = pre_blur_radius((double)d->sigma);
  }
  for (int i = 0; i < d->n; ++i) {
    const GanPreRegion& g = d->regions[i];
    if (g.height < 1 || g.width < 1 || g.src_offset < 0 || g.pitch < 1 || (int64_t)g.width * d->c > g.pitch) return GAN_E_ARG;
  }
  size_t worst = 0;
  for (int lo = 0; lo < d->n; lo += GAN_PREPROCESS_MAX_REGIONS) {
    const int m = d->n - lo < GAN_PREPROCESS_MAX_REGIONS ? d->n - lo : GAN_PREPROCESS_MAX_REGIONS;
    size_t bytes = (d->stages & GAN_PRE_CLAHE) ? pre_align16((size_t)m * d->c * d->grid * d->grid * 256) : 0;
    for (int i = 0; i < m; ++i) {
      const GanPreRegion& g = d->regions[lo + i];
      if ((d->stages & GAN_PRE_CLAHE) && (g.height < d->grid || g.width < d->grid)) return GAN_E_SHAPE;
      if ((d->stages & GAN_PRE_BLUR) && (g.height < r + 1 || g.width < r + 1)) return GAN_E_SHAPE;
      if ((d->stages & GAN_PRE_SHARPEN) && (g.height < 2 || g.width < 2)) return GAN_E_SHAPE;
      if ((int64_t)(g.height - 1) * g.pitch + (int64_t)g.width * d->c >= (1LL << 31)) return GAN_E_SHAPE;
      if (d->stages & (GAN_PRE_BLUR | GAN_PRE_SHARPEN)) bytes += pre_align16((size_t)g.height * (((size_t)g.width * d->c + 3) & ~(size_t)3));
    }
    worst = bytes > worst ? bytes : worst;
  }
  *need = worst < 16 ? 16 : worst;
  return 0;
}

size_t gan_preprocess_workspace_bytes(const GanPreprocessDesc* d) {
  size_t need = 0;
  return pre_validate(d, &need) == 0 ? need : 0;
}

template <int MODE>
static int pre_stencil_launch(PreArgs& a, int to_buf, dim3 grid, hipStream_t stream) {
  a.to_buf = to_buf;
  GAN_LAUNCH(pre_stencil_kernel<MODE>, grid, dim3(256), 0, stream, a);
  GAN_CHECK_LAUNCH();
  return 0;
}

int gan_preprocess_u8(const GanPreprocessDesc* d, gan_stream_t stream) {
  size_t need = 0;
  const int rc = pre_validate(d, &need);
  if (rc) return rc;
  if (!d->src || !d->workspace || ((uintptr_t)d->workspace & 15) || d->src_bytes < 1) return GAN_E_ARG;
  for (int i = 0; i < d->n; ++i) {
    const GanPreRegion& g = d->regions[i];
    if (g.src_offset + (int64_t)(g.height - 1) * g.pitch + (int64_t)g.width * d->c > d->src_bytes) return GAN_E_ARG;
  }
  if (d->workspace_bytes < need) return GAN_E_WORKSPACE;
  const bool clahe = d->stages & GAN_PRE_CLAHE, blur = d->stages & GAN_PRE_BLUR, sharpen = d->stages & GAN_PRE_SHARPEN;
  hipStream_t s = (hipStream_t)stream;
  PreArgs a;
  a.buf = d->src; a.c = d->c; a.grid = clahe ? d->grid : 1; a.r = 0; a.to_buf = 0;
  for (int i = 0; i < 6; ++i) a.q[i] = 0;
  if (blur) {
    a.r = pre_blur_radius((double)d->sigma);
    pre_blur_taps((double)d->sigma, a.r, a.q);
  }
  for (int lo = 0; lo < d->n; lo += GAN_PREPROCESS_MAX_REGIONS) {
    const int m = d->n - lo < GAN_PREPROCESS_MAX_REGIONS ? d->n - lo : GAN_PREPROCESS_MAX_REGIONS;
    const size_t lut_bytes = clahe ? pre_align16((size_t)m * d->c * d->grid * d->grid * 256) : 0;
    a.lut = (uint8_t*)d->workspace;
    a.scratch = (uint8_t*)d->workspace + lut_bytes;
    size_t at = 0;
    int th_max = 1, h_max = 1, nb_max = 1;
    for (int i = 0; i < m; ++i) {
      const GanPreRegion& g = d->regions[lo + i];
      PreRegionDev& o = a.g[i];
      o.off = g.src_offset; o.pitch = g.pitch; o.h = g.height; o.w = g.width;
      o.spitch = (g.width * d->c + 3) & ~3;
      o.scratch = (long long)at;
      if (blur || sharpen) at += pre_align16((size_t)g.height * o.spitch);
      o.tw = (g.width + a.grid - 1) / a.grid; o.th = (g.height + a.grid - 1) / a.grid;
      const int area = o.tw * o.th;
      const double lim = (double)d->clip * area / 256.0;         // (a limit of `area` or more clips nothing)
      o.limit = d->clip > 0.f ? (lim >= area ? area : lim >= 1.0 ? (int)lim : 1) : 0x7fffffff;
      o.scale = (float)(255.0 / area);
      o.inv_tw = 1.0f / (float)o.tw; o.inv_th = 1.0f / (float)o.th;
      th_max = o.th > th_max ? o.th : th_max;
      h_max = g.height > h_max ? g.height : h_max;
      nb_max = g.width * d->c > nb_max ? g.width * d->c : nb_max;
    }
    for (int i = m; i < GAN_PREPROCESS_MAX_REGIONS; ++i) a.g[i] = a.g[0];
    if (clahe) {
      GAN_LAUNCH(pre_lut_kernel, dim3((unsigned)(a.grid * a.grid), (unsigned)d->c, (unsigned)m), dim3(256), 0, s, a);
      GAN_CHECK_LAUNCH();
      const int nsub = (th_max + 3 + PRE_APPLY_ROWS - 1) / PRE_APPLY_ROWS;
      const size_t lds = (size_t)2 * d->c * a.grid * 256;
      const int staged = lds <= (size_t)PRE_LUT_LDS;
      const dim3 grid((unsigned)((a.grid + 1) * nsub), (unsigned)m);
      if (d->c == 1)
        GAN_LAUNCH(pre_apply_kernel<1>, grid, dim3(256), staged ? lds : 0, s, a, nsub, staged);
      else
        GAN_LAUNCH(pre_apply_kernel<3>, grid, dim3(256), staged ? lds : 0, s, a, nsub, staged);
      GAN_CHECK_LAUNCH();
    }
    if (blur || sharpen) {
      const dim3 grid((unsigned)((nb_max + PRE_TW - 1) / PRE_TW), (unsigned)((h_max + PRE_TH - 1) / PRE_TH), (unsigned)m);
      int e;
      if (blur && sharpen) {
        if ((e = pre_stencil_launch<PRE_BLUR>(a, 0, grid, s))) return e;
        if ((e = pre_stencil_launch<PRE_SHARPEN>(a, 1, grid, s))) return e;
      } else {
        if ((e = pre_stencil_launch<PRE_COPY>(a, 0, grid, s))) return e;
        if ((e = blur ? pre_stencil_launch<PRE_BLUR>(a, 1, grid, s) : pre_stencil_launch<PRE_SHARPEN>(a, 1, grid, s))) return e;
      }
    }
  }
  return 0;
}
