// Image-quality metrics of a batch of image pairs (include/gan_amd.h: gan_image_quality): SSIM as tf.image.ssim defines it
// (11-tap Gaussian, sigma 1.5, VALID padding, k1 0.01, k2 0.03, max_val 1), PSNR, mean absolute and mean squared error, all on the
// display range u = 0.5 * x + 0.5.  No counterpart in the reference's training loop: its only use of tf.image.ssim compares the
// input with the target (pix2pix.py:182-184).
//
// Two launches.  quality_tile_kernel: one workgroup per (image, 32 x 32 tile of the SSIM map).  Per real channel it stages the
// 42 x 42 pixels under the tile of both images in LDS as CENTRED values x' = 0.5 * x (u = x' + 0.5), filters the four maps the
// definition needs - x', y', x'y', x'^2 + y'^2 - along the rows into LDS and along the columns into registers, and adds lum * cs over
// the tile's positions; |x' - y'| and (x' - y')^2 are added over the pixels the tile OWNS (its 32 x 32 origin block; the last tile
// of a row / column also owns the pixels up to the image edge), so every pixel and every map position counts exactly once.  The
// three fp32 sums go to workspace[image][tile].  quality_finalize_kernel: one workgroup per image adds the tile sums in a fixed
// order (double) and writes {ssim, psnr, mae, mse}.  No atomics: the result is bit-identical from call to call and an image's row
// does not depend on the rest of the batch.
//
// Centring: covariance and variance do not move with the +0.5, so F(x'y') - F(x')F(y') and F(x'^2 + y'^2) - F(x')^2 - F(y')^2 are
// the definition's second moments with operands of a quarter of the magnitude (|x'| <= 0.5 against u <= 1): less cancellation where
// it hurts, on bright flat images, at no cost.  Only the luminance term needs the means themselves: mx = F(x') + 0.5.
#include "common.h"
#include "ssim_window.h"

namespace {

constexpr int QT = 32;            // tile edge of the SSIM map
constexpr int QK = SSIM_K;        // filter taps (ssim_window.h: the window, c1, c2 and the rounding discipline, shared with dssim.hip)
constexpr int QS = QT + QK - 1;   // staged edge: 42
constexpr int QTHREADS = 256;

struct QualityArgs {
  const void* a;
  const void* b;
  int pitch_a, pitch_b;
  int n, h, w, c;
  int tiles_x, tiles_y;
  float g[QK];                    // Gaussian window, normalised in double on the host
  float* partial;                 // [n][tiles_y * tiles_x][4]: {sum lum*cs, sum |x'-y'|, sum (x'-y')^2, 0}
};

template <typename TA, typename TB>
__global__ __launch_bounds__(QTHREADS) void quality_tile_kernel(const QualityArgs q) {
  __shared__ float sa[QS][QS];
  __shared__ float sb[QS][QS];
  __shared__ float hm[4][QS][QT];       // row-filtered x', y', x'y', x'^2 + y'^2
  __shared__ float red[3][QTHREADS / 64];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const int ty = tile / q.tiles_x, tx = tile - ty * q.tiles_x;
  const int y0 = ty * QT, x0 = tx * QT;
  const int mh = q.h - (QK - 1), mw = q.w - (QK - 1);              // SSIM map size
  const int vy = min(QT, mh - y0), vx = min(QT, mw - x0);          // map positions of this tile (>= 1)
  const int sy = vy + QK - 1, sx = vx + QK - 1;                    // staged pixels that exist: y0 + sy <= h, x0 + sx <= w
  // pixels this tile owns for MAE / MSE: its origin block, and up to the image edge for the last tile of a row / column
  const int oy = (ty == q.tiles_y - 1) ? sy : QT, ox = (tx == q.tiles_x - 1) ? sx : QT;
  const TA* A = (const TA*)q.a;
  const TB* B = (const TB*)q.b;
  for (int img = blockIdx.y; img < q.n; img += gridDim.y) {
    float s_ssim = 0.f, s_abs = 0.f, s_sq = 0.f;
    for (int ch = 0; ch < q.c; ++ch) {
      __syncthreads();                                             // the previous channel's (image's) readers are done
      for (int i = tid; i < QS * QS; i += QTHREADS) {
        const int r = i / QS, x = i - r * QS;
        float va = 0.f, vb = 0.f;
        if (r < sy && x < sx) {
          const long long pix = ((long long)img * q.h + (y0 + r)) * q.w + (x0 + x);
          va = 0.5f * ld_f(A + pix * q.pitch_a + ch);
          vb = 0.5f * ld_f(B + pix * q.pitch_b + ch);
          if (r < oy && x < ox) {
            const float df = q_sub(va, vb);
            s_abs += fabsf(df);
            s_sq = fmaf(df, df, s_sq);
          }
        }
        sa[r][x] = va;
        sb[r][x] = vb;
      }
      __syncthreads();
      for (int i = tid; i < QS * QT; i += QTHREADS) {              // along the rows
        const int r = i / QT, x = i - r * QT;
        float fa = 0.f, fb = 0.f, fab = 0.f, fsq = 0.f;
#pragma unroll
        for (int k = 0; k < QK; ++k) {
          const float va = sa[r][x + k], vb = sb[r][x + k], wk = q.g[k];
          fa = fmaf(wk, va, fa);
          fb = fmaf(wk, vb, fb);
          fab = fmaf(wk, q_mul(va, vb), fab);
          fsq = fmaf(wk, q_add(q_mul(va, va), q_mul(vb, vb)), fsq);
        }
        hm[0][r][x] = fa;
        hm[1][r][x] = fb;
        hm[2][r][x] = fab;
        hm[3][r][x] = fsq;
      }
      __syncthreads();
      for (int i = tid; i < QT * QT; i += QTHREADS) {              // along the columns, then the index itself
        const int r = i / QT, x = i - r * QT;
        if (r >= vy || x >= vx) continue;
        float ma = 0.f, mb = 0.f, eab = 0.f, esq = 0.f;
#pragma unroll
        for (int k = 0; k < QK; ++k) {
          const float wk = q.g[k];
          ma = fmaf(wk, hm[0][r + k][x], ma);
          mb = fmaf(wk, hm[1][r + k][x], mb);
          eab = fmaf(wk, hm[2][r + k][x], eab);
          esq = fmaf(wk, hm[3][r + k][x], esq);
        }
        const SsimTerms t = ssim_terms(ma, mb, eab, esq);
        s_ssim += q_mul(t.lum, t.cs);
      }
    }
    // fixed-order workgroup sum: butterfly inside each wave, then the four wave sums in order
    s_ssim = wave_sum(s_ssim);
    s_abs = wave_sum(s_abs);
    s_sq = wave_sum(s_sq);
    __syncthreads();
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = s_ssim;
      red[1][tid >> 6] = s_abs;
      red[2][tid >> 6] = s_sq;
    }
    __syncthreads();
    if (tid == 0) {
      float* p = q.partial + ((long long)img * (q.tiles_x * q.tiles_y) + tile) * 4;
#pragma unroll
      for (int j = 0; j < 3; ++j) p[j] = ((red[j][0] + red[j][1]) + red[j][2]) + red[j][3];
      p[3] = 0.f;
    }
  }
}

__global__ __launch_bounds__(QTHREADS) void quality_finalize_kernel(const float* partial, int tiles, double map_count, double pix_count,
                                                                   float* out) {
  __shared__ double red[3][QTHREADS];
  const int tid = threadIdx.x;
  const float* p = partial + (long long)blockIdx.x * tiles * 4;
  double s[3] = {0.0, 0.0, 0.0};
  for (int t = tid; t < tiles; t += QTHREADS)
    for (int j = 0; j < 3; ++j) s[j] += (double)p[(long long)t * 4 + j];
  for (int j = 0; j < 3; ++j) red[j][tid] = s[j];
  __syncthreads();
  for (int o = QTHREADS / 2; o > 0; o >>= 1) {
    if (tid < o)
      for (int j = 0; j < 3; ++j) red[j][tid] += red[j][tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    float* o = out + (long long)blockIdx.x * 4;
    const double mae = red[1][0] / pix_count, mse = red[2][0] / pix_count;       // x' - y' = u_a - u_b
    o[0] = (float)(red[0][0] / map_count);
    o[1] = (float)(-10.0 * log10(mse));         // +inf for an exact match
    o[2] = (float)mae;
    o[3] = (float)mse;
  }
}

inline int q_tiles(int v) { return (v - (QK - 1) + QT - 1) / QT; }
inline bool q_shape_ok(int n, int h, int w, int c) { return n >= 1 && h >= QK && w >= QK && h <= 4096 && w <= 4096 && (c == 1 || c == 3); }

template <typename TA> int launch_b(int dtype_b, const QualityArgs& q, dim3 grid, hipStream_t st) {
  switch (dtype_b) {
    case GAN_F32: GAN_LAUNCH((quality_tile_kernel<TA, float>), grid, dim3(QTHREADS), 0, st, q); break;
    case GAN_BF16: GAN_LAUNCH((quality_tile_kernel<TA, bf16_t>), grid, dim3(QTHREADS), 0, st, q); break;
    default: GAN_LAUNCH((quality_tile_kernel<TA, f16_t>), grid, dim3(QTHREADS), 0, st, q); break;
  }
  return 0;
}

}  // namespace

extern "C" size_t gan_image_quality_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c) {
  if (!q_shape_ok(n, h, w, c)) return 0;
  return (size_t)n * q_tiles(h) * q_tiles(w) * 4 * sizeof(float);
}

extern "C" int gan_image_quality(const GanQualityDesc* d, gan_stream_t stream) {
  if (!d || d->struct_size != sizeof(GanQualityDesc)) return GAN_E_ARG;
  const GanTensor &a = d->a, &b = d->b;
  if (!a.ptr || !b.ptr || !d->out || !d->workspace) return GAN_E_ARG;
  if (!gan_dtype_ok(d->dtype_a) || !gan_dtype_ok(d->dtype_b)) return GAN_E_ARG;
  if (a.c != 1 && a.c != 3) return GAN_E_ARG;
  if (a.n != b.n || a.h != b.h || a.w != b.w || a.c != b.c) return GAN_E_ARG;
  if (a.n < 1 || a.pitch < a.c || b.pitch < b.c) return GAN_E_ARG;
  if (a.h < QK || a.w < QK || a.h > 4096 || a.w > 4096) return GAN_E_SHAPE;
  if (d->workspace_bytes < gan_image_quality_workspace_bytes(a.n, a.h, a.w, a.c)) return GAN_E_WORKSPACE;
  QualityArgs q;
  q.a = a.ptr; q.b = b.ptr; q.pitch_a = a.pitch; q.pitch_b = b.pitch;
  q.n = a.n; q.h = a.h; q.w = a.w; q.c = a.c;
  q.tiles_x = q_tiles(a.w); q.tiles_y = q_tiles(a.h);
  ssim_window(q.g);
  q.partial = (float*)d->workspace;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = q.tiles_x * q.tiles_y;
  const dim3 grid(tiles, a.n < 65535 ? a.n : 65535);
  switch (d->dtype_a) {
    case GAN_F32: launch_b<float>(d->dtype_b, q, grid, st); break;
    case GAN_BF16: launch_b<bf16_t>(d->dtype_b, q, grid, st); break;
    default: launch_b<f16_t>(d->dtype_b, q, grid, st); break;
  }
  GAN_CHECK_LAUNCH();
  const double map_count = (double)(a.h - (QK - 1)) * (a.w - (QK - 1)) * a.c, pix_count = (double)a.h * a.w * a.c;
  GAN_LAUNCH(quality_finalize_kernel, dim3(a.n), dim3(QTHREADS), 0, st, (const float*)d->workspace, tiles, map_count, pix_count, d->out);
  GAN_CHECK_LAUNCH();
  return 0;
}
