// Structural dissimilarity as a generator loss (include/gan_amd.h: gan_dssim): loss = 1 - mean SSIM with SSIM
// exactly as quality.hip computes it (ssim_window.h: same window, constants, centred moments, rounding discipline), and the
// gradient with respect to the prediction a.
//
// Two launches.  dssim_tile_kernel: one workgroup per (image, 32 x 32 tile of PIXELS).  A pixel p takes part in the map positions
// q = p - 10 .. p per axis, and a map position reads the pixels q .. q + 10: the tile's gradient depends on the 42 x 42 positions
// from (y0 - 10, x0 - 10) on and those on the 52 x 52 pixels from the same origin.  Per real channel the workgroup stages these pixels
// of both images in LDS as centred values x' = 0.5 * x (zero outside the image), filters the four maps x', y', x'y', x'^2 + y'^2 along
// the rows and the columns as quality.hip does, forms at every position of the valid map the three derivative maps
//   P = dS/dF(x'),  Q = dS/dF(x'y'),  R = dS/dF(x'^2 + y'^2)
// (zero at positions outside the valid map, so they drop out of G^T), runs the transposed separable filter back to its 32 x 32
// pixels and writes da = coef * (G^T[P] + y' G^T[Q] + 2 x' G^T[R]) once per pixel it owns.  It also adds S over the map positions it
// owns - the 32 x 32 block with the tile's own origin, clipped to the map - so that every position counts exactly once, and writes
// one fp32 partial to workspace[image][tile].  dssim_finalize_kernel adds the partials in a fixed order in double and forms
// 1 - mean.  No atomics.
//
// The derivatives are taken in the CENTRED variables (the +0.5 moves neither a variance nor a derivative with respect to a pixel):
// with lum = A1 / B1 and cs = A2 / B2
//   P = (2 cs / B1) (my - lum mx) - (2 lum / B2) (mb - cs ma),   Q = 2 lum / B2,   R = -lum cs / B2.
// This is the header's P, Q, R regrouped (mx = ma + 0.5): each bracket is a difference of like quantities instead of a difference
// of two large quotients, and for a == b (lum = cs = 1, ma = mb) P is exactly 0 and Q = -2 R, so the gradient is exactly 0.
//
// LDS: the staged pixels (2 x 52 x 52) are dead after the row pass and hold P, Q, R (3 x 42 x 42) afterwards; the row-filtered maps
// (4 x 52 x 42) are dead after the column pass and hold the row-transposed maps (3 x 42 x 32): 56.6 KB in all.
#include "common.h"
#include "ssim_window.h"

namespace {

constexpr int DT = 32;                  // tile edge in pixels
constexpr int DK = SSIM_K;
constexpr int DM = DT + DK - 1;         // map positions per axis a tile's gradient depends on: 42
constexpr int DS = DM + DK - 1;         // staged pixels per axis: 52
constexpr int DTHREADS = 256;
constexpr int DPIX = DT * DT / DTHREADS;   // owned pixels per thread: 4

struct DssimArgs {
  const void* a;
  const void* b;
  void* da;                             // NULL: loss only
  int pitch_a, pitch_b, pitch_da, dtype_da;
  int n, h, w, c;
  int tiles_x, tiles_y;
  float g[DK];
  float coef;                           // -0.5 * grad_scale / (c |M|): the batch-1 coefficient
  float batch;                          // n: da = (coef * v) / n, so an image's gradient is its batch-1 gradient divided by n, rounded once
  const float* ls;                      // loss-scale state or NULL
  float* partial;                       // [n][tiles_y * tiles_x]: sum of S over the map positions the tile owns
};

__device__ __forceinline__ void st_any(void* p, long long i, int dtype, float v) {
  if (dtype == GAN_F32) ((float*)p)[i] = v;
  else if (dtype == GAN_BF16) ((bf16_t*)p)[i] = (bf16_t)v;
  else ((f16_t*)p)[i] = (f16_t)v;
}

template <typename TA, typename TB>
__global__ __launch_bounds__(DTHREADS) void dssim_tile_kernel(const DssimArgs q) {
  __shared__ float s_in[2 * DS * DS];            // staged x', y'; then P, Q, R
  __shared__ float s_hm[4 * DS * DM];            // row-filtered maps; then the row-transposed P, Q, R
  __shared__ float red[DTHREADS / 64];
  float (*sa)[DS] = reinterpret_cast<float (*)[DS]>(s_in);
  float (*sb)[DS] = reinterpret_cast<float (*)[DS]>(s_in + DS * DS);
  float (*pqr)[DM][DM] = reinterpret_cast<float (*)[DM][DM]>(s_in);         // 3 * 42 * 42 <= 2 * 52 * 52
  float (*hm)[DS][DM] = reinterpret_cast<float (*)[DS][DM]>(s_hm);
  float (*tr)[DM][DT] = reinterpret_cast<float (*)[DM][DT]>(s_hm);          // 3 * 42 * 32 <= 4 * 52 * 42
  static_assert(3 * DM * DM <= 2 * DS * DS && 3 * DM * DT <= 4 * DS * DM, "aliased LDS regions");
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const int ty = tile / q.tiles_x, tx = tile - ty * q.tiles_x;
  const int y0 = ty * DT, x0 = tx * DT;                            // first pixel of the tile = first map position it owns
  const int py0 = y0 - (DK - 1), px0 = x0 - (DK - 1);              // origin of the staged pixels and of the 42 x 42 positions
  const int mh = q.h - (DK - 1), mw = q.w - (DK - 1);              // SSIM map size
  const bool grad = q.da != nullptr;
  const float coef = q.ls ? q.coef * q.ls[0] : q.coef;
  const TA* A = (const TA*)q.a;
  const TB* B = (const TB*)q.b;
  for (int img = blockIdx.y; img < q.n; img += gridDim.y) {
    float s_ssim = 0.f;
    for (int ch = 0; ch < q.c; ++ch) {
      __syncthreads();                                             // the previous channel's (image's) readers are done
      for (int i = tid; i < DS * DS; i += DTHREADS) {
        const int r = i / DS, x = i - r * DS;
        const int gy = py0 + r, gx = px0 + x;
        float va = 0.f, vb = 0.f;
        if (gy >= 0 && gy < q.h && gx >= 0 && gx < q.w) {
          const long long pix = ((long long)img * q.h + gy) * q.w + gx;
          va = 0.5f * ld_f(A + pix * q.pitch_a + ch);
          vb = 0.5f * ld_f(B + pix * q.pitch_b + ch);
        }
        sa[r][x] = va;
        sb[r][x] = vb;
      }
      __syncthreads();
      float own_a[DPIX], own_b[DPIX];                              // x', y' at the pixels this thread writes
#pragma unroll
      for (int j = 0; j < DPIX; ++j) {
        const int i = tid + j * DTHREADS, r = i / DT, x = i - r * DT;
        own_a[j] = sa[r + DK - 1][x + DK - 1];
        own_b[j] = sb[r + DK - 1][x + DK - 1];
      }
      for (int i = tid; i < DS * DM; i += DTHREADS) {              // along the rows
        const int r = i / DM, x = i - r * DM;
        float fa = 0.f, fb = 0.f, fab = 0.f, fsq = 0.f;
#pragma unroll
        for (int k = 0; k < DK; ++k) {
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
      __syncthreads();                                             // (the staged pixels are dead from here: pqr takes their place)
      for (int i = tid; i < DM * DM; i += DTHREADS) {              // along the columns, then S and its derivatives
        const int r = i / DM, x = i - r * DM;
        const int qy = py0 + r, qx = px0 + x;
        float P = 0.f, Q = 0.f, R = 0.f;
        if (qy >= 0 && qy < mh && qx >= 0 && qx < mw) {
          float ma = 0.f, mb = 0.f, eab = 0.f, esq = 0.f;
#pragma unroll
          for (int k = 0; k < DK; ++k) {
            const float wk = q.g[k];
            ma = fmaf(wk, hm[0][r + k][x], ma);
            mb = fmaf(wk, hm[1][r + k][x], mb);
            eab = fmaf(wk, hm[2][r + k][x], eab);
            esq = fmaf(wk, hm[3][r + k][x], esq);
          }
          const SsimTerms t = ssim_terms(ma, mb, eab, esq);
          if (r >= DK - 1 && x >= DK - 1) s_ssim += q_mul(t.lum, t.cs);     // the positions this tile owns
          const float il = 2.f / t.lum_d, ic = 2.f / t.cs_d;
          const float dl = q_mul(q_mul(t.cs, il), q_sub(t.my, q_mul(t.lum, t.mx)));
          const float dc = q_mul(q_mul(t.lum, ic), q_sub(mb, q_mul(t.cs, ma)));
          P = q_sub(dl, dc);
          Q = q_mul(t.lum, ic);
          R = -0.5f * q_mul(t.cs, Q);
        }
        if (grad) {
          pqr[0][r][x] = P;
          pqr[1][r][x] = Q;
          pqr[2][r][x] = R;
        }
      }
      if (!grad) continue;                                         // (uniform over the workgroup)
      __syncthreads();                                             // (the row-filtered maps are dead from here: tr takes their place)
      for (int i = tid; i < DM * DT; i += DTHREADS) {              // transposed filter along the rows: pixel column x <- positions x + 10 - k
        const int r = i / DT, x = i - r * DT;
        float tp = 0.f, tq = 0.f, tr_ = 0.f;
#pragma unroll
        for (int k = 0; k < DK; ++k) {
          const float wk = q.g[k];
          tp = fmaf(wk, pqr[0][r][x + DK - 1 - k], tp);
          tq = fmaf(wk, pqr[1][r][x + DK - 1 - k], tq);
          tr_ = fmaf(wk, pqr[2][r][x + DK - 1 - k], tr_);
        }
        tr[0][r][x] = tp;
        tr[1][r][x] = tq;
        tr[2][r][x] = tr_;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < DPIX; ++j) {                             // along the columns: pixel row r <- positions r + 10 - k; then the pixel
        const int i = tid + j * DTHREADS, r = i / DT, x = i - r * DT;
        const int gy = y0 + r, gx = x0 + x;
        if (gy >= q.h || gx >= q.w) continue;
        float gp = 0.f, gq = 0.f, gr = 0.f;
#pragma unroll
        for (int k = 0; k < DK; ++k) {
          const float wk = q.g[k];
          gp = fmaf(wk, tr[0][r + DK - 1 - k][x], gp);
          gq = fmaf(wk, tr[1][r + DK - 1 - k][x], gq);
          gr = fmaf(wk, tr[2][r + DK - 1 - k][x], gr);
        }
        // y' G^T[Q] and 2 x' G^T[R] rounded on their own: for a == b they are equal and opposite
        const float v = q_add(gp, q_add(q_mul(own_b[j], gq), q_mul(q_mul(2.f, own_a[j]), gr)));
        const long long pix = ((long long)img * q.h + gy) * q.w + gx;
        st_any(q.da, pix * q.pitch_da + ch, q.dtype_da, q_mul(coef, v) / q.batch);
      }
    }
    // fixed-order workgroup sum: butterfly inside each wave, then the four wave sums in order
    s_ssim = wave_sum(s_ssim);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = s_ssim;
    __syncthreads();
    if (tid == 0) q.partial[(long long)img * (q.tiles_x * q.tiles_y) + tile] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

__global__ __launch_bounds__(DTHREADS) void dssim_finalize_kernel(const float* partial, long long count, double map_count, float loss_scale,
                                                                 int acc, float* loss_out) {
  __shared__ double red[DTHREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (long long t = tid; t < count; t += DTHREADS) s += (double)partial[t];
  red[tid] = s;
  __syncthreads();
  for (int o = DTHREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float t = (float)(1.0 - red[0] / map_count) * loss_scale;
    loss_out[0] = acc ? loss_out[0] + t : t;
  }
}

inline int d_tiles(int v) { return (v + DT - 1) / DT; }
inline bool d_shape_ok(int n, int h, int w, int c) {
  return n >= 1 && h >= DK && w >= DK && h <= SSIM_MAX_EDGE && w <= SSIM_MAX_EDGE && (c == 1 || c == 3);
}

template <typename TA> void launch_b(int dtype_b, const DssimArgs& q, dim3 grid, hipStream_t st) {
  switch (dtype_b) {
    case GAN_F32: GAN_LAUNCH((dssim_tile_kernel<TA, float>), grid, dim3(DTHREADS), 0, st, q); break;
    case GAN_BF16: GAN_LAUNCH((dssim_tile_kernel<TA, bf16_t>), grid, dim3(DTHREADS), 0, st, q); break;
    default: GAN_LAUNCH((dssim_tile_kernel<TA, f16_t>), grid, dim3(DTHREADS), 0, st, q); break;
  }
}

}  // namespace

extern "C" size_t gan_dssim_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c) {
  if (!d_shape_ok(n, h, w, c)) return 0;
  return (size_t)n * d_tiles(h) * d_tiles(w) * sizeof(float);
}

extern "C" int gan_dssim(const GanDssimDesc* d, gan_stream_t stream) {
  if (!d || d->struct_size != sizeof(GanDssimDesc)) return GAN_E_ARG;
  const GanTensor &a = d->a, &b = d->b, &da = d->da;
  if (!a.ptr || !b.ptr || !d->loss_out || !d->workspace) return GAN_E_ARG;
  if (!gan_dtype_ok(d->dtype_a) || !gan_dtype_ok(d->dtype_b)) return GAN_E_ARG;
  if (a.c != 1 && a.c != 3) return GAN_E_ARG;
  if (a.n != b.n || a.h != b.h || a.w != b.w || a.c != b.c) return GAN_E_ARG;
  if (a.n < 1 || a.pitch < a.c || b.pitch < b.c) return GAN_E_ARG;
  if (d->loss_accumulate != 0 && d->loss_accumulate != 1) return GAN_E_ARG;
  if (da.ptr) {
    if (!gan_dtype_ok(d->dtype_da)) return GAN_E_ARG;
    if (da.n != a.n || da.h != a.h || da.w != a.w || da.c != a.c || da.pitch < da.c) return GAN_E_ARG;
  }
  if (a.h < DK || a.w < DK || a.h > SSIM_MAX_EDGE || a.w > SSIM_MAX_EDGE) return GAN_E_SHAPE;
  if (d->workspace_bytes < gan_dssim_workspace_bytes(a.n, a.h, a.w, a.c)) return GAN_E_WORKSPACE;
  DssimArgs q;
  q.a = a.ptr; q.b = b.ptr; q.da = da.ptr;
  q.pitch_a = a.pitch; q.pitch_b = b.pitch; q.pitch_da = da.ptr ? da.pitch : 0; q.dtype_da = d->dtype_da;
  q.n = a.n; q.h = a.h; q.w = a.w; q.c = a.c;
  q.tiles_x = d_tiles(a.w); q.tiles_y = d_tiles(a.h);
  ssim_window(q.g);
  const double map_count = (double)a.n * a.c * (double)(a.h - (DK - 1)) * (a.w - (DK - 1));
  q.coef = (float)(-0.5 * (double)d->grad_scale / (map_count / a.n));
  q.batch = (float)a.n;
  q.ls = d->scale_state;
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
  GAN_LAUNCH(dssim_finalize_kernel, dim3(1), dim3(DTHREADS), 0, st, (const float*)d->workspace, (long long)a.n * tiles, map_count,
             d->loss_scale, d->loss_accumulate, d->loss_out);
  GAN_CHECK_LAUNCH();
  return 0;
}
