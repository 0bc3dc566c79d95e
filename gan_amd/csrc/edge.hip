// Sobel edge term of the generator loss (include/gan_amd.h: gan_edge_l1): the mean absolute Sobel response of
// d = a - b over the valid positions, and its gradient with respect to the prediction a.
//
//   ex(q) = (Sx * d)(q) / 8,  ey(q) = (Sy * d)(q) / 8,  Sx = [[-1,0,1],[-2,0,2],[-1,0,1]], Sy = Sx^T (correlation), 1 <= q <= size - 2
//   loss = sum (|ex| + |ey|) / (2 n c M),  M = (h - 2)(w - 2)
//   dloss/da(p) = k(p) / (16 n c M),  k(p) = sum over the valid q, |q - p|_inf <= 1, of Sx(p - q) sgn(ex(q)) + Sy(p - q) sgn(ey(q))
// k is an integer in [-16, 16] (sgn(0) = 0).  Rounding order of the gradient: g = (float(k) * F) / float(n) with the one precomputed
// factor F = (float)(grad_scale / (16 c M)) (the batch-1 coefficient, computed on the host in double), then g * scale_state[0] when
// given - every operation rounded to fp32 on its own, never fused - and da = dtype_da(g) or, grad_accumulate,
// dtype_da(float(da_old) + g): one fp32 addition, one rounding to the storage type.  The division by n keeps an image's gradient at
// batch n within half an ulp of its batch-1 gradient / n, as gan_dssim does; a factor with n folded in does not (up to 2 ulps).
//
// Two launches.  edge_tile_kernel: one workgroup per (image, 32 x 32 tile of PIXELS).  A pixel p takes part in the positions
// p - 1 .. p + 1 per axis and a position reads the pixels q - 1 .. q + 1: the tile's gradient depends on the 34 x 34 positions from
// (y0 - 1, x0 - 1) on and those on the 36 x 36 pixels from (y0 - 2, x0 - 2) on.  The workgroup stages d of these pixels for all real
// channels in LDS (zero outside the image: no valid position reads those), forms sgn(ex), sgn(ey) at the 34 x 34 positions (both
// zero at positions outside the valid map, so they drop out of k) packed into one word, and every thread then forms k at the four
// pixels it owns and writes - or reads, adds to and writes - their da elements once, channel by channel: only the c real channels
// may change, and a 16-byte store would have to read the pad channels first, which another launch may be filling.  A pixel of a or b
// that is one aligned 16-byte unit (the step's bf16 / fp16 buffers of pitch 8, fp32 of pitch 4) is fetched with one 16-byte load.
// The workgroup also adds |ex| + |ey| over the positions it owns - those on its own 32 x 32 pixels - so that every position counts
// once, and writes one fp32 partial to workspace[image][tile].  edge_finalize_kernel adds the partials in a fixed order in double.
// No atomics; every wave reaches every barrier (no thread leaves early: the guards are on the work, not on the thread).
//
// LDS: d 3 x 36 x 36 floats + signs 3 x 34 x 34 words = 29.4 KB.  ds_read_b32 / ds_write_b32 bank over 32-lane halves: a half reads
// 32 consecutive dwords of a row (or two runs around a row break), conflict-free up to the two lanes at a break.
#include "common.h"

namespace {

constexpr int ET = 32;                  // tile edge in pixels
constexpr int EM = ET + 2;              // positions per axis a tile's gradient depends on: 34
constexpr int ES = EM + 2;              // staged pixels per axis: 36
constexpr int EC = 3;                   // channels at most
constexpr int ETHREADS = 256;
constexpr int EPIX = ET * ET / ETHREADS;   // owned pixels per thread: 4

struct EdgeArgs {
  const void* a;
  const void* b;
  void* da;                             // NULL: loss only
  int pitch_a, pitch_b, pitch_da, dtype_da;
  int n, h, w, c;
  int tiles_x, tiles_y;
  int vec_a, vec_b;                     // a pixel of a / b is one aligned 16-byte unit
  int acc;                              // grad_accumulate
  float factor;                         // F = grad_scale / (16 c M): the batch-1 coefficient
  float batch;                          // n: g = (float(k) * F) / n
  const float* ls;                      // loss-scale state or NULL
  float* partial;                       // [n][tiles_y * tiles_x]: sum of |ex| + |ey| over the positions the tile owns
};

// products and sums that must be rounded on their own (the default contraction would fuse them into the operation that follows)
__device__ __forceinline__ float e_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float e_div(float x, float y) {
#pragma clang fp contract(off)
  return x / y;
}
__device__ __forceinline__ float e_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}

__device__ __forceinline__ float ld_any(const void* p, long long i, int dtype) {
  if (dtype == GAN_F32) return ((const float*)p)[i];
  if (dtype == GAN_BF16) return (float)((const bf16_t*)p)[i];
  return (float)((const f16_t*)p)[i];
}
__device__ __forceinline__ void st_any(void* p, long long i, int dtype, float v) {
  if (dtype == GAN_F32) ((float*)p)[i] = v;
  else if (dtype == GAN_BF16) ((bf16_t*)p)[i] = (bf16_t)v;
  else ((f16_t*)p)[i] = (f16_t)v;
}

// the c real channels of one pixel -> out[0 .. c); out[c ..] is not meaningful
template <typename T> __device__ __forceinline__ void ld_pixel(const T* p, int c, bool vec, float* out) {
  if (vec) {
    float f[VecOf<T>::N];
    unpack16<T>(*(const uint4*)p, f);
    out[0] = f[0]; out[1] = f[1]; out[2] = f[2];
  } else {
#pragma unroll
    for (int ch = 0; ch < EC; ++ch)
      if (ch < c) out[ch] = ld_f(p + ch);
  }
}

__device__ __forceinline__ int sgn(float v) { return (v > 0.f) - (v < 0.f); }

template <typename TA, typename TB>
__global__ __launch_bounds__(ETHREADS) void edge_tile_kernel(const EdgeArgs q) {
  __shared__ float s_d[EC][ES][ES];              // d = a - b at the staged pixels
  __shared__ int s_sg[EC][EM][EM];               // sgn(ex) in the low half, sgn(ey) in the high half
  __shared__ float red[ETHREADS / 64];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const int ty = tile / q.tiles_x, tx = tile - ty * q.tiles_x;
  const int y0 = ty * ET, x0 = tx * ET;                            // first pixel of the tile = first position it owns
  const bool grad = q.da != nullptr;
  const TA* A = (const TA*)q.a;
  const TB* B = (const TB*)q.b;
  for (int img = blockIdx.y; img < q.n; img += gridDim.y) {
    __syncthreads();                                               // the previous image's readers are done
    for (int i = tid; i < ES * ES; i += ETHREADS) {
      const int r = i / ES, x = i - r * ES;
      const int gy = y0 - 2 + r, gx = x0 - 2 + x;
      float va[EC] = {0.f, 0.f, 0.f}, vb[EC] = {0.f, 0.f, 0.f};
      if (gy >= 0 && gy < q.h && gx >= 0 && gx < q.w) {
        const long long pix = ((long long)img * q.h + gy) * q.w + gx;
        ld_pixel(A + pix * q.pitch_a, q.c, q.vec_a != 0, va);
        ld_pixel(B + pix * q.pitch_b, q.c, q.vec_b != 0, vb);
      }
#pragma unroll
      for (int ch = 0; ch < EC; ++ch)
        if (ch < q.c) s_d[ch][r][x] = va[ch] - vb[ch];
    }
    __syncthreads();
    float part = 0.f;
    for (int i = tid; i < EM * EM; i += ETHREADS) {                // position (r, x) of the 34 x 34: centre at staged (r + 1, x + 1)
      const int r = i / EM, x = i - r * EM;
      const int qy = y0 - 1 + r, qx = x0 - 1 + x;
      const bool valid = qy >= 1 && qy <= q.h - 2 && qx >= 1 && qx <= q.w - 2;
      const bool own = r >= 1 && r <= ET && x >= 1 && x <= ET;     // on the tile's own pixels
#pragma unroll
      for (int ch = 0; ch < EC; ++ch) {
        if (ch < q.c) {
          int code = 0;
          if (valid) {
            const float d00 = s_d[ch][r][x], d01 = s_d[ch][r][x + 1], d02 = s_d[ch][r][x + 2];
            const float d10 = s_d[ch][r + 1][x], d12 = s_d[ch][r + 1][x + 2];
            const float d20 = s_d[ch][r + 2][x], d21 = s_d[ch][r + 2][x + 1], d22 = s_d[ch][r + 2][x + 2];
            const float ex = 0.125f * ((d02 - d00) + 2.f * (d12 - d10) + (d22 - d20));
            const float ey = 0.125f * ((d20 - d00) + 2.f * (d21 - d01) + (d22 - d02));
            code = (sgn(ex) & 0xffff) | (int)((unsigned)sgn(ey) << 16);
            if (own) part += fabsf(ex) + fabsf(ey);
          }
          s_sg[ch][r][x] = code;
        }
      }
    }
    __syncthreads();
    if (grad) {                                                    // (uniform over the workgroup; no barrier inside)
      const float ls = q.ls ? q.ls[0] : 1.f;
#pragma unroll
      for (int j = 0; j < EPIX; ++j) {
        const int i = tid + j * ETHREADS, r = i / ET, x = i - r * ET;
        const int gy = y0 + r, gx = x0 + x;
        if (gy < q.h && gx < q.w) {
          const long long pix = ((long long)img * q.h + gy) * q.w + gx;
#pragma unroll
          for (int ch = 0; ch < EC; ++ch) {
            if (ch < q.c) {
              int k = 0;                                           // pixel p = position (r + 1, x + 1); q = p - u at (r + 1 - uy, x + 1 - ux)
#pragma unroll
              for (int uy = -1; uy <= 1; ++uy) {
#pragma unroll
                for (int ux = -1; ux <= 1; ++ux) {
                  if (uy == 0 && ux == 0) continue;
                  const int code = s_sg[ch][r + 1 - uy][x + 1 - ux];
                  const int sx = (int)(short)(code & 0xffff), sy = code >> 16;
                  k += ux * (2 - (uy < 0 ? -uy : uy)) * sx + uy * (2 - (ux < 0 ? -ux : ux)) * sy;     // Sx(u) sgn(ex) + Sy(u) sgn(ey)
                }
              }
              float g = e_div(e_mul((float)k, q.factor), q.batch);
              if (q.ls) g = e_mul(g, ls);
              const long long idx = pix * q.pitch_da + ch;
              if (q.acc) g = e_add(ld_any(q.da, idx, q.dtype_da), g);
              st_any(q.da, idx, q.dtype_da, g);
            }
          }
        }
      }
    }
    // fixed-order workgroup sum: butterfly inside each wave, then the four wave sums in order
    part = wave_sum(part);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) q.partial[(long long)img * (q.tiles_x * q.tiles_y) + tile] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

__global__ __launch_bounds__(ETHREADS) void edge_finalize_kernel(const float* partial, long long count, double denom, float loss_scale,
                                                                int acc, float* loss_out) {
  __shared__ double red[ETHREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (long long t = tid; t < count; t += ETHREADS) s += (double)partial[t];
  red[tid] = s;
  __syncthreads();
  for (int o = ETHREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float t = e_mul((float)(red[0] / denom), loss_scale);
    loss_out[0] = acc ? e_add(loss_out[0], t) : t;
  }
}

constexpr int EDGE_MAX = 4096;
inline int e_tiles(int v) { return (v + ET - 1) / ET; }
inline bool e_shape_ok(int n, int h, int w, int c) {
  return n >= 1 && h >= 3 && w >= 3 && h <= EDGE_MAX && w <= EDGE_MAX && (c == 1 || c == 3);
}
inline bool e_vec(const GanTensor& t, int dtype) {
  const size_t es = dtype == GAN_F32 ? 4 : 2;
  return (size_t)t.pitch * es == 16 && !((uintptr_t)t.ptr & 15);       // (c <= 3 < the unit's elements: the real channels lie inside)
}

template <typename TA> void launch_b(int dtype_b, const EdgeArgs& q, dim3 grid, hipStream_t st) {
  switch (dtype_b) {
    case GAN_F32: GAN_LAUNCH((edge_tile_kernel<TA, float>), grid, dim3(ETHREADS), 0, st, q); break;
    case GAN_BF16: GAN_LAUNCH((edge_tile_kernel<TA, bf16_t>), grid, dim3(ETHREADS), 0, st, q); break;
    default: GAN_LAUNCH((edge_tile_kernel<TA, f16_t>), grid, dim3(ETHREADS), 0, st, q); break;
  }
}

}  // namespace

extern "C" size_t gan_edge_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c) {
  if (!e_shape_ok(n, h, w, c)) return 0;
  return (size_t)n * e_tiles(h) * e_tiles(w) * sizeof(float);
}

extern "C" int gan_edge_l1(const GanEdgeDesc* d, gan_stream_t stream) {
  if (!d || d->struct_size != sizeof(GanEdgeDesc)) return GAN_E_ARG;
  const GanTensor &a = d->a, &b = d->b, &da = d->da;
  if (!a.ptr || !b.ptr || !d->loss_out || !d->workspace) return GAN_E_ARG;
  if (!gan_dtype_ok(d->dtype_a) || !gan_dtype_ok(d->dtype_b)) return GAN_E_ARG;
  if (a.c != 1 && a.c != 3) return GAN_E_ARG;
  if (a.n != b.n || a.h != b.h || a.w != b.w || a.c != b.c) return GAN_E_ARG;
  if (a.n < 1 || a.pitch < a.c || b.pitch < b.c) return GAN_E_ARG;
  if (d->loss_accumulate != 0 && d->loss_accumulate != 1) return GAN_E_ARG;
  if (d->grad_accumulate != 0 && d->grad_accumulate != 1) return GAN_E_ARG;
  if (da.ptr) {
    if (!gan_dtype_ok(d->dtype_da)) return GAN_E_ARG;
    if (da.n != a.n || da.h != a.h || da.w != a.w || da.c != a.c || da.pitch < da.c) return GAN_E_ARG;
  }
  if (a.h < 3 || a.w < 3 || a.h > EDGE_MAX || a.w > EDGE_MAX) return GAN_E_SHAPE;
  if (d->workspace_bytes < gan_edge_workspace_bytes(a.n, a.h, a.w, a.c)) return GAN_E_WORKSPACE;
  EdgeArgs q;
  q.a = a.ptr; q.b = b.ptr; q.da = da.ptr;
  q.pitch_a = a.pitch; q.pitch_b = b.pitch; q.pitch_da = da.ptr ? da.pitch : 0; q.dtype_da = d->dtype_da;
  q.n = a.n; q.h = a.h; q.w = a.w; q.c = a.c;
  q.tiles_x = e_tiles(a.w); q.tiles_y = e_tiles(a.h);
  q.vec_a = e_vec(a, d->dtype_a); q.vec_b = e_vec(b, d->dtype_b);
  q.acc = d->grad_accumulate;
  const double terms = (double)a.n * a.c * (double)(a.h - 2) * (a.w - 2);      // n c M
  q.factor = (float)((double)d->grad_scale / (16.0 * (terms / a.n)));
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
  GAN_LAUNCH(edge_finalize_kernel, dim3(1), dim3(ETHREADS), 0, st, (const float*)d->workspace, (long long)a.n * tiles, 2.0 * terms,
             d->loss_scale, d->loss_accumulate, d->loss_out);
  GAN_CHECK_LAUNCH();
  return 0;
}
