// Multi-scale structural dissimilarity as a generator loss (include/gan_amd.h: gan_msssim): per image and
// channel MS = prod_{j < M-1} max(CS_j, 0)^{w_j} * max(S_{M-1}, 0)^{w_{M-1}} over a pyramid of M levels, loss = 1 - mean, and the gradient
// with respect to the prediction a.  Every window operation is ssim_window.h's, so a level's lum and cs are the floats quality.hip
// and dssim.hip form on the same pixels.
//
// Level 0 is the stored image, read as the centred values x' = 0.5 * x; level j + 1 is the 2 x 2 mean of level j with the last row /
// column repeated where a side is odd, x_{j+1}(i, k) = 0.25 * ((x_j(2i, 2k) + x_j(2i, k1)) + (x_j(i1, 2k) + x_j(i1, k1))), formed in
// fp32 in that order by the same instructions for a and b (a == b stays a == b on every level).
//
// Launches, M levels, with gradient 2 M + 1, loss only M + 1:
//   M - 1  msssim_pool_kernel      level j -> level j + 1 of both images, planar fp32 [n][c][h_j][w_j] in the workspace
//   1      msssim_tile_kernel<.., false>  the statistics of ALL levels, driven by a tile table: one workgroup per (level, 32 x 32 tile,
//          image) stages 42 x 42 pixels per channel, filters the four maps as dssim.hip does and writes the fp32 sums of cs and of
//          lum * cs over the map positions it owns to workspace[level][image][channel][tile][2]
//   1      msssim_finalize_kernel  one wave per image adds the partials in a fixed order in double, forms CS_j, S_{M-1}, MS, the
//          per-image score, the coefficients k_j / |map_j| (0 where a factor was clamped) and, over all images in a fixed order, the
//          loss word
//   M      msssim_tile_kernel<.., true>   from the coarsest level down to level 0: dssim.hip's gradient scheme (52 x 52 staged pixels, 42 x 42
//          map positions, transposed separable filter back to the tile's 32 x 32 pixels) with P, Q, R of cs alone on the levels
//          below the last, G_j = k_j g_j + U(G_{j+1}) with U the exact transpose of the pooling read from the workspace; levels
//          above 0 write G_j to the workspace, level 0 writes (or updates) da once per element from its owner thread.
// No atomics; every sum has a fixed order: bit-identical from call to call.  Enqueue-only, capturable, allocates nothing.
//
// Derivatives in the centred variables (dssim.hip's header): with cs = A2 / B2 the maps of CS_j are
//   P = -(2 / B2) (mb - cs ma),   Q = 2 / B2,   R = -cs / B2 = -0.5 cs Q,
// for a == b (cs = 1, ma = mb) P is exactly 0 and R = -Q / 2, so g_j is exactly 0 on every level, and with it da.
//
// gfx950 build (-Rpass-analysis=kernel-resource-usage), all operand-type instances alike: statistics 35,648 B of LDS, 79 VGPRs;
// gradient 56,576 B (the staged pixels and the row-filtered maps are reused as in dssim.hip), 135 VGPRs; pooling no LDS, <= 32 VGPRs;
// finalize 32 B, 141 VGPRs; no scratch in any of them.
#include "common.h"
#include "ssim_window.h"

namespace {

constexpr int MT = 32;                  // tile edge in pixels
constexpr int MK = SSIM_K;
constexpr int MTHREADS = 256;
constexpr int MPIX = MT * MT / MTHREADS;   // owned pixels per thread: 4
constexpr int MAX_SCALES = 5;

struct MsLevel {
  int h, w;                             // pixels of the level
  int tiles_x, tiles_y;                 // 32 x 32 tiles of its pixels
  int tile_base;                        // first workgroup of the level in the statistics launch
  long long pyr;                        // floats from pyr_a / pyr_b / gws to the level's [n][c][h][w] (level 0: unused)
  long long part;                       // floats from partial to the level's [n][c][tiles][2]
};

struct MsArgs {
  const void* a;
  const void* b;
  void* da;                             // NULL: loss only
  int pitch_a, pitch_b, pitch_da, dtype_da;
  int n, c, scales;
  int level;                            // the level of a pool (source) or gradient launch
  int grad_acc;
  MsLevel lv[MAX_SCALES];
  float g[MK];
  float coef;                           // -0.5 * grad_scale / c: the batch-1 coefficient of G_0
  float batch;                          // n: da = (coef * G_0) / n
  const float* ls;                      // loss-scale state or NULL
  float* pyr_a;                         // pooled levels of a and b
  float* pyr_b;
  float* gws;                           // G_j of the levels above 0
  float* partial;
  float* kk;                            // [scales][n][c]: k_j / |map_j|
};

__device__ __forceinline__ void st_any(void* p, long long i, int dtype, float v) {
  if (dtype == GAN_F32) ((float*)p)[i] = v;
  else if (dtype == GAN_BF16) ((bf16_t*)p)[i] = (bf16_t)v;
  else ((f16_t*)p)[i] = (f16_t)v;
}
__device__ __forceinline__ float ld_any(const void* p, long long i, int dtype) {
  if (dtype == GAN_F32) return ((const float*)p)[i];
  if (dtype == GAN_BF16) return (float)((const bf16_t*)p)[i];
  return (float)((const f16_t*)p)[i];
}

// x', y' of one pixel of a level: the stored values halved (level 0) or the pooled fp32 values
template <typename TA, typename TB>
__device__ __forceinline__ void ld_level(const MsArgs& q, int level, int img, int ch, int y, int x, float& va, float& vb) {
  const MsLevel& L = q.lv[level];
  if (level == 0) {
    const long long pix = ((long long)img * L.h + y) * L.w + x;
    va = 0.5f * ld_f((const TA*)q.a + pix * q.pitch_a + ch);
    vb = 0.5f * ld_f((const TB*)q.b + pix * q.pitch_b + ch);
  } else {
    const long long i = L.pyr + (((long long)img * q.c + ch) * L.h + y) * L.w + x;
    va = q.pyr_a[i];
    vb = q.pyr_b[i];
  }
}

template <typename TA, typename TB>
__global__ __launch_bounds__(MTHREADS) void msssim_pool_kernel(const MsArgs q) {
  const int src = q.level;
  const MsLevel& S = q.lv[src];
  const MsLevel& D = q.lv[src + 1];
  const long long total = (long long)q.n * q.c * D.h * D.w;
  for (long long t = (long long)blockIdx.x * MTHREADS + threadIdx.x; t < total; t += (long long)gridDim.x * MTHREADS) {
    const int k = (int)(t % D.w);
    long long r = t / D.w;
    const int i = (int)(r % D.h);
    r /= D.h;
    const int ch = (int)(r % q.c), img = (int)(r / q.c);
    const int y0 = 2 * i, x0 = 2 * k;
    const int y1 = y0 + 1 < S.h ? y0 + 1 : S.h - 1, x1 = x0 + 1 < S.w ? x0 + 1 : S.w - 1;
    float a00, a01, a10, a11, b00, b01, b10, b11;
    ld_level<TA, TB>(q, src, img, ch, y0, x0, a00, b00);
    ld_level<TA, TB>(q, src, img, ch, y0, x1, a01, b01);
    ld_level<TA, TB>(q, src, img, ch, y1, x0, a10, b10);
    ld_level<TA, TB>(q, src, img, ch, y1, x1, a11, b11);
    q.pyr_a[D.pyr + t] = 0.25f * q_add(q_add(a00, a01), q_add(a10, a11));
    q.pyr_b[D.pyr + t] = 0.25f * q_add(q_add(b00, b01), q_add(b10, b11));
  }
}

// GRAD false: the statistics of every level in one launch (blockIdx.x runs over the tile table).  GRAD true: the gradient of the
// level q.level.  MN map positions per axis around a tile, staged pixels MS = MN + 10 per axis, both from the origin tile - OFF.
template <typename TA, typename TB, bool GRAD>
__global__ __launch_bounds__(MTHREADS) void msssim_tile_kernel(const MsArgs q) {
  constexpr int OFF = GRAD ? MK - 1 : 0;
  constexpr int MN = MT + OFF;            // 42 | 32
  constexpr int MS = MN + MK - 1;         // 52 | 42
  __shared__ float s_in[2 * MS * MS];            // staged x', y'; then P, Q, R
  __shared__ float s_hm[4 * MS * MN];            // row-filtered maps; then the row-transposed P, Q, R
  __shared__ float red[2][MTHREADS / 64];
  float (*sa)[MS] = reinterpret_cast<float (*)[MS]>(s_in);
  float (*sb)[MS] = reinterpret_cast<float (*)[MS]>(s_in + MS * MS);
  float (*pqr)[MN][MN] = reinterpret_cast<float (*)[MN][MN]>(s_in);
  float (*hm)[MS][MN] = reinterpret_cast<float (*)[MS][MN]>(s_hm);
  float (*tr)[MN][MT] = reinterpret_cast<float (*)[MN][MT]>(s_hm);
  static_assert(3 * MN * MN <= 2 * MS * MS && 3 * MN * MT <= 4 * MS * MN, "aliased LDS regions");
  const int tid = threadIdx.x;
  int level = q.level;
  if (!GRAD) {
    level = 0;
    while (level + 1 < q.scales && (int)blockIdx.x >= q.lv[level + 1].tile_base) ++level;
  }
  const MsLevel& L = q.lv[level];
  const int tile = GRAD ? (int)blockIdx.x : (int)blockIdx.x - L.tile_base;
  const int tiles = L.tiles_x * L.tiles_y;
  const int ty = tile / L.tiles_x, tx = tile - ty * L.tiles_x;
  const int y0 = ty * MT, x0 = tx * MT;                            // first pixel of the tile = first map position it owns
  const int py0 = y0 - OFF, px0 = x0 - OFF;                        // origin of the staged pixels and of the MN x MN positions
  const int mh = L.h - (MK - 1), mw = L.w - (MK - 1);              // map size of the level
  const bool last = level == q.scales - 1;                        // its factor is lum * cs; below it, cs alone
  const float coef = q.ls ? q.coef * q.ls[0] : q.coef;
  for (int img = blockIdx.y; img < q.n; img += gridDim.y) {
    for (int ch = 0; ch < q.c; ++ch) {
      __syncthreads();                                             // the previous channel's (image's) readers are done
      for (int i = tid; i < MS * MS; i += MTHREADS) {
        const int r = i / MS, x = i - r * MS;
        const int gy = py0 + r, gx = px0 + x;
        float va = 0.f, vb = 0.f;
        if (gy >= 0 && gy < L.h && gx >= 0 && gx < L.w) ld_level<TA, TB>(q, level, img, ch, gy, gx, va, vb);
        sa[r][x] = va;
        sb[r][x] = vb;
      }
      __syncthreads();
      float own_a[MPIX], own_b[MPIX];                              // x', y' at the pixels this thread writes
      if (GRAD) {
#pragma unroll
        for (int j = 0; j < MPIX; ++j) {
          const int i = tid + j * MTHREADS, r = i / MT, x = i - r * MT;
          own_a[j] = sa[r + OFF][x + OFF];
          own_b[j] = sb[r + OFF][x + OFF];
        }
      }
      for (int i = tid; i < MS * MN; i += MTHREADS) {              // along the rows
        const int r = i / MN, x = i - r * MN;
        float fa = 0.f, fb = 0.f, fab = 0.f, fsq = 0.f;
#pragma unroll
        for (int k = 0; k < MK; ++k) {
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
      float s_cs = 0.f, s_s = 0.f;
      for (int i = tid; i < MN * MN; i += MTHREADS) {              // along the columns, then the terms and their derivatives
        const int r = i / MN, x = i - r * MN;
        const int qy = py0 + r, qx = px0 + x;
        float P = 0.f, Q = 0.f, R = 0.f;
        if (qy >= 0 && qy < mh && qx >= 0 && qx < mw) {
          float ma = 0.f, mb = 0.f, eab = 0.f, esq = 0.f;
#pragma unroll
          for (int k = 0; k < MK; ++k) {
            const float wk = q.g[k];
            ma = fmaf(wk, hm[0][r + k][x], ma);
            mb = fmaf(wk, hm[1][r + k][x], mb);
            eab = fmaf(wk, hm[2][r + k][x], eab);
            esq = fmaf(wk, hm[3][r + k][x], esq);
          }
          const SsimTerms t = ssim_terms(ma, mb, eab, esq);
          if (!GRAD) {                                             // (every position here is one the tile owns)
            s_cs += t.cs;
            s_s += q_mul(t.lum, t.cs);
          } else if (last) {                                       // dssim.hip's maps of lum * cs
            const float il = 2.f / t.lum_d, ic = 2.f / t.cs_d;
            const float dl = q_mul(q_mul(t.cs, il), q_sub(t.my, q_mul(t.lum, t.mx)));
            const float dc = q_mul(q_mul(t.lum, ic), q_sub(mb, q_mul(t.cs, ma)));
            P = q_sub(dl, dc);
            Q = q_mul(t.lum, ic);
            R = -0.5f * q_mul(t.cs, Q);
          } else {                                                 // the maps of cs alone
            Q = 2.f / t.cs_d;
            P = -q_mul(Q, q_sub(mb, q_mul(t.cs, ma)));
            R = -0.5f * q_mul(t.cs, Q);
          }
        }
        if (GRAD) {
          pqr[0][r][x] = P;
          pqr[1][r][x] = Q;
          pqr[2][r][x] = R;
        }
      }
      if (!GRAD) {
        // fixed-order workgroup sums: butterfly inside each wave, then the four wave sums in order
        s_cs = wave_sum(s_cs);
        s_s = wave_sum(s_s);
        if ((tid & 63) == 0) {
          red[0][tid >> 6] = s_cs;
          red[1][tid >> 6] = s_s;
        }
        __syncthreads();
        if (tid == 0) {
          float* out = q.partial + L.part + ((((long long)img * q.c + ch) * tiles) + tile) * 2;
          out[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
          out[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        }
        continue;
      }
      __syncthreads();                                             // (the row-filtered maps are dead from here: tr takes their place)
      for (int i = tid; i < MN * MT; i += MTHREADS) {              // transposed filter along the rows: pixel column x <- positions x + 10 - k
        const int r = i / MT, x = i - r * MT;
        float tp = 0.f, tq = 0.f, tr_ = 0.f;
#pragma unroll
        for (int k = 0; k < MK; ++k) {
          const float wk = q.g[k];
          tp = fmaf(wk, pqr[0][r][x + MK - 1 - k], tp);
          tq = fmaf(wk, pqr[1][r][x + MK - 1 - k], tq);
          tr_ = fmaf(wk, pqr[2][r][x + MK - 1 - k], tr_);
        }
        tr[0][r][x] = tp;
        tr[1][r][x] = tq;
        tr[2][r][x] = tr_;
      }
      __syncthreads();
      const float kk = q.kk[((long long)level * q.n + img) * q.c + ch];
#pragma unroll
      for (int j = 0; j < MPIX; ++j) {                             // along the columns: pixel row r <- positions r + 10 - k; then the pixel
        const int i = tid + j * MTHREADS, r = i / MT, x = i - r * MT;
        const int gy = y0 + r, gx = x0 + x;
        if (gy >= L.h || gx >= L.w) continue;
        float gp = 0.f, gq = 0.f, gr = 0.f;
#pragma unroll
        for (int k = 0; k < MK; ++k) {
          const float wk = q.g[k];
          gp = fmaf(wk, tr[0][r + MK - 1 - k][x], gp);
          gq = fmaf(wk, tr[1][r + MK - 1 - k][x], gq);
          gr = fmaf(wk, tr[2][r + MK - 1 - k][x], gr);
        }
        // y' G^T[Q] and 2 x' G^T[R] rounded on their own: for a == b they are equal and opposite
        float v = q_mul(kk, q_add(gp, q_add(q_mul(own_b[j], gq), q_mul(q_mul(2.f, own_a[j]), gr))));
        if (!last) {                                               // U(G_{j+1}): 0.25 of the parent per tap of the parent that is this pixel
          const MsLevel& U = q.lv[level + 1];
          const int taps = ((gy == L.h - 1 && !(gy & 1)) ? 2 : 1) * ((gx == L.w - 1 && !(gx & 1)) ? 2 : 1);
          const float up = q.gws[U.pyr + (((long long)img * q.c + ch) * U.h + (gy >> 1)) * U.w + (gx >> 1)];
          v = q_add(v, q_mul(0.25f * (float)taps, up));
        }
        if (level > 0) {
          q.gws[L.pyr + (((long long)img * q.c + ch) * L.h + gy) * L.w + gx] = v;
        } else {
          const long long e = (((long long)img * L.h + gy) * L.w + gx) * q.pitch_da + ch;
          const float gv = q_mul(coef, v) / q.batch;
          st_any(q.da, e, q.dtype_da, q.grad_acc ? q_add(ld_any(q.da, e, q.dtype_da), gv) : gv);
        }
      }
    }
  }
}

struct MsFinal {
  int n, c, scales;
  MsLevel lv[MAX_SCALES];
  float power[MAX_SCALES];
  const float* partial;
  float* kk;
  float* per_image;                     // or NULL
  float* loss_out;
  float loss_scale;
  int acc;
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One workgroup, one wave per image (images dealt to the four waves in turn).  Every lane of the wave holds the same sums (the
// butterfly adds the same pairs in every lane), so the scalar work that follows is uniform and lane 0 writes.
__global__ __launch_bounds__(MTHREADS) void msssim_finalize_kernel(const MsFinal f) {
  __shared__ double red[MTHREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double score_sum = 0.0;
  for (int img = wave; img < f.n; img += MTHREADS / 64) {
    double score = 0.0;
    for (int ch = 0; ch < f.c; ++ch) {
      double term[MAX_SCALES];                                     // CS_j below the last level, S at the last
      double ms = 1.0;
      bool clamped = false;
#pragma unroll
      for (int j = 0; j < MAX_SCALES; ++j) {
        if (j >= f.scales) continue;
        const MsLevel& L = f.lv[j];
        const int tiles = L.tiles_x * L.tiles_y;
        const float* p = f.partial + L.part + ((long long)img * f.c + ch) * tiles * 2 + (j == f.scales - 1 ? 1 : 0);
        double s = 0.0;
        for (int t = lane; t < tiles; t += 64) s += (double)p[2 * (long long)t];
        s = wave_sum_d(s);
        term[j] = s / ((double)(L.h - (MK - 1)) * (double)(L.w - (MK - 1)));
        if (term[j] > 0.0) ms *= pow(term[j], (double)f.power[j]);
        else { ms *= f.power[j] == 0.f ? 1.0 : 0.0; clamped = true; }      // max(term, 0)^w, and no gradient through the clamp
      }
      score += ms;
#pragma unroll
      for (int j = 0; j < MAX_SCALES; ++j) {
        if (j >= f.scales) continue;
        const MsLevel& L = f.lv[j];
        const double k = clamped ? 0.0 : (double)f.power[j] * ms / term[j] / ((double)(L.h - (MK - 1)) * (double)(L.w - (MK - 1)));
        if (lane == 0) f.kk[((long long)j * f.n + img) * f.c + ch] = (float)k;
      }
    }
    score /= (double)f.c;
    if (lane == 0 && f.per_image) f.per_image[img] = (float)score;
    score_sum += score;
  }
  if (lane == 0) red[wave] = score_sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double mean = (((red[0] + red[1]) + red[2]) + red[3]) / (double)f.n;
    const float t = (float)(1.0 - mean) * f.loss_scale;
    f.loss_out[0] = f.acc ? f.loss_out[0] + t : t;
  }
}

inline int m_tiles(int v) { return (v + MT - 1) / MT; }
// every level holds a full window also when it is pooled without the repeated edge: h, w >= 11 * 2^(scales - 1)
inline bool m_shape_ok(int n, int h, int w, int c, int scales) {
  if (scales < 1 || scales > MAX_SCALES) return false;
  return n >= 1 && (h >> (scales - 1)) >= MK && (w >> (scales - 1)) >= MK && h <= SSIM_MAX_EDGE && w <= SSIM_MAX_EDGE && (c == 1 || c == 3);
}

struct MsLayout {
  MsLevel lv[MAX_SCALES];
  long long pyr_floats;                 // one pooled pyramid (levels 1 ..): three of them (a, b, G)
  long long part_floats;
  long long kk_floats;
  int tiles_total;
};
inline MsLayout m_layout(int n, int h, int w, int c, int scales) {
  MsLayout y;
  long long pyr = 0, part = 0;
  int base = 0;
  for (int j = 0; j < scales; ++j) {
    MsLevel& L = y.lv[j];
    L.h = h; L.w = w;
    L.tiles_x = m_tiles(w); L.tiles_y = m_tiles(h);
    L.tile_base = base;
    base += L.tiles_x * L.tiles_y;
    L.pyr = pyr;
    if (j > 0) pyr += (long long)n * c * h * w;
    L.part = part;
    part += (long long)n * c * L.tiles_x * L.tiles_y * 2;
    h = (h + 1) / 2; w = (w + 1) / 2;
  }
  for (int j = scales; j < MAX_SCALES; ++j) y.lv[j] = MsLevel{0, 0, 0, 0, base, 0, 0};
  y.pyr_floats = pyr;
  y.part_floats = part;
  y.kk_floats = (long long)scales * n * c;
  y.tiles_total = base;
  return y;
}

template <typename TA, typename TB> void launch_ab(int what, const MsArgs& q, dim3 grid, hipStream_t st) {
  if (what == 0) GAN_LAUNCH((msssim_pool_kernel<TA, TB>), grid, dim3(MTHREADS), 0, st, q);
  else if (what == 1) GAN_LAUNCH((msssim_tile_kernel<TA, TB, false>), grid, dim3(MTHREADS), 0, st, q);
  else GAN_LAUNCH((msssim_tile_kernel<TA, TB, true>), grid, dim3(MTHREADS), 0, st, q);
}
template <typename TA> void launch_b(int what, int dtype_b, const MsArgs& q, dim3 grid, hipStream_t st) {
  switch (dtype_b) {
    case GAN_F32: launch_ab<TA, float>(what, q, grid, st); break;
    case GAN_BF16: launch_ab<TA, bf16_t>(what, q, grid, st); break;
    default: launch_ab<TA, f16_t>(what, q, grid, st); break;
  }
}
// what: 0 pool, 1 statistics, 2 gradient.  Launches that never touch level 0 use the <float, float> instance.
void launch(int what, bool level0, int dtype_a, int dtype_b, const MsArgs& q, dim3 grid, hipStream_t st) {
  if (!level0) { launch_ab<float, float>(what, q, grid, st); return; }
  switch (dtype_a) {
    case GAN_F32: launch_b<float>(what, dtype_b, q, grid, st); break;
    case GAN_BF16: launch_b<bf16_t>(what, dtype_b, q, grid, st); break;
    default: launch_b<f16_t>(what, dtype_b, q, grid, st); break;
  }
}

}  // namespace

extern "C" size_t gan_msssim_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t scales) {
  if (!m_shape_ok(n, h, w, c, scales)) return 0;
  const MsLayout y = m_layout(n, h, w, c, scales);
  return (size_t)(3 * y.pyr_floats + y.part_floats + y.kk_floats) * sizeof(float);
}

extern "C" int gan_msssim(const GanMsssimDesc* d, gan_stream_t stream) {
  if (!d || d->struct_size != sizeof(GanMsssimDesc)) return GAN_E_ARG;
  const GanTensor &a = d->a, &b = d->b, &da = d->da;
  if (!a.ptr || !b.ptr || !d->loss_out || !d->workspace) return GAN_E_ARG;
  if (!gan_dtype_ok(d->dtype_a) || !gan_dtype_ok(d->dtype_b)) return GAN_E_ARG;
  if (a.c != 1 && a.c != 3) return GAN_E_ARG;
  if (a.n != b.n || a.h != b.h || a.w != b.w || a.c != b.c) return GAN_E_ARG;
  if (a.n < 1 || a.pitch < a.c || b.pitch < b.c) return GAN_E_ARG;
  if (d->loss_accumulate != 0 && d->loss_accumulate != 1) return GAN_E_ARG;
  if (d->grad_accumulate != 0 && d->grad_accumulate != 1) return GAN_E_ARG;
  if (d->scales < 1 || d->scales > MAX_SCALES) return GAN_E_ARG;
  for (int j = 0; j < d->scales; ++j)
    if (!(d->power[j] >= 0.f) || isinf(d->power[j])) return GAN_E_ARG;
  if (da.ptr) {
    if (!gan_dtype_ok(d->dtype_da)) return GAN_E_ARG;
    if (da.n != a.n || da.h != a.h || da.w != a.w || da.c != a.c || da.pitch < da.c) return GAN_E_ARG;
  }
  if (!m_shape_ok(a.n, a.h, a.w, a.c, d->scales)) return GAN_E_SHAPE;
  if (d->workspace_bytes < gan_msssim_workspace_bytes(a.n, a.h, a.w, a.c, d->scales)) return GAN_E_WORKSPACE;
  const int M = d->scales;
  const MsLayout y = m_layout(a.n, a.h, a.w, a.c, M);
  MsArgs q;
  q.a = a.ptr; q.b = b.ptr; q.da = da.ptr;
  q.pitch_a = a.pitch; q.pitch_b = b.pitch; q.pitch_da = da.ptr ? da.pitch : 0; q.dtype_da = d->dtype_da;
  q.n = a.n; q.c = a.c; q.scales = M; q.level = 0; q.grad_acc = d->grad_accumulate;
  for (int j = 0; j < MAX_SCALES; ++j) q.lv[j] = y.lv[j];
  ssim_window(q.g);
  q.coef = (float)(-0.5 * (double)d->grad_scale / a.c);
  q.batch = (float)a.n;
  q.ls = d->scale_state;
  float* ws = (float*)d->workspace;
  q.pyr_a = ws;
  q.pyr_b = ws + y.pyr_floats;
  q.gws = ws + 2 * y.pyr_floats;
  q.partial = ws + 3 * y.pyr_floats;
  q.kk = q.partial + y.part_floats;
  hipStream_t st = (hipStream_t)stream;
  const int ny = a.n < 65535 ? a.n : 65535;
  for (int j = 0; j + 1 < M; ++j) {                                // the pyramid
    q.level = j;
    const long long total = (long long)a.n * a.c * y.lv[j + 1].h * y.lv[j + 1].w;
    const long long blocks = (total + MTHREADS - 1) / MTHREADS;
    launch(0, j == 0, d->dtype_a, d->dtype_b, q, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), st);
    GAN_CHECK_LAUNCH();
  }
  q.level = 0;
  launch(1, true, d->dtype_a, d->dtype_b, q, dim3(y.tiles_total, ny), st);
  GAN_CHECK_LAUNCH();
  MsFinal f;
  f.n = a.n; f.c = a.c; f.scales = M;
  for (int j = 0; j < MAX_SCALES; ++j) { f.lv[j] = y.lv[j]; f.power[j] = j < M ? d->power[j] : 0.f; }
  f.partial = q.partial; f.kk = q.kk; f.per_image = d->per_image; f.loss_out = d->loss_out;
  f.loss_scale = d->loss_scale; f.acc = d->loss_accumulate;
  GAN_LAUNCH(msssim_finalize_kernel, dim3(1), dim3(MTHREADS), 0, st, f);
  GAN_CHECK_LAUNCH();
  if (!da.ptr) return 0;
  for (int j = M - 1; j >= 0; --j) {                               // the gradient, coarsest level first
    q.level = j;
    launch(2, j == 0, d->dtype_a, d->dtype_b, q, dim3(y.lv[j].tiles_x * y.lv[j].tiles_y, ny), st);
    GAN_CHECK_LAUNCH();
  }
  return 0;
}
