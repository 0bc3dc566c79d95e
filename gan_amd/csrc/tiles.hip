// Tiled inference (include/gan_amd.h: gan_tile_grid, gan_tile_gather_u8, gan_tile_blend): an image larger than the network's input
// is cut into overlapping tile x tile pieces that go through one inference call as a batch, and the outputs are blended back.  No
// counterpart in the reference, which resizes every image to img_size x img_size before it predicts (pix2pix.py:43-52).
//
// Geometry, per image axis of length L with tile size S, overlap V, stride T = S - V:
//     count n = 1 if L == S, else ceil((L - S) / T) + 1;   origin of tile k = min(k * T, L - S)
// so the tiles 0 .. n-2 sit on the stride and the last one is pulled back to end at the image edge; tiles are numbered row-major,
// t = ky * nx + kx.  With V <= S / 2 (S <= 2 T) a coordinate p is covered by at most two tiles on the stride, k = p / T - 1 and
// p / T (the offset into k = p / T - 2 would be >= 2 T >= S), plus, possibly, the last tile: at most 3.
//
// Weight arithmetic (the tests rely on this order).  Per axis the integer hat of the offset i inside a tile, hat(i) = min(i + 1, S - i)
// (>= 1), and over ALL tiles k of the grid that cover p, whether or not this launch holds them, i_k = p - origin_k:
//     a_k(p) = float(hat(i_k)) / float(sum_j hat(i_j))                   one fp32 division of exactly representable integers
//     out(py, px, ch) = sum_{ky ascending} sum_{kx ascending} (a_ky(py) * a_kx(px)) * tile_value
// in fp32; every product and every addition is rounded on its own (__fmul_rn / __fadd_rn: nothing is contracted into an FMA), the
// terms are added in exactly that order, and the sum starts from 0.0f (accumulate = 0) or from the stored value (accumulate = 1).  A
// pixel one tile covers has the weight 1.0f / 1.0f * 1.0f: the tile's value comes back bit for bit.  Because a launch that holds only
// the tiles [t0, t0 + n) adds its terms in the same ascending order onto the stored fp32 value, an image's tiles split over several
// launches in ascending order give the bits of one launch.
//
// Both kernels are streaming, gather-form on the output side: tile_blend_kernel gives every output pixel to one thread, which
// finds the covering tiles, reads them (one 16-byte load per tile for a 16-bit view of pitch 8) and writes its c floats once - no
// atomics, no workspace.  tile_gather_kernel gives every destination pixel to one thread, which reads its c source bytes through
// the clamped index and writes the c real channels; the pad channels of a wider pitch are not touched, as gan_pack leaves them.
//
// tile_gather_f_kernel (gan_tile_gather) is the same gather from a float image - the blended fp32 output of one generator as the
// input of the next, the cycle of a CycleGAN at the source resolution - with a bit copy or one rounding in place of the table.
#include <type_traits>

#include "common.h"

namespace {

constexpr int TILE_THREADS = 256;

struct TileGeo {
  int h, w, tile, stride;      // stride = tile - overlap
  int ny, nx;
};

inline int axis_count(int L, int S, int T) { return L == S ? 1 : (L - S + T - 1) / T + 1; }

__device__ __forceinline__ int axis_origin(int k, int n, int L, int S, int T) { return k == n - 1 ? L - S : k * T; }

// The tiles of one axis that cover coordinate p, ascending: k[] and the offset inside each; -> how many (1 ..= 3) and the sum of
// their hats.
__device__ __forceinline__ int axis_cover(int p, int n, int L, int S, int T, int* k, int* off, int& hat_sum) {
  int cnt = 0;
  hat_sum = 0;
  const int kb = p / T;
  for (int j = max(kb - 1, 0); j <= min(kb, n - 2); ++j) {     // tiles on the stride: origin j * T <= p
    const int i = p - j * T;
    if (i < S) { k[cnt] = j; off[cnt] = i; hat_sum += min(i + 1, S - i); ++cnt; }
  }
  const int i = p - (L - S);                                   // the last tile, pulled back to the edge: p - origin < S always
  if (i >= 0) { k[cnt] = n - 1; off[cnt] = i; hat_sum += min(i + 1, S - i); ++cnt; }
  return cnt;
}

struct GatherArgs {
  const uint8_t* src;
  long long src_bytes;
  int src_pitch, col0;
  TileGeo g;
  int t0, n;
  const float* lut;
  void* dst;
  int pitch;
};

template <typename T, int C>
__global__ __launch_bounds__(TILE_THREADS) void tile_gather_kernel(const GatherArgs a) {
  const int S = a.g.tile;
  const long long per = (long long)S * S, total = per * a.n;
  T* __restrict__ dst = (T*)a.dst;
  for (long long i = (long long)blockIdx.x * TILE_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * TILE_THREADS) {
    const int tl = (int)(i / per), rem = (int)(i - tl * per);
    const int r = rem / S, x = rem - r * S;
    const int t = a.t0 + tl, ky = t / a.g.nx, kx = t - ky * a.g.nx;
    const int sy = axis_origin(ky, a.g.ny, a.g.h, S, a.g.stride) + r;
    const int sx = axis_origin(kx, a.g.nx, a.g.w, S, a.g.stride) + x;
    const long long at = (long long)sy * a.src_pitch + (long long)(a.col0 + sx) * C;
    T* o = dst + i * a.pitch;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) st_f(o + ch, a.lut[a.src[min(max(at + ch, 0LL), a.src_bytes - 1)]]);
  }
}

struct GatherFArgs {
  const void* src;
  long long src_elems;
  int src_pitch, col0;         // elements / pixels
  TileGeo g;
  int t0, n;
  void* dst;
  int pitch;
};

// The float-source sibling: the same thread-per-destination-pixel index arithmetic, no table.  TS == TD moves the bits (a NaN keeps
// its payload); otherwise TS is float and st_f rounds to nearest.
template <typename TS, typename TD, int C>
__global__ __launch_bounds__(TILE_THREADS) void tile_gather_f_kernel(const GatherFArgs a) {
  const int S = a.g.tile;
  const long long per = (long long)S * S, total = per * a.n;
  const TS* __restrict__ src = (const TS*)a.src;
  TD* __restrict__ dst = (TD*)a.dst;
  for (long long i = (long long)blockIdx.x * TILE_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * TILE_THREADS) {
    const int tl = (int)(i / per), rem = (int)(i - tl * per);
    const int r = rem / S, x = rem - r * S;
    const int t = a.t0 + tl, ky = t / a.g.nx, kx = t - ky * a.g.nx;
    const int sy = axis_origin(ky, a.g.ny, a.g.h, S, a.g.stride) + r;
    const int sx = axis_origin(kx, a.g.nx, a.g.w, S, a.g.stride) + x;
    const long long at = (long long)sy * a.src_pitch + (long long)(a.col0 + sx) * C;
    TD* o = dst + i * a.pitch;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const TS v = src[min(max(at + ch, 0LL), a.src_elems - 1)];
      if constexpr (std::is_same<TS, TD>::value) o[ch] = v;
      else st_f(o + ch, ld_f(&v));
    }
  }
}

struct BlendArgs {
  const void* tiles;
  int pitch;
  float* image;
  TileGeo g;
  int t0, n, accumulate;
};

// VEC: the view is 16-bit storage of pitch 8 on a 16-byte aligned pointer - a pixel's channels arrive in one 16-byte load
template <typename T, int C, bool VEC>
__global__ __launch_bounds__(TILE_THREADS) void tile_blend_kernel(const BlendArgs a) {
  const int S = a.g.tile, T_ = a.g.stride;
  const long long total = (long long)a.g.h * a.g.w;
  const T* __restrict__ tiles = (const T*)a.tiles;
  for (long long i = (long long)blockIdx.x * TILE_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * TILE_THREADS) {
    const int py = (int)(i / a.g.w), px = (int)(i - (long long)py * a.g.w);
    int kys[3], iys[3], kxs[3], ixs[3], sum_y, sum_x;
    const int cy = axis_cover(py, a.g.ny, a.g.h, S, T_, kys, iys, sum_y);
    const int cx = axis_cover(px, a.g.nx, a.g.w, S, T_, kxs, ixs, sum_x);
    float* o = a.image + i * C;
    float acc[C];
    bool any = false;
    for (int jy = 0; jy < cy; ++jy) {
      const float ay = (float)min(iys[jy] + 1, S - iys[jy]) / (float)sum_y;
      for (int jx = 0; jx < cx; ++jx) {
        const int tl = kys[jy] * a.g.nx + kxs[jx] - a.t0;
        if (tl < 0 || tl >= a.n) continue;
        if (!any) {
          any = true;
#pragma unroll
          for (int ch = 0; ch < C; ++ch) acc[ch] = a.accumulate ? o[ch] : 0.f;
        }
        const float ax = (float)min(ixs[jx] + 1, S - ixs[jx]) / (float)sum_x;
        const float wgt = __fmul_rn(ay, ax);
        const long long pix = ((long long)tl * S + iys[jy]) * S + ixs[jx];
        float v[8];
        if constexpr (VEC) {
          unpack16<T>(*(const uint4*)(tiles + pix * 8), v);
        } else {
#pragma unroll
          for (int ch = 0; ch < C; ++ch) v[ch] = ld_f(tiles + pix * a.pitch + ch);
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) acc[ch] = __fadd_rn(acc[ch], __fmul_rn(wgt, v[ch]));
      }
    }
    if (any) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) o[ch] = acc[ch];
    } else if (!a.accumulate) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) o[ch] = 0.f;
    }
  }
}

inline unsigned tile_blocks(long long threads) {
  const long long b = (threads + TILE_THREADS - 1) / TILE_THREADS;
  return (unsigned)(b < 8192 ? b : 8192);       // grid-stride beyond: 32 workgroups per CU
}

inline size_t dtype_size(int dtype) { return dtype == GAN_F32 ? 4 : 2; }

// the checks the two launches share, after their pointers: geometry (GAN_E_SHAPE), then the view and the tile range (GAN_E_ARG)
inline int check_tiles(const GanTensor& v, int dtype, int h, int w, int c, int tile, int overlap, int t0, int n, TileGeo* g) {
  int32_t ny, nx;
  const int rc = gan_tile_grid(h, w, tile, overlap, &ny, &nx);
  if (rc) return rc;
  if (v.n != n || v.h != tile || v.w != tile || v.c != c || v.pitch < c) return GAN_E_ARG;
  if (t0 < 0 || n < 1 || (long long)t0 + n > (long long)ny * nx) return GAN_E_ARG;
  if ((uintptr_t)v.ptr % dtype_size(dtype)) return GAN_E_ARG;
  g->h = h; g->w = w; g->tile = tile; g->stride = tile - overlap; g->ny = ny; g->nx = nx;
  return 0;
}

template <typename T> void launch_gather(int c, const GatherArgs& a, dim3 grid, hipStream_t st) {
  if (c == 1)
    GAN_LAUNCH((tile_gather_kernel<T, 1>), grid, dim3(TILE_THREADS), 0, st, a);
  else
    GAN_LAUNCH((tile_gather_kernel<T, 3>), grid, dim3(TILE_THREADS), 0, st, a);
}

template <typename TS, typename TD> void launch_gather_f(int c, const GatherFArgs& a, dim3 grid, hipStream_t st) {
  if (c == 1)
    GAN_LAUNCH((tile_gather_f_kernel<TS, TD, 1>), grid, dim3(TILE_THREADS), 0, st, a);
  else
    GAN_LAUNCH((tile_gather_f_kernel<TS, TD, 3>), grid, dim3(TILE_THREADS), 0, st, a);
}

template <typename T> void launch_blend(int c, bool vec, const BlendArgs& a, dim3 grid, hipStream_t st) {
  if (c == 1) {
    if (vec) GAN_LAUNCH((tile_blend_kernel<T, 1, true>), grid, dim3(TILE_THREADS), 0, st, a);
    else GAN_LAUNCH((tile_blend_kernel<T, 1, false>), grid, dim3(TILE_THREADS), 0, st, a);
  } else {
    if (vec) GAN_LAUNCH((tile_blend_kernel<T, 3, true>), grid, dim3(TILE_THREADS), 0, st, a);
    else GAN_LAUNCH((tile_blend_kernel<T, 3, false>), grid, dim3(TILE_THREADS), 0, st, a);
  }
}

}  // namespace

extern "C" int gan_tile_grid(int32_t h, int32_t w, int32_t tile, int32_t overlap, int32_t* ny, int32_t* nx) {
  if (!ny || !nx) return GAN_E_ARG;
  if (tile < 16 || tile > 1024 || tile % 8) return GAN_E_SHAPE;
  if (overlap < 0 || 2 * overlap > tile) return GAN_E_SHAPE;
  if (h < tile || w < tile || h > 4096 || w > 4096) return GAN_E_SHAPE;
  *ny = axis_count(h, tile, tile - overlap);
  *nx = axis_count(w, tile, tile - overlap);
  return 0;
}

extern "C" int gan_tile_gather_u8(const GanTileGatherDesc* d, gan_stream_t stream) {
  if (!d || d->struct_size != sizeof(GanTileGatherDesc)) return GAN_E_ARG;
  if (!d->src || !d->lut || !d->dst.ptr) return GAN_E_ARG;
  if (!gan_dtype_ok(d->dtype) || (d->c != 1 && d->c != 3)) return GAN_E_ARG;
  GatherArgs a;
  const int rc = check_tiles(d->dst, d->dtype, d->h, d->w, d->c, d->tile, d->overlap, d->t0, d->n, &a.g);
  if (rc) return rc;
  if ((uintptr_t)d->lut & 3) return GAN_E_ARG;
  // the part used lies inside a source row, and its last row inside the buffer
  if (d->col0 < 0 || d->src_pitch < 1 || d->src_bytes < 1 || ((long long)d->col0 + d->w) * d->c > d->src_pitch) return GAN_E_ARG;
  if ((long long)(d->h - 1) * d->src_pitch + ((long long)d->col0 + d->w) * d->c > d->src_bytes) return GAN_E_ARG;
  a.src = d->src; a.src_bytes = d->src_bytes; a.src_pitch = d->src_pitch; a.col0 = d->col0;
  a.t0 = d->t0; a.n = d->n; a.lut = d->lut; a.dst = d->dst.ptr; a.pitch = d->dst.pitch;
  const dim3 grid(tile_blocks((long long)d->n * d->tile * d->tile));
  hipStream_t st = (hipStream_t)stream;
  switch (d->dtype) {
    case GAN_F32: launch_gather<float>(d->c, a, grid, st); break;
    case GAN_BF16: launch_gather<bf16_t>(d->c, a, grid, st); break;
    default: launch_gather<f16_t>(d->c, a, grid, st); break;
  }
  GAN_CHECK_LAUNCH();
  return 0;
}

extern "C" int gan_tile_gather(const GanTileGatherFDesc* d, gan_stream_t stream) {
  if (!d || d->struct_size != sizeof(GanTileGatherFDesc)) return GAN_E_ARG;
  if (!d->src || !d->dst.ptr) return GAN_E_ARG;
  if (!gan_dtype_ok(d->src_dtype) || !gan_dtype_ok(d->dst_dtype) || (d->c != 1 && d->c != 3)) return GAN_E_ARG;
  if (d->src_dtype != d->dst_dtype && d->src_dtype != GAN_F32) return GAN_E_ARG;      // a bit copy, or fp32 rounded once
  GatherFArgs a;
  const int rc = check_tiles(d->dst, d->dst_dtype, d->h, d->w, d->c, d->tile, d->overlap, d->t0, d->n, &a.g);
  if (rc) return rc;
  if ((uintptr_t)d->src % dtype_size(d->src_dtype)) return GAN_E_ARG;
  // the part used lies inside a source row, and its last row inside the buffer
  if (d->col0 < 0 || d->src_pitch < 1 || d->src_elems < 1 || ((long long)d->col0 + d->w) * d->c > d->src_pitch) return GAN_E_ARG;
  if ((long long)(d->h - 1) * d->src_pitch + ((long long)d->col0 + d->w) * d->c > d->src_elems) return GAN_E_ARG;
  a.src = d->src; a.src_elems = d->src_elems; a.src_pitch = d->src_pitch; a.col0 = d->col0;
  a.t0 = d->t0; a.n = d->n; a.dst = d->dst.ptr; a.pitch = d->dst.pitch;
  const dim3 grid(tile_blocks((long long)d->n * d->tile * d->tile));
  hipStream_t st = (hipStream_t)stream;
  if (d->src_dtype == GAN_F32) {
    switch (d->dst_dtype) {
      case GAN_F32: launch_gather_f<float, float>(d->c, a, grid, st); break;
      case GAN_BF16: launch_gather_f<float, bf16_t>(d->c, a, grid, st); break;
      default: launch_gather_f<float, f16_t>(d->c, a, grid, st); break;
    }
  } else if (d->src_dtype == GAN_BF16) {
    launch_gather_f<bf16_t, bf16_t>(d->c, a, grid, st);
  } else {
    launch_gather_f<f16_t, f16_t>(d->c, a, grid, st);
  }
  GAN_CHECK_LAUNCH();
  return 0;
}

extern "C" int gan_tile_blend(const GanTileBlendDesc* d, gan_stream_t stream) {
  if (!d || d->struct_size != sizeof(GanTileBlendDesc)) return GAN_E_ARG;
  if (!d->tiles.ptr || !d->image) return GAN_E_ARG;
  if (!gan_dtype_ok(d->dtype) || (d->c != 1 && d->c != 3)) return GAN_E_ARG;
  BlendArgs a;
  const int rc = check_tiles(d->tiles, d->dtype, d->h, d->w, d->c, d->tile, d->overlap, d->t0, d->n, &a.g);
  if (rc) return rc;
  if (((uintptr_t)d->image & 3) || (d->accumulate != 0 && d->accumulate != 1)) return GAN_E_ARG;
  a.tiles = d->tiles.ptr; a.pitch = d->tiles.pitch; a.image = d->image;
  a.t0 = d->t0; a.n = d->n; a.accumulate = d->accumulate;
  const bool vec = d->dtype != GAN_F32 && d->tiles.pitch == 8 && ((uintptr_t)d->tiles.ptr & 15) == 0;
  const dim3 grid(tile_blocks((long long)d->h * d->w));
  hipStream_t st = (hipStream_t)stream;
  switch (d->dtype) {
    case GAN_F32: launch_blend<float>(d->c, false, a, grid, st); break;
    case GAN_BF16: launch_blend<bf16_t>(d->c, vec, a, grid, st); break;
    default: launch_blend<f16_t>(d->c, vec, a, grid, st); break;
  }
  GAN_CHECK_LAUNCH();
  return 0;
}
