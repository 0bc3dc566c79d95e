// Differentiable augmentation of the discriminator inputs (include/gan_amd.h: gan_diffaug_draw, gan_diffaug_apply; DESIGN.md
// section 20).  Streaming launches: a record per image drawn by one small launch, then one gather per view and direction.
#include <string.h>

#include "common.h"

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {      // (the counter hash of the dropout masks and the image pool)
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// One axis of the cutout: the rectangle's [start, start + size / 2) intersected with [0, size) -> (x0, extent)
__device__ __forceinline__ void cut_axis(uint64_t bits32, int size, int& x0, int& ext) {
  const int cs = size / 2;
  const uint64_t n = (uint64_t)size + (uint64_t)(1 - cs % 2);
  const int start = (int)((bits32 * n) >> 32) - cs / 2;
  const int lo = max(start, 0), hi = min(start + cs, size);
  x0 = lo;
  ext = hi - lo;
}

// n <= 128 records, one thread each.  Every thread reads the counter; the barrier puts all those reads in front of the one store.
__global__ __launch_bounds__(128) void diffaug_draw_kernel(GanDiffAugParams* params, int n, int h, int w, uint32_t policy,
                                                           uint64_t seed, uint32_t sid, int32_t* launches) {
  const uint32_t draw = (uint32_t)*launches;
  const int i = threadIdx.x;
  if (i < n) {
    const uint64_t key = mix64(seed ^ ((uint64_t)draw << 32) ^ sid);
    GanDiffAugParams p;
    p.tx = p.ty = 0;
    p.cut_x0 = p.cut_y0 = p.cut_w = p.cut_h = 0;
    p.brightness = 0.f;
    p.saturation = 1.f;
    if (policy & GAN_DIFFAUG_TRANSLATION) {
      const uint64_t h0 = mix64(key ^ (uint64_t)(4 * i));
      const int Tx = (w + 4) / 8, Ty = (h + 4) / 8;
      p.tx = (int)(((h0 & 0xffffffffull) * (uint64_t)(2 * Tx + 1)) >> 32) - Tx;
      p.ty = (int)(((h0 >> 32) * (uint64_t)(2 * Ty + 1)) >> 32) - Ty;
    }
    if (policy & GAN_DIFFAUG_CUTOUT) {
      const uint64_t h1 = mix64(key ^ (uint64_t)(4 * i + 1));
      int x0, cw, y0, ch;
      cut_axis(h1 & 0xffffffffull, w, x0, cw);
      cut_axis(h1 >> 32, h, y0, ch);
      if (cw > 0 && ch > 0) { p.cut_x0 = x0; p.cut_y0 = y0; p.cut_w = cw; p.cut_h = ch; }
    }
    if (policy & GAN_DIFFAUG_BRIGHTNESS) {
      const uint64_t h2 = mix64(key ^ (uint64_t)(4 * i + 2));
      p.brightness = (float)(uint32_t)(h2 >> 40) * 0x1p-24f - 0.5f;
    }
    if (policy & GAN_DIFFAUG_SATURATION) {
      const uint64_t h3 = mix64(key ^ (uint64_t)(4 * i + 3));
      p.saturation = (float)(uint32_t)(h3 >> 40) * 0x1p-23f;
    }
    params[i] = p;
  }
  __syncthreads();
  if (threadIdx.x == 0) *launches = (int32_t)(draw + 1u);
}

// storage element <-> its bits <-> float
template <typename T> struct Bits { typedef uint16_t U; };
template <> struct Bits<float> { typedef uint32_t U; };
__device__ __forceinline__ float bits_f(float*, uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ float bits_f(bf16_t*, uint16_t u) { return __uint_as_float((uint32_t)u << 16); }
__device__ __forceinline__ float bits_f(f16_t*, uint16_t u) { return h2f(u); }
__device__ __forceinline__ uint32_t f_bits(float*, float v) { return __float_as_uint(v); }
__device__ __forceinline__ uint16_t f_bits(bf16_t*, float v) { const bf16_t b = (bf16_t)v; return *(const uint16_t*)&b; }
__device__ __forceinline__ uint16_t f_bits(f16_t*, float v) { const f16_t b = (f16_t)v; return *(const uint16_t*)&b; }

struct DiffAugArgs {
  const void* src; void* dst; const GanDiffAugParams* params;
  long long simg, dimg;           // elements between consecutive images of src / dst
  int h, w, c, spitch, dpitch, sample0;
  FastDiv wdiv;
};

// One group (an image's G channels at one pixel): raw bits in -> raw bits out.  move: colour is the identity for this image.
template <typename T, int G, bool BWD>
__device__ __forceinline__ void diffaug_group(const typename Bits<T>::U* r, typename Bits<T>::U* o, bool move, float s, float br) {
  if (move) {
#pragma unroll
    for (int k = 0; k < G; ++k) o[k] = r[k];
    return;
  }
  T* const tag = nullptr;
  if constexpr (G == 1) {        // (forward only: the backward of a one-channel image always moves bits)
    o[0] = f_bits(tag, bits_f(tag, r[0]) + br);
  } else {
    float x[G];
#pragma unroll
    for (int k = 0; k < G; ++k) x[k] = bits_f(tag, r[k]);
    const float m = (x[0] + x[1] + x[2]) / 3.0f;
#pragma unroll
    for (int k = 0; k < G; ++k) o[k] = f_bits(tag, BWD ? fmaf(s, x[k], (1.0f - s) * m) : fmaf(x[k] - m, s, m) + br);
  }
}

// A thread owns one pixel of dst (forward: an output pixel p, it reads x(p - t); backward: an input pixel q, it reads dy(q + t)).
// VEC: the source pixel is one aligned 16-byte unit.
template <typename T, int G, bool BWD, bool VEC>
__global__ __launch_bounds__(256) void diffaug_apply_kernel(const DiffAugArgs a) {
  typedef typename Bits<T>::U U;
  constexpr int N = VecOf<T>::N;            // elements of a 16-byte unit
  const int b = blockIdx.y;
  const uint32_t pix = blockIdx.x * 256u + threadIdx.x;
  if (pix >= (uint32_t)(a.h * a.w)) return;
  const GanDiffAugParams P = a.params[a.sample0 + b];
  const int py = (int)fdiv(pix, a.wdiv), px = (int)pix - py * a.w;
  const int qx = BWD ? px + P.tx : px - P.tx, qy = BWD ? py + P.ty : py - P.ty;      // the pixel of src this one reads
  const int ox = BWD ? qx : px, oy = BWD ? qy : py;                                  // ... and the OUTPUT pixel of the pair (the cut's side)
  const bool cut = P.cut_w > 0 && ox >= P.cut_x0 && ox < P.cut_x0 + P.cut_w && oy >= P.cut_y0 && oy < P.cut_y0 + P.cut_h;
  const bool live = !cut && qx >= 0 && qx < a.w && qy >= 0 && qy < a.h;
  const bool move = G == 1 ? (BWD || P.brightness == 0.f) : (P.saturation == 1.f && (BWD || P.brightness == 0.f));
  const float s = P.saturation, br = P.brightness;
  U* d = (U*)a.dst + (size_t)b * a.dimg + (size_t)pix * a.dpitch;
  const U* sp = (const U*)a.src + (size_t)b * a.simg + (size_t)(live ? qy * a.w + qx : 0) * a.spitch;      // (never read when !live)
  if (VEC) {
    U raw[N];
    if (live) {
      const uint4 v = *(const uint4*)sp;
      const uint32_t wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < N; ++k) raw[k] = sizeof(U) == 4 ? (U)wds[k] : (U)(wds[k >> 1] >> ((k & 1) * 16));
    }
#pragma unroll
    for (int g = 0; g + G <= N; g += G) {
      if (g < a.c) {                        // (c is a multiple of G)
        U o[G];
        if (live) {
          diffaug_group<T, G, BWD>(raw + g, o, move, s, br);
        } else {
#pragma unroll
          for (int k = 0; k < G; ++k) o[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < G; ++k) d[g + k] = o[k];
      }
    }
  } else {
    for (int g = 0; g < a.c; g += G) {
      U r[G], o[G];
      if (live) {
#pragma unroll
        for (int k = 0; k < G; ++k) r[k] = sp[g + k];
        diffaug_group<T, G, BWD>(r, o, move, s, br);
      } else {
#pragma unroll
        for (int k = 0; k < G; ++k) o[k] = 0;
      }
#pragma unroll
      for (int k = 0; k < G; ++k) d[g + k] = o[k];
    }
  }
}

template <typename T, int G, bool BWD>
void diffaug_launch(bool vec, dim3 grid, hipStream_t st, const DiffAugArgs& a) {
  if (vec)
    GAN_LAUNCH((diffaug_apply_kernel<T, G, BWD, true>), grid, dim3(256), 0, st, a);
  else
    GAN_LAUNCH((diffaug_apply_kernel<T, G, BWD, false>), grid, dim3(256), 0, st, a);
}
template <typename T>
void diffaug_launch_t(int group_c, bool bwd, bool vec, dim3 grid, hipStream_t st, const DiffAugArgs& a) {
  if (group_c == 1) {
    if (bwd) diffaug_launch<T, 1, true>(vec, grid, st, a);
    else diffaug_launch<T, 1, false>(vec, grid, st, a);
  } else {
    if (bwd) diffaug_launch<T, 3, true>(vec, grid, st, a);
    else diffaug_launch<T, 3, false>(vec, grid, st, a);
  }
}

}  // namespace

extern "C" int gan_diffaug_policy(const char* names, uint32_t* policy) {
  if (!names || !policy) return GAN_E_ARG;
  static const char* const kNames[4] = {"translation", "cutout", "brightness", "saturation"};
  uint32_t mask = 0;
  const char* p = names;
  if (!*p) { *policy = 0; return 0; }
  for (;;) {
    const char* e = strchr(p, ',');
    const size_t len = e ? (size_t)(e - p) : strlen(p);
    int hit = -1;
    for (int k = 0; k < 4; ++k)
      if (strlen(kNames[k]) == len && !strncmp(kNames[k], p, len)) hit = k;
    if (hit < 0) return GAN_E_ARG;
    mask |= 1u << hit;
    if (!e) break;
    p = e + 1;
  }
  *policy = mask;
  return 0;
}

extern "C" int gan_diffaug_draw(GanDiffAugParams* params, int32_t n, int32_t h, int32_t w, uint32_t policy, uint64_t seed,
                                uint32_t stream_id, int32_t* launches, gan_stream_t stream) {
  if (!params || !launches || n < 1 || n > 128 || h < 1 || w < 1 || (policy & ~15u)) return GAN_E_ARG;
  if (((uintptr_t)params & 3) || ((uintptr_t)launches & 3)) return GAN_E_ARG;
  GAN_LAUNCH(diffaug_draw_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, params, n, h, w, policy, seed, stream_id, launches);
  GAN_CHECK_LAUNCH();
  return 0;
}

extern "C" int gan_diffaug_apply(const GanDiffAugDesc* d, gan_stream_t stream) {
  if (!d || d->struct_size != sizeof(GanDiffAugDesc)) return GAN_E_ARG;
  if (!gan_dtype_ok(d->dtype) || !d->src.ptr || !d->dst.ptr || !d->params) return GAN_E_ARG;
  const GanTensor &s = d->src, &t = d->dst;
  if (s.n < 1 || s.h < 1 || s.w < 1 || s.c < 1 || s.pitch < s.c || t.pitch < t.c) return GAN_E_ARG;
  if (s.n != t.n || s.h != t.h || s.w != t.w || s.c != t.c) return GAN_E_ARG;
  if ((d->group_c != 1 && d->group_c != 3) || s.c % d->group_c || d->sample0 < 0 || (d->direction != 0 && d->direction != 1))
    return GAN_E_ARG;
  const size_t es = d->dtype == GAN_F32 ? 4 : 2;
  if ((((uintptr_t)s.ptr | (uintptr_t)t.ptr) & (es - 1)) || ((uintptr_t)d->params & 3)) return GAN_E_ARG;
  const long long pixels = (long long)s.h * s.w;
  if (pixels * (s.pitch > t.pitch ? s.pitch : t.pitch) >= 0x7fffffffLL || s.n > 65535) return GAN_E_SHAPE;   // 32-bit offsets inside an image
  DiffAugArgs a;
  a.src = s.ptr; a.dst = t.ptr; a.params = d->params;
  a.simg = pixels * s.pitch; a.dimg = pixels * t.pitch;
  a.h = s.h; a.w = s.w; a.c = s.c; a.spitch = s.pitch; a.dpitch = t.pitch; a.sample0 = d->sample0;
  a.wdiv = make_fastdiv((uint32_t)s.w);
  const bool vec = (size_t)s.pitch * es == 16 && !((uintptr_t)s.ptr & 15);       // (c <= pitch: the c channels lie inside the unit)
  const dim3 grid((unsigned)((pixels + 255) / 256), (unsigned)s.n);
  const bool bwd = d->direction == 1;
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == GAN_F32) diffaug_launch_t<float>(d->group_c, bwd, vec, grid, st, a);
  else if (d->dtype == GAN_BF16) diffaug_launch_t<bf16_t>(d->group_c, bwd, vec, grid, st, a);
  else diffaug_launch_t<f16_t>(d->group_c, bwd, vec, grid, st, a);
  GAN_CHECK_LAUNCH();
  return 0;
}
