// The SSIM definition shared by quality.hip (the metric) and dssim.hip (the loss): tf.image.ssim's window and constants, and the
// separately rounded products that make SSIM exactly 1 for a == b.  One definition, so that the two agree bit for bit per map position.
#pragma once
#include <math.h>
#include "common.h"

constexpr int SSIM_K = 11;            // filter taps
constexpr float SSIM_C1 = 1e-4f;      // (0.01 * max_val)^2
constexpr float SSIM_C2 = 9e-4f;      // (0.03 * max_val)^2
constexpr int SSIM_MAX_EDGE = 4096;   // largest h, w

// Gaussian window, sigma 1.5, normalised in double on the host
static inline void ssim_window(float* g) {
  double v[SSIM_K], sum = 0.0;
  for (int k = 0; k < SSIM_K; ++k) sum += v[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
  for (int k = 0; k < SSIM_K; ++k) g[k] = (float)(v[k] / sum);
}

// products and sums whose roundings must not be fused into the operation that follows: with a == b the sums below are then exact
// doubles of each other and SSIM comes out as exactly 1.  __fmul_rn / __fadd_rn do NOT give that on this compiler - they are plain
// x * y, x + y, which the default -ffp-contract=fast-honor-pragmas fuses into v_fma where it likes, differently from kernel to
// kernel - so the contraction is switched off here, per operation: these compile to v_mul_f32 / v_add_f32 / v_sub_f32.
__device__ __forceinline__ float q_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float q_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ float q_sub(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}

// luminance and contrast-structure terms of one map position from the CENTRED moments (quality.hip: x' = 0.5 * x, u = x' + 0.5):
// ma = F(x'), mb = F(y'), eab = F(x'y'), esq = F(x'^2 + y'^2)
struct SsimTerms {
  float mx, my, lum_d, cs_d, lum, cs;
};
__device__ __forceinline__ SsimTerms ssim_terms(float ma, float mb, float eab, float esq) {
  SsimTerms t;
  t.mx = q_add(ma, 0.5f);
  t.my = q_add(mb, 0.5f);
  const float lum_n = q_add(q_mul(2.f, q_mul(t.mx, t.my)), SSIM_C1);
  t.lum_d = q_add(q_add(q_mul(t.mx, t.mx), q_mul(t.my, t.my)), SSIM_C1);
  const float cs_n = q_add(q_sub(q_mul(2.f, eab), q_mul(2.f, q_mul(ma, mb))), SSIM_C2);
  t.cs_d = q_add(q_sub(esq, q_add(q_mul(ma, ma), q_mul(mb, mb))), SSIM_C2);
  t.lum = lum_n / t.lum_d;
  t.cs = cs_n / t.cs_d;
  return t;
}
