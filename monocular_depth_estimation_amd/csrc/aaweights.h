// Weight arithmetic of the antialiased bilinear resize (aa.hip,
// include/mde_aa_abi.h), shared by the kernel and the host query
// mde_aa_axis_weights so that the two cannot drift apart.
//
// The filter is ATen's (F.interpolate(mode='bilinear', antialias=True)): a
// triangle per axis, widened by the scale when downscaling, every step in fp32.
// Each product, sum and quotient is rounded to fp32 on its own (aa_mul /
// aa_add / aa_div: uncontracted operators on the host and the device), for
// lerp.h's reason: a contracted or wider `center` moves xmin.  At 1242 -> 640 a
// float64 version of the same formula is 1.9e-5 away from ATen's weights; this
// one is within 2^-23.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mde {

constexpr float kAaMaxScale = 8.f;  // per-axis in / out supported
constexpr int kAaMaxTaps = 17;      // (int)(c + 8 + .5) - (int)(c - 8 + .5) <= 17

// `#pragma clang fp contract(off)` and plain operators on both sides, not
// __fmul_rn / __fadd_rn: unless OCML_BASIC_ROUNDED_OPERATIONS is defined the
// toolchain's header defines those two as `x * y` and `x + y`, which carry the
// translation unit's contraction mode into the caller once inlined.  With them
// the device fused center's product into the sums that follow it, and at
// 18 -> 7 its weights left the host's (and ATen's) by an ulp.
__host__ __device__ inline float aa_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__host__ __device__ inline float aa_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__host__ __device__ inline float aa_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);  // IEEE division
#else
  return a / b;
#endif
}

struct AaAxis {
  float scale, support, invscale;
  int in;
};

__host__ __device__ inline AaAxis aa_axis(int64_t in, int64_t out) {
  const float scale = aa_div((float)in, (float)out);
  const bool down = scale >= 1.f;
  return {scale, down ? scale : 1.f, down ? aa_div(1.f, scale) : 1.f, (int)in};
}

// in / out within the supported range (the comparison ATen's arithmetic would
// make: on the fp32 scale).
__host__ __device__ inline bool aa_axis_supported(int64_t in, int64_t out) {
  return aa_div((float)in, (float)out) <= kAaMaxScale;
}

// Output index i of an axis: first source index *xmin, the normalised weights
// w[0], w[stride], .. of sources xmin .. xmin + taps - 1, and taps as the return
// value (1 .. kAaMaxTaps; end taps may carry weight 0).
__host__ __device__ inline int aa_weights(const AaAxis& A, int i, int* xmin, float* w,
                                          int stride) {
  const float center = aa_mul(A.scale, aa_add((float)i, 0.5f));
  int lo = (int)aa_add(aa_add(center, -A.support), 0.5f);
  if (lo < 0) lo = 0;
  const int64_t end = (int64_t)aa_add(aa_add(center, A.support), 0.5f);  // may pass 2^31
  const int hi = end > A.in ? A.in : (int)end;
  int taps = hi - lo;
  if (taps > kAaMaxTaps) taps = kAaMaxTaps;  // cannot happen at scale <= 8; keeps w[] in bounds
  if (taps < 1) {                            // nor this: center lies inside [0, in]
    lo = lo > A.in - 1 ? A.in - 1 : lo;
    taps = 1;
  }
  float total = 0.f;
  for (int j = 0; j < taps; ++j) {
    float a = aa_mul(aa_add(aa_add((float)(j + lo), -center), 0.5f), A.invscale);
    a = a < 0.f ? -a : a;
    const float t = a < 1.f ? aa_add(1.f, -a) : 0.f;
    w[j * stride] = t;
    total = aa_add(total, t);
  }
  if (total != 0.f)
    for (int j = 0; j < taps; ++j) w[j * stride] = aa_div(w[j * stride], total);
  else
    w[0] = 1.f;
  *xmin = lo;
  return taps;
}

}  // namespace mde
