// Bilinear source-index and weight arithmetic shared by resize.hip and
// evalpair.hip.
//
// Index math follows ATen's area_pixel_compute_source_index so the sampled
// pixels and the interpolation weights are the ones F.interpolate uses.
// Products are written with __fmul_rn/__fadd_rn so hipcc cannot contract them
// into FMAs: a contracted source index could floor to a different pixel than
// the reference near integer boundaries.
#pragma once

#include <hip/hip_runtime.h>

namespace mde {

struct Lin {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ float src_index(float scale, int dst, int align) {
  if (align) return __fmul_rn(scale, (float)dst);
  float s = __fadd_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), -0.5f);
  return s < 0.f ? 0.f : s;
}

__device__ __forceinline__ Lin lin_index(float scale, int dst, int in_size,
                                         int align) {
  const float s = src_index(scale, dst, align);
  int i0 = (int)s;  // s >= 0, so truncation is floor
  if (i0 > in_size - 1) i0 = in_size - 1;
  const int i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  float l1 = __fadd_rn(s, -(float)i0);
  l1 = fminf(fmaxf(l1, 0.f), 1.f);
  return {i0, i1, __fadd_rn(1.f, -l1), l1};
}

// l0 a + l1 b with the rounding pinned (one product, one fused multiply-add):
// the fp32 and bf16-storage instantiations of a kernel must not let the
// compiler contract the sum differently (bf16 results == rounded fp32 ones).
__device__ __forceinline__ float lerp2(const Lin& L, float a, float b) {
  return __fmaf_rn(L.l1, b, __fmul_rn(L.l0, a));
}

}  // namespace mde
