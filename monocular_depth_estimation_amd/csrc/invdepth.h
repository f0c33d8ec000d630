// The depth of an inverse-depth sample, D(v) = clamp(maxd / v, lo, maxd), shared by
// evalpair.hip (which compares it with the ground truth) and infer.hip (which
// writes it): one definition, so both give the same bits.
#pragma once

#include <hip/hip_runtime.h>

namespace mde {

// torch.clamp(maxd / v, lo, maxd).  `maxDepth / depth` with a Python number on the
// left is Tensor.__rtruediv__, which ATen evaluates as depth.reciprocal() * maxDepth:
// two roundings, reproduced here so the depth is bit-for-bit the one the reference's
// inverse_depth_norm (and the unfused composition of this package's ops) gives.
__device__ __forceinline__ float inv_depth(float v, float maxd, float lo) {
  float d = __fmul_rn(__frcp_rn(v), maxd);
  d = d < lo ? lo : d;
  d = d > maxd ? maxd : d;
  return d;
}

}  // namespace mde
