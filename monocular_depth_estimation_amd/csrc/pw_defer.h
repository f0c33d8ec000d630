// A BatchNorm + ReLU backward apply pass evaluated on a consumer's operand
// load: the pass is a pointwise function of the upstream gradient g, the
// BatchNorm's input y and a few per-channel constants, so a kernel that reads
// d/dy exactly once can form it itself and d/dy is never written.  One text
// for every such consumer (skip.hip's 1x1 conv backward, conv3x3.hip's guide
// weight gradient), so that they all round as the apply kernels do.
#pragma once

#include <hip/hip_runtime.h>

struct PwDeferCo {
  float sc, sh, c2, c3, c4, P, Q;  // DEF 3: P = w1[o]
};

//   DEF 1 (bn_bwd_apply_*_kernel):  G = A [y sc + sh > 0] g + B y + D
//   DEF 2 (sebn_bwd_apply_kernel):  G = [y sc + sh > 0] (P g + Q) + Tc (y - mu) + R
//   DEF 3: DEF 1 whose g is first multiplied by P (rounded on its own)
// (c2, c3, c4) = (A, B, D) or (mu, Tc, R).
template <int DEF>
__device__ __forceinline__ float pw_defer1(float g, float y, const PwDeferCo& k) {
#pragma clang fp contract(off)
  if constexpr (DEF == 1 || DEF == 3) {
    if constexpr (DEF == 3) g = k.P * g;  // skip_bwd_c1_kernel's stored w[k] * g
    // the operations bn_bwd_apply_plane_kernel's `A * e + B * v + D` compiles
    // to (mask from fma(x, sc, sh); fma(B, v, A * e), then + D), spelled out
    // so that the fold leaves every bit of the step's result where it was
    const float e = fmaf(y, k.sc, k.sh) > 0.f ? g : 0.f;
    return fmaf(k.c3, y, k.c2 * e) + k.c4;
  } else {
    const float z = fmaf(y, k.sc, k.sh);
    return (z > 0.f ? fmaf(k.P, g, k.Q) : 0.f) + fmaf(k.c3, y - k.c2, k.c4);
  }
}

template <int DEF>
__device__ __forceinline__ float4 pw_defer4(float4 g, float4 y, const PwDeferCo& k) {
  return make_float4(pw_defer1<DEF>(g.x, y.x, k), pw_defer1<DEF>(g.y, y.y, k),
                     pw_defer1<DEF>(g.z, y.z, k), pw_defer1<DEF>(g.w, y.w, k));
}
