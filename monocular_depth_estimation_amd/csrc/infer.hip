// The two ends of the deployed GuideDepth path (include/mde_infer_abi.h;
// src/GuideDepth/inference.py:215-227 and :234,245-247).
//
// infer_prep_kernel: camera frames (uint8 HWC) or tensor images (fp32 CHW) to
// the network's input, both evaluation views at once: to_tensor, the horizontal
// flip and the bilinear downscale.  A thread owns one output pixel (y, x) of one
// frame and writes its three channels for view 0 and, with views == 2, for view
// 1.  Both views share the row and column weights: view 1 is the resize of the
// flipped frame, whose columns i0, i1 are the frame's W-1-i0, W-1-i1.
//
// infer_depth_kernel: the network's output to metres at the frame's resolution.
// D (invdepth.h) on the four source samples, then the interpolation: exactly
// evalpair.hip's sample(), written out instead of compared.
//
// Both are gathers bound by memory traffic: the source rows a block touches are
// a few cache lines read many times, the output leaves coalesced.  Every
// interpolation is lerp.h's (lin_index, lerp2), so the fused path and the
// composition it replaces (bilinear_fwd_kernel of resize.hip) give the same
// bits.  One launch each; blocks stride over (frame, 256-pixel chunk) pairs so
// that no size within the documented limits exceeds the grid.

#include "common.h"
#include "invdepth.h"
#include "lerp.h"
#include "mde_infer_abi.h"

namespace {

using mde::inv_depth;
using mde::Lin;
using mde::lerp2;
using mde::lin_index;

constexpr int kBlock = 256;
constexpr int64_t kGridCap = 1 << 16;  // blocks launched at most; they stride over the rest

struct PrepArgs {
  int64_t n, H, W, h, w;
  int64_t chunks;  // 256-pixel chunks of one frame's h * w output pixels
  float sh, sw;
  int views, ident;
};

// to_tensor of one sample: uint8 -> fl(u / 255) (IEEE division, as ATen's div);
// a float image is taken as it is.
__device__ __forceinline__ float to_unit(uint8_t u) { return __fdiv_rn((float)u, 255.f); }
__device__ __forceinline__ float to_unit(float v) { return v; }

// Element (y, x, c) of frame `img`: uint8 frames are [H, W, 3], float images [3, H, W].
template <typename T>
__device__ __forceinline__ float px(const T* __restrict__ img, const PrepArgs& A, int y, int x,
                                    int c);
template <>
__device__ __forceinline__ float px<uint8_t>(const uint8_t* __restrict__ img, const PrepArgs& A,
                                             int y, int x, int c) {
  return to_unit(img[((int64_t)y * A.W + x) * 3 + c]);
}
template <>
__device__ __forceinline__ float px<float>(const float* __restrict__ img, const PrepArgs& A, int y,
                                           int x, int c) {
  return to_unit(img[((int64_t)c * A.H + y) * A.W + x]);
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
    infer_prep_kernel(const T* __restrict__ frames, float* __restrict__ out, PrepArgs A) {
  const int64_t hw = A.h * A.w, total = A.n * A.chunks;
  const int Wm1 = (int)A.W - 1;
  for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const int64_t img = b / A.chunks;
    const int64_t p = (b - img * A.chunks) * kBlock + threadIdx.x;
    if (p >= hw) continue;
    const int y = (int)(p / A.w), x = (int)(p - (int64_t)y * A.w);
    const T* f = frames + img * 3 * A.H * A.W;
    float* o0 = out + img * 3 * hw + p;
    float* o1 = out + (A.n + img) * 3 * hw + p;
    if (A.ident) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        o0[c * hw] = px(f, A, y, x, c);
        if (A.views == 2) o1[c * hw] = px(f, A, y, Wm1 - x, c);
      }
      continue;
    }
    const Lin Hy = lin_index(A.sh, y, (int)A.H, 0);
    const Lin Wx = lin_index(A.sw, x, (int)A.W, 0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o0[c * hw] = lerp2(Hy, lerp2(Wx, px(f, A, Hy.i0, Wx.i0, c), px(f, A, Hy.i0, Wx.i1, c)),
                         lerp2(Wx, px(f, A, Hy.i1, Wx.i0, c), px(f, A, Hy.i1, Wx.i1, c)));
      if (A.views == 2) {
        const int j0 = Wm1 - Wx.i0, j1 = Wm1 - Wx.i1;  // the flipped frame's columns i0, i1
        o1[c * hw] = lerp2(Hy, lerp2(Wx, px(f, A, Hy.i0, j0, c), px(f, A, Hy.i0, j1, c)),
                           lerp2(Wx, px(f, A, Hy.i1, j0, c), px(f, A, Hy.i1, j1, c)));
      }
    }
  }
}

struct DepthArgs {
  int64_t n, ph, pw, H, W;
  int64_t chunks;  // 256-pixel chunks of one map's H * W pixels
  float sh, sw;
  float maxd, lo;
  int ident;
};

__global__ void __launch_bounds__(kBlock)
    infer_depth_kernel(const float* __restrict__ inv, float* __restrict__ depth, DepthArgs A) {
  const int64_t HW = A.H * A.W, total = A.n * A.chunks;
  for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const int64_t img = b / A.chunks;
    const int64_t p = (b - img * A.chunks) * kBlock + threadIdx.x;
    if (p >= HW) continue;
    const float* plane = inv + img * A.ph * A.pw;
    float* o = depth + img * HW + p;
    if (A.ident) {
      *o = inv_depth(plane[p], A.maxd, A.lo);
      continue;
    }
    const int y = (int)(p / A.W), x = (int)(p - (int64_t)y * A.W);
    const Lin Hy = lin_index(A.sh, y, (int)A.ph, 0);
    const Lin Wx = lin_index(A.sw, x, (int)A.pw, 0);
    const float* r0 = plane + (int64_t)Hy.i0 * A.pw;
    const float* r1 = plane + (int64_t)Hy.i1 * A.pw;
    const float a = inv_depth(r0[Wx.i0], A.maxd, A.lo), bb = inv_depth(r0[Wx.i1], A.maxd, A.lo);
    const float c = inv_depth(r1[Wx.i0], A.maxd, A.lo), d = inv_depth(r1[Wx.i1], A.maxd, A.lo);
    *o = lerp2(Hy, lerp2(Wx, a, bb), lerp2(Wx, c, d));
  }
}

unsigned grid_for(int64_t blocks) { return (unsigned)(blocks < kGridCap ? blocks : kGridCap); }

}  // namespace

extern "C" {

int mde_infer_prep(const void* frames, void* out, int64_t n, int64_t H, int64_t W, int64_t h,
                   int64_t w, int layout, int views, void* stream) {
  const int64_t lim31 = (int64_t)1 << 31, lim30 = (int64_t)1 << 30;
  if (!frames || !out || n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 ||
      (layout != 0 && layout != 1) || (views != 1 && views != 2) || n >= lim31 || H >= lim31 ||
      h >= lim31 || n * H >= lim31 || n * h >= lim31 || views * 3 * (n * h) >= lim31 ||
      W >= lim30 || w >= lim30)
    return MDE_ERR_INVALID_ARG;
  PrepArgs A{n, H, W, h, w, mde::cdiv(h * w, kBlock), (float)H / (float)h, (float)W / (float)w,
             views, (h == H && w == W) ? 1 : 0};
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = n * A.chunks;
  const double out_bytes = 4.0 * views * 3.0 * n * (double)h * (double)w;
  if (layout == 0)
    MDE_LAUNCH(mde::K_INFER_PREP, 3.0 * n * (double)H * (double)W + out_bytes, st,
               infer_prep_kernel<uint8_t>, dim3(grid_for(blocks)), dim3(kBlock), 0,
               (const uint8_t*)frames, (float*)out, A);
  else
    MDE_LAUNCH(mde::K_INFER_PREP, 12.0 * n * (double)H * (double)W + out_bytes, st,
               infer_prep_kernel<float>, dim3(grid_for(blocks)), dim3(kBlock), 0,
               (const float*)frames, (float*)out, A);
  return MDE_OK;
}

int mde_infer_depth(const void* inv, void* depth, int64_t n, int64_t ph, int64_t pw, int64_t H,
                    int64_t W, float max_depth, int dtype, void* stream) {
  if (dtype != MDE_F32) return MDE_ERR_UNSUPPORTED;
  const int64_t lim31 = (int64_t)1 << 31, lim30 = (int64_t)1 << 30;
  if (!inv || !depth || n <= 0 || ph <= 0 || pw <= 0 || H <= 0 || W <= 0 || n >= lim31 ||
      H >= lim31 || ph >= lim31 || n * H >= lim31 || W >= lim30 || n * ph >= lim31 || pw >= lim30)
    return MDE_ERR_INVALID_ARG;
  DepthArgs A{n, ph, pw, H, W, mde::cdiv(H * W, kBlock), (float)ph / (float)H,
              (float)pw / (float)W, max_depth, (float)((double)max_depth / 100.0),
              (ph == H && pw == W) ? 1 : 0};
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = n * A.chunks;
  MDE_LAUNCH(mde::K_INFER_DEPTH, 4.0 * n * ((double)ph * pw + (double)H * W), st,
             infer_depth_kernel, dim3(grid_for(blocks)), dim3(kBlock), 0, (const float*)inv,
             (float*)depth, A);
  return MDE_OK;
}

}  // extern "C"
