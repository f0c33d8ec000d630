// GuideDepth evaluation tail in one pass (include/mde_eval_abi.h).
//
// Replaces, per test image and for both views of src/GuideDepth/evaluate.py
// (the image :104-105 and its horizontal flip :93-94,107-108):
// inverse_depth_norm (:174-177), the bilinear upscale to the ground-truth
// resolution (:113-116), the dataset crop (:129-132) and Result.evaluate's
// reductions (metrics.py:41-62).  Each thread reads one ground-truth pixel
// gt(y, j) once and serves both views with it: view 0 compares it with the
// upsampled prediction at (y, j); view 1 is the flipped frame's pixel
// (y, x = W-1-j), whose ground truth flip(gt)(y, x) is this same gt(y, j), so
// no flipped copy of gt exists.  The crop window applies to each frame's own
// coordinates.  Nothing is written but [n, 2, 16] doubles.
//
// The 16 sums per (image, view) are those of metrics.hip (same layout, fp32
// per-pixel terms, double accumulation; the logarithms correctly rounded:
// acc_add below).  The depth D(v) = clamp(maxd / v, maxd / 100, maxd), rounded
// as torch rounds it (inv_depth, invdepth.h), is applied to the four source samples
// before the interpolation (the reference resizes the clamped depth) with
// torch.clamp's semantics: 0 -> maxd, negative -> maxd / 100, NaN stays NaN.
// The interpolation is resize.hip's arithmetic (lerp.h).  The source
// samples are gathered from the small prediction (a block's kRows rows read a
// handful of source rows: cache hits), the gt rows are read coalesced.
//
// Reduction: a block owns kRows rows of ONE image and writes a partial
// [2][16]; one block per image sums that image's partials in a fixed order.
// No atomics; image i's numbers depend on image i's data alone, not on n or i.
// Algorithmic HBM bytes: 4 n (H W + 2 ph pw).

#include <cmath>

#include "common.h"
#include "invdepth.h"
#include "lerp.h"
#include "mde_eval_abi.h"

namespace {

using mde::inv_depth;
using mde::Lin;
using mde::lerp2;
using mde::lin_index;

constexpr int kSums = 16;
constexpr int kUsed = 14;
constexpr int kRows = 4;
constexpr int kOut = 2 * kSums;  // doubles per image: [view][16]
constexpr int kSeg = 8;          // the final kernel's partial segments per output

struct PairArgs {
  int64_t ph, pw, H, W;
  int64_t bpi;  // blocks per image
  float sh, sw;
  float maxd, lo;
  int ident;           // ph == H && pw == W: the sample itself
  int c0, c1, c2, c3;  // crop rows [c0, c1), cols [c2, c3)
};

struct Acc {
  unsigned c[4];
  double s[kUsed - 4];
};

__device__ __forceinline__ void acc_zero(Acc& a) {
#pragma unroll
  for (int i = 0; i < 4; ++i) a.c[i] = 0u;
#pragma unroll
  for (int i = 0; i < kUsed - 4; ++i) a.s[i] = 0.0;
}

// metrics.hip's per-pixel terms (fp32) and accumulation (double).  The logarithms are
// the correctly rounded fp32 values (taken in double, rounded once), as numpy's and
// ATen's float32 log are to within an ulp and without a bias: the device library's
// logf / log10f measured a relative bias of 3e-8 over a 480x640 map, which the
// square-free sums 8 and 9 keep in full and which is above the reference's own
// float32 error (tests/test_gpu_evaluater.py).
__device__ __forceinline__ void acc_add(Acc& a, float p, float g) {
  const float th = fmaxf(g / p, p / g);
  const float d = g - p;
  const float lp = (float)log((double)p), lg = (float)log((double)g);
  const float l10 = (float)log10((double)p) - (float)log10((double)g);
  const float ip = 1.f / p - 1.f / g;
  a.c[0] += 1u;
  a.c[1] += th < 1.25f ? 1u : 0u;
  a.c[2] += th < 1.25f * 1.25f ? 1u : 0u;
  a.c[3] += th < 1.25f * 1.25f * 1.25f ? 1u : 0u;
  a.s[0] += (double)(d * d);
  a.s[1] += (double)((lg - lp) * (lg - lp));
  a.s[2] += (double)(fabsf(d) / g);
  a.s[3] += (double)(d * d / g);
  a.s[4] += (double)(lp - lg);
  a.s[5] += (double)fabsf(l10);
  a.s[6] += (double)fabsf(d);
  a.s[7] += (double)(l10 * l10);
  a.s[8] += (double)fabsf(ip);
  a.s[9] += (double)(ip * ip);
}

__device__ __forceinline__ float sample(const float* __restrict__ plane, const PairArgs& A,
                                        const Lin& Hy, const Lin& Wx, int y, int x) {
  if (A.ident) return inv_depth(plane[(int64_t)y * A.pw + x], A.maxd, A.lo);
  const float* r0 = plane + (int64_t)Hy.i0 * A.pw;
  const float* r1 = plane + (int64_t)Hy.i1 * A.pw;
  const float a = inv_depth(r0[Wx.i0], A.maxd, A.lo), b = inv_depth(r0[Wx.i1], A.maxd, A.lo);
  const float c = inv_depth(r1[Wx.i0], A.maxd, A.lo), d = inv_depth(r1[Wx.i1], A.maxd, A.lo);
  return lerp2(Hy, lerp2(Wx, a, b), lerp2(Wx, c, d));
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block b of image i: gt rows [b kRows, b kRows + kRows) of that image.
__global__ void __launch_bounds__(256)
    eval_pair_partial_kernel(const float* __restrict__ inv, const float* __restrict__ inv_flip,
                             const float* __restrict__ gt, PairArgs A, double* __restrict__ part) {
  __shared__ double red[4][kOut];
  const int64_t img = blockIdx.x / A.bpi;
  const int y0 = (int)(blockIdx.x - img * A.bpi) * kRows;
  const int W = (int)A.W, H = (int)A.H;
  const float* p0 = inv + img * A.ph * A.pw;
  const float* p1 = inv_flip ? inv_flip + img * A.ph * A.pw : nullptr;
  const float* gp = gt + img * A.H * A.W;
  Acc a0, a1;
  acc_zero(a0);
  acc_zero(a1);
  const int ya = y0 > A.c0 ? y0 : A.c0;
  const int yb = min(min(y0 + kRows, A.c1), H);
  for (int j = threadIdx.x; j < W; j += 256) {
    const int x = W - 1 - j;  // the flipped frame's column served by gt(y, j)
    const bool in0 = j >= A.c2 && j < A.c3;
    const bool in1 = p1 != nullptr && x >= A.c2 && x < A.c3;
    if (!in0 && !in1) continue;
    const Lin W0 = lin_index(A.sw, j, (int)A.pw, 0);
    const Lin W1 = lin_index(A.sw, x, (int)A.pw, 0);
    for (int y = ya; y < yb; ++y) {
      const Lin Hy = lin_index(A.sh, y, (int)A.ph, 0);
      const float g = gp[(int64_t)y * W + j];
      if (in0) acc_add(a0, sample(p0, A, Hy, W0, y, j), g);
      if (in1) acc_add(a1, sample(p1, A, Hy, W1, y, x), g);
    }
  }
  // wave sums of the 2 x 14 values, then the four waves in a fixed order
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const Acc& a = v ? a1 : a0;
#pragma unroll
    for (int i = 0; i < kUsed; ++i) {
      const double t = wave_sum_d(i < 4 ? (double)a.c[i] : a.s[i - 4]);
      if (lane == 0) red[wid][v * kSums + i] = t;
    }
  }
  __syncthreads();
  if (threadIdx.x < kOut) {
    const int i = threadIdx.x;
    const double t = (i & (kSums - 1)) < kUsed
                         ? (red[0][i] + red[1][i]) + (red[2][i] + red[3][i])
                         : 0.0;
    part[(int64_t)blockIdx.x * kOut + i] = t;
  }
}

// Block i: sums[i][v][k] = sum_b part[i][b][v][k], b in a fixed order (kSeg
// strided segments, then the segments in order).
__global__ void __launch_bounds__(kOut * kSeg)
    eval_pair_final_kernel(const double* __restrict__ part, int64_t bpi,
                           double* __restrict__ sums) {
  __shared__ double red[kSeg][kOut];
  const int o = threadIdx.x & (kOut - 1), seg = threadIdx.x / kOut;
  const double* p = part + (int64_t)blockIdx.x * bpi * kOut + o;
  double v = 0.0;
  for (int64_t b = seg; b < bpi; b += kSeg) v += p[b * kOut];
  red[seg][o] = v;
  __syncthreads();
  if (threadIdx.x < kOut) {
    double t = red[0][o];
#pragma unroll
    for (int s = 1; s < kSeg; ++s) t += red[s][o];
    sums[(int64_t)blockIdx.x * kOut + o] = t;
  }
}

int64_t blocks_per_image(int64_t H) { return mde::cdiv(H, kRows); }

}  // namespace

extern "C" {

size_t mde_eval_pair_workspace(int64_t n, int64_t H, int64_t W) {
  if (n <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)(sizeof(double) * kOut * n * blocks_per_image(H));
}

int mde_eval_pair_sums(const void* inv_pred, const void* inv_pred_flip, const void* gt, int64_t n,
                       int64_t ph, int64_t pw, int64_t H, int64_t W, float max_depth,
                       const int32_t* crop, void* workspace, double* sums, int dtype,
                       void* stream) {
  if (dtype != MDE_F32) return MDE_ERR_UNSUPPORTED;
  const int64_t lim31 = (int64_t)1 << 31, lim30 = (int64_t)1 << 30;
  if (!inv_pred || !gt || !workspace || !sums || n <= 0 || ph <= 0 || pw <= 0 || H <= 0 ||
      W <= 0 || n * H >= lim31 || W >= lim30 || n * ph >= lim31 || pw >= lim30)
    return MDE_ERR_INVALID_ARG;
  PairArgs A{ph, pw, H, W, blocks_per_image(H), (float)ph / (float)H, (float)pw / (float)W,
             max_depth, (float)((double)max_depth / 100.0), (ph == H && pw == W) ? 1 : 0,
             0, (int)H, 0, (int)W};
  if (crop) {
    if (crop[0] < 0 || crop[0] > crop[1] || crop[1] > H || crop[2] < 0 || crop[2] > crop[3] ||
        crop[3] > W)
      return MDE_ERR_INVALID_ARG;
    A.c0 = crop[0];
    A.c1 = crop[1];
    A.c2 = crop[2];
    A.c3 = crop[3];
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = n * A.bpi;
  double* part = (double*)workspace;
  MDE_LAUNCH(mde::K_EVAL_PAIR, 4.0 * n * ((double)H * W + 2.0 * ph * pw), st,
             eval_pair_partial_kernel, dim3((unsigned)blocks), dim3(256), 0,
             (const float*)inv_pred, (const float*)inv_pred_flip, (const float*)gt, A, part);
  MDE_LAUNCH(mde::K_EVAL_PAIR_FINAL, 8.0 * kOut * (blocks + n), st, eval_pair_final_kernel,
             dim3((unsigned)n), dim3(kOut * kSeg), 0, part, A.bpi, sums);
  return MDE_OK;
}

}  // extern "C"
