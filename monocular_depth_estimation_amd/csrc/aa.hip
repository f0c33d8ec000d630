// Antialiased bilinear resize (include/mde_aa_abi.h): the filter of
// F.interpolate(mode='bilinear', antialias=True), which torchvision's
// transforms.Resize runs on float tensors, fused where infer.hip's infer_prep
// sits: uint8 HWC frames (or fp32 CHW images / planes) in, the resized view
// and, with views == 2, the resized horizontally flipped view out.  One launch,
// no scratch, capturable.
//
// Separable, horizontal first, fp32 intermediate, taps summed sequentially from
// j = 0 as ATen's CPU path does: fl(t0 w0), then acc = fma(t_j, w_j, acc)
// (aa_mac).  ATen writes `output += t * w`; its AVX2 / AVX512 builds, the ones
// a current x86 host dispatches to, contract that into a fused multiply-add,
// and with the fused form this kernel reproduces their output bit for bit
// wherever the weights are equal (tests/_aa_cases.py).  The weights themselves
// are NOT contracted: aaweights.h, shared with mde_aa_axis_weights.
//
// aa_kernel: one 256-thread block per 8 x 32 output tile of one frame, blocks
// striding over (frame, tile) pairs.  Three phases:
//   1. threads 0-31 fill the tile's column table, threads 32-39 its row table
//      (xmin, taps, normalised weights) in LDS; both views share them;
//   2. horizontal pass over the source rows the tile's 8 rows span (7 scale +
//      2 support + 1 at most): global -> fp32 slab in LDS laid out
//      [view][channel][source row][32 tile columns].  A tile's source pixels
//      leave global memory here, once, not once per output row;
//   3. vertical pass out of the slab, thread (r, x) = (tid / 32, tid % 32):
//      the 32 lanes of a half-wave read 32 consecutive floats of one slab row
//      (ds_read_b32 banks per 32-lane half: conflict-free) and write 128
//      contiguous bytes of the output.
// The column weights lie [tap][column] for the same reason; the row weights are
// read at one address per half-wave (a broadcast).
//
// The tile is 8 x 32 and not wider or taller: a row of 32 columns is the
// half-wave's bank group; 8 rows make the 256 threads one output pixel each in
// phase 3 while the slab rows shared by vertically adjacent outputs are loaded
// once; a taller tile would not fit the slab at scale 8 (75 source rows x 32 x
// 4 B x 3 channels = 28.8 KB per view).  The slab is dynamic LDS sized from the
// vertical scale; when both views do not fit kSlabBudget the block runs them
// one after the other (view 1 reads other source columns anyway).

#include "aaweights.h"
#include "common.h"
#include "mde_aa_abi.h"

namespace {

using mde::AaAxis;
using mde::kAaMaxTaps;

constexpr int kBlock = 256;
constexpr int kTR = 8, kTC = 32;         // output tile: rows x columns
constexpr int64_t kGridCap = 1 << 16;    // blocks launched at most; they stride over the rest
constexpr int kSlabBudget = 48 * 1024;   // dynamic LDS; the tables take 2.9 KB more

static_assert(kTR * kTC == kBlock, "phase 3: one output pixel per thread");

struct AaArgs {
  int64_t n, H, W, h, w;
  int64_t tiles_x, tiles;  // per frame
  AaAxis ax, ay;
  int views, vres;  // views in all / resident in the slab at once
  int span;         // slab rows allocated per (view, channel)
};

__device__ __forceinline__ float to_unit(uint8_t u) { return __fdiv_rn((float)u, 255.f); }
__device__ __forceinline__ float to_unit(float v) { return v; }

// Element (y, x, c) of one frame: uint8 frames are [H, W, C], float ones [C, H, W].
template <typename T, int C>
__device__ __forceinline__ float px(const T* __restrict__ f, const AaArgs& A, int y, int x, int c) {
  if constexpr (sizeof(T) == 1)
    return to_unit(f[((int64_t)y * A.W + x) * C + c]);
  else
    return to_unit(f[((int64_t)c * A.H + y) * A.W + x]);
}

// acc + t w, rounded once.
__device__ __forceinline__ float aa_mac(float acc, float t, float w) {
  return __fmaf_rn(t, w, acc);
}

// One entry of an axis table; an axis that keeps its size copies the sample.
__device__ __forceinline__ void table_entry(const AaAxis& a, int64_t out_size, int i, int* xmin,
                                            int* taps, float* w, int stride) {
  if (out_size == a.in) {
    *xmin = i;
    *taps = 1;
    w[0] = 1.f;
  } else {
    *taps = mde::aa_weights(a, i, xmin, w, stride);
  }
}

template <typename T, int C>
__global__ void __launch_bounds__(kBlock)
    aa_kernel(const T* __restrict__ frames, float* __restrict__ out, AaArgs A) {
  __shared__ int s_xmin[kTC], s_xn[kTC], s_ymin[kTR], s_yn[kTR];
  __shared__ float s_wx[kAaMaxTaps][kTC];
  __shared__ float s_wy[kTR][kAaMaxTaps];
  extern __shared__ float slab[];

  const int tid = threadIdx.x;
  const int64_t hw = A.h * A.w, total = A.n * A.tiles;
  const int Wm1 = (int)A.W - 1;
  for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const int64_t img = b / A.tiles;
    const int64_t t = b - img * A.tiles;
    const int64_t ty = t / A.tiles_x;
    const int y0 = (int)(ty * kTR), x0 = (int)((t - ty * A.tiles_x) * kTC);
    const int rows = (int)(A.h - y0 < kTR ? A.h - y0 : kTR);
    const int cols = (int)(A.w - x0 < kTC ? A.w - x0 : kTC);
    const T* f = frames + img * C * A.H * A.W;

    __syncthreads();  // the previous tile's readers are done with the tables and the slab
    if (tid < kTC) {
      if (tid < cols) table_entry(A.ax, A.w, x0 + tid, &s_xmin[tid], &s_xn[tid], &s_wx[0][tid], kTC);
    } else if (tid < kTC + kTR) {
      const int r = tid - kTC;
      if (r < rows) table_entry(A.ay, A.h, y0 + r, &s_ymin[r], &s_yn[r], &s_wy[r][0], 1);
    }
    __syncthreads();

    const int lo = s_ymin[0];
    int hi = lo;
    for (int r = 0; r < rows; ++r) hi = max(hi, s_ymin[r] + s_yn[r]);
    const int span = min(hi - lo, A.span);  // == hi - lo; the min keeps the slab in bounds

    for (int v0 = 0; v0 < A.views; v0 += A.vres) {
      if (v0) __syncthreads();  // view 0's vertical pass is done with the slab
      // ---- horizontal: item = (source row s, resident view vv, column x), all C channels:
      // the channels of a pixel share its address arithmetic and its weight, their
      // loads are independent (for uint8 frames three bytes of one cache line)
      const int items = span * A.vres * kTC;
      for (int it = tid; it < items; it += kBlock) {
        const int x = it & (kTC - 1);
        const int q = it / kTC;
        const int vv = A.vres == 2 ? (q & 1) : 0;
        const int s = A.vres == 2 ? (q >> 1) : q;
        if (x >= cols) continue;
        const int xm = s_xmin[x], nx = s_xn[x];
        const bool flip = (v0 + vv) != 0;
        const int y = lo + s, step = flip ? -1 : 1;
        int col = flip ? Wm1 - xm : xm;
        const float w0 = s_wx[0][x];
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = __fmul_rn(px<T, C>(f, A, y, col, c), w0);
        for (int j = 1; j < nx; ++j) {
          col += step;
          const float wj = s_wx[j][x];
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] = aa_mac(acc[c], px<T, C>(f, A, y, col, c), wj);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) slab[((vv * C + c) * A.span + s) * kTC + x] = acc[c];
      }
      __syncthreads();
      // ---- vertical: thread = output pixel (r, x) of the tile
      const int r = tid / kTC, x = tid & (kTC - 1);
      if (r < rows && x < cols) {
        const int ym = s_ymin[r] - lo;
        const int ny = min(s_yn[r], span - ym);
        const int64_t p = (int64_t)(y0 + r) * A.w + (x0 + x);
        for (int vv = 0; vv < A.vres; ++vv) {
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const float* col = slab + ((vv * C + c) * A.span + ym) * kTC + x;
            float acc = __fmul_rn(col[0], s_wy[r][0]);
            for (int j = 1; j < ny; ++j) acc = aa_mac(acc, col[j * kTC], s_wy[r][j]);
            out[(((int64_t)(v0 + vv) * A.n + img) * C + c) * hw + p] = acc;
          }
        }
      }
    }
  }
}

// Slab rows a tile can need: its first row starts at most 1 below c0 - support
// + .5, its last row ends at most at c7 + support + .5, c7 - c0 = 7 scale; the
// fp32 roundings of those sums are covered by the two extra rows.
int span_bound(const AaAxis& ay, int64_t H) {
  const double s = 7.0 * (double)ay.scale + 2.0 * (double)ay.support + 3.0;
  return (int)(s < (double)H ? s : (double)H);
}

bool size_limits_ok(int64_t n, int64_t c, int64_t H, int64_t W, int64_t h, int64_t w, int views) {
  const int64_t lim31 = (int64_t)1 << 31, lim30 = (int64_t)1 << 30;
  return n > 0 && H > 0 && W > 0 && h > 0 && w > 0 && n < lim31 && H < lim31 && h < lim31 &&
         n * H < lim31 && n * h < lim31 && views * c * (n * h) < lim31 && W < lim30 && w < lim30;
}

template <typename T, int C>
int launch(int kid, double bytes, const void* frames, void* out, int64_t n, int64_t H, int64_t W,
           int64_t h, int64_t w, int views, hipStream_t st) {
  AaArgs A{};
  A.n = n, A.H = H, A.W = W, A.h = h, A.w = w;
  A.tiles_x = mde::cdiv(w, kTC);
  A.tiles = A.tiles_x * mde::cdiv(h, kTR);
  A.ax = mde::aa_axis(W, w);
  A.ay = mde::aa_axis(H, h);
  A.views = views;
  A.span = span_bound(A.ay, H);
  const int per_view = A.span * C * kTC * (int)sizeof(float);
  A.vres = (views == 2 && 2 * per_view <= kSlabBudget) ? 2 : 1;
  if (per_view > kSlabBudget) return MDE_ERR_UNSUPPORTED;  // not within scale <= 8
  const int64_t blocks = n * A.tiles;
  MDE_LAUNCH(kid, bytes, st, (aa_kernel<T, C>),
             dim3((unsigned)(blocks < kGridCap ? blocks : kGridCap)), dim3(kBlock),
             (size_t)(A.vres * per_view), (const T*)frames, (float*)out, A);
  return MDE_OK;
}

}  // namespace

extern "C" {

int mde_aa_prep(const void* frames, void* out, int64_t n, int64_t H, int64_t W, int64_t h,
                int64_t w, int layout, int views, void* stream) {
  if (!frames || !out || (layout != 0 && layout != 1) || (views != 1 && views != 2) ||
      !size_limits_ok(n, 3, H, W, h, w, views))
    return MDE_ERR_INVALID_ARG;
  if (!mde::aa_axis_supported(H, h) || !mde::aa_axis_supported(W, w)) return MDE_ERR_UNSUPPORTED;
  const double out_bytes = 4.0 * views * 3.0 * n * (double)h * (double)w;
  hipStream_t st = (hipStream_t)stream;
  if (layout == 0)
    return launch<uint8_t, 3>(mde::K_INFER_PREP, 3.0 * n * (double)H * (double)W + out_bytes,
                              frames, out, n, H, W, h, w, views, st);
  return launch<float, 3>(mde::K_INFER_PREP, 12.0 * n * (double)H * (double)W + out_bytes, frames,
                          out, n, H, W, h, w, views, st);
}

int mde_aa_resize_fwd(const void* x, void* y, int64_t planes, int64_t H, int64_t W, int64_t h,
                      int64_t w, int dtype, void* stream) {
  if (dtype != MDE_F32) return MDE_ERR_UNSUPPORTED;
  if (!x || !y || !size_limits_ok(planes, 1, H, W, h, w, 1)) return MDE_ERR_INVALID_ARG;
  if (!mde::aa_axis_supported(H, h) || !mde::aa_axis_supported(W, w)) return MDE_ERR_UNSUPPORTED;
  return launch<float, 1>(mde::K_BILINEAR_FWD,
                          4.0 * planes * ((double)H * (double)W + (double)h * (double)w), x, y,
                          planes, H, W, h, w, 1, (hipStream_t)stream);
}

int mde_aa_axis_weights(int64_t in, int64_t out, int32_t* xmin, int32_t* xsize, float* weights,
                        int64_t stride) {
  const int64_t lim31 = (int64_t)1 << 31;
  if (!xmin || !xsize || !weights || in <= 0 || out <= 0 || in >= lim31 || out >= lim31 ||
      stride <= 0)
    return MDE_ERR_INVALID_ARG;
  if (!mde::aa_axis_supported(in, out)) return MDE_ERR_UNSUPPORTED;
  const AaAxis a = mde::aa_axis(in, out);
  // the largest tap count first, so that nothing is written when stride is too small
  int most = 0;
  float w[kAaMaxTaps];
  for (int64_t i = 0; i < out; ++i) {
    int lo;
    const int taps = mde::aa_weights(a, (int)i, &lo, w, 1);
    most = taps > most ? taps : most;
  }
  if (stride < most) return MDE_ERR_INVALID_ARG;
  for (int64_t i = 0; i < out; ++i) {
    int lo;
    float* wi = weights + i * stride;
    const int taps = mde::aa_weights(a, (int)i, &lo, w, 1);
    for (int64_t j = 0; j < stride; ++j) wi[j] = j < taps ? w[j] : 0.f;
    xmin[i] = lo;
    xsize[i] = taps;
  }
  return most;
}

}  // extern "C"
