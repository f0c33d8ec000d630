// Image logging (include/mde_viz_abi.h): torchvision's make_grid fused with the
// reference's colorize (src/train.py:160-194, src/utils.py:69-96), and
// make_grid(normalize=True) for the RGB batch.  One launch each, no scratch,
// capturable.
//
// Both kernels are streaming passes over the GRID: a thread owns four
// horizontally adjacent grid pixels (consecutive in the flattened Hg x Wg plane,
// so a quad may run over a row end), finds for each the map pixel it shows or
// that it is a pad pixel, and writes one packed word per output plane: four
// colour bytes as one 32-bit store (viz_colorize_grid_kernel), four floats as
// one 16-byte store (viz_image_grid_kernel).
//
// Alignment.  Neither Wg nor Hg * Wg is a multiple of four in general, so plane
// c of an output starts at any address mod 4 (mod 16 for floats).  A plane is
// therefore cut into quads from the plane's own ALIGNED word grid: with
// s = (address of the plane's first element, in elements) mod 4, thread t owns
// the plane's pixels 4 t - s ... 4 t - s + 3.  Every quad is one aligned word;
// only the first and the last quad of a plane are partial, and those are
// written element by element.  The quad's values depend on s, so they are
// recomputed for a plane whose s differs from the previous plane's -- never,
// when Hg * Wg is a multiple of four and the outputs are aligned, which is the
// case of every even-sized batch of maps (486 x 1934, 966 x 3854).
//
// viz_colorize_grid_kernel computes the colour index of x' (and of |x' - y|)
// once per pixel and looks the three channels up in an LDS copy of the table,
// one packed RGB word per entry (entry 256: the NaN colour), so a pixel costs
// one ds_read_b32 per output whatever the plane count.
//
// The arithmetic is include/mde_viz_abi.h's, step by step in fp32 with IEEE
// division (__fdiv_rn; nothing here may be contracted or replaced by a
// reciprocal: the outputs are compared byte for byte).

#include "cmaps.h"
#include "common.h"
#include "mde_viz_abi.h"

namespace {

constexpr int kBlock = 256;
constexpr int kGridCap = 2048;  // blocks launched at most (8 per CU); they stride over the rest
constexpr int kCmaps = 3;
constexpr int kNanEntry = 256;  // table entry of a NaN: RGB (0, 0, 0)

const uint8_t kCmapHost[kCmaps][768] = {
    {MDE_CMAP_PLASMA_RGB}, {MDE_CMAP_VIRIDIS_RGB}, {MDE_CMAP_REDS_RGB}};
__constant__ uint8_t kCmapDev[kCmaps][768] = {
    {MDE_CMAP_PLASMA_RGB}, {MDE_CMAP_VIRIDIS_RGB}, {MDE_CMAP_REDS_RGB}};

// The grid (mde_viz_abi.h "Grid geometry"), all sizes < 2^31 and 3 P < 2^31.
struct Geo {
  int n, h, w;
  int xmaps;
  int ch, cw;    // cell pitch: h + padding, w + padding
  int padding;
  int Hg, Wg;
  int P;         // Hg * Wg
  int single;    // n == 1: the grid is the map
};

// Where grid pixel (gy, gx) comes from: the map k and the offset iy * w + ix
// inside it; k < 0 for a pad pixel.
struct Src {
  int k, off;
};

__device__ __forceinline__ Src locate(const Geo& G, int gy, int gx) {
  if (G.single) return Src{0, gy * G.w + gx};
  const int yy = gy - G.padding, xx = gx - G.padding;
  if (yy < 0 || xx < 0) return Src{-1, 0};
  const int r = yy / G.ch, c = xx / G.cw;
  const int iy = yy - r * G.ch, ix = xx - c * G.cw;
  const int k = r * G.xmaps + c;
  if (iy >= G.h || ix >= G.w || k >= G.n) return Src{-1, 0};
  return Src{k, iy * G.w + ix};
}

// colorize's table entry of one value (mde_viz_abi.h "colorize").
__device__ __forceinline__ int color_entry(float v, float vmin, float d, bool flat) {
  const float t = flat ? __fmul_rn(v, 0.f) : __fdiv_rn(__fsub_rn(v, vmin), d);
  const float xa = __fmul_rn(t, 256.f);
  if (xa != xa) return kNanEntry;
  if (xa == 256.f) return 255;
  if (xa < 0.f) return 0;
  if (xa >= 256.f) return 255;
  return (int)xa;
}

struct ColorArgs {
  const float* x;
  const float* xnorm;
  const float* y;
  const float* range;
  float vmin, vmax, pad_value;
  uint8_t* out[2];   // colorize(x'), colorize(|x' - y|); either may be null
  int shift[2][3];   // (address of plane c of out[o]) mod 4
  int cmap;
  int quads;         // threads' worth of work: quads per plane, partial ones included
  Geo G;
};

__global__ void __launch_bounds__(kBlock)
    viz_colorize_grid_kernel(ColorArgs A) {
  __shared__ uint32_t s_rgb[kNanEntry + 1];
  {
    const int i = threadIdx.x;  // kBlock == 256 entries
    const uint8_t* e = &kCmapDev[A.cmap][3 * i];
    s_rgb[i] = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
    if (i == 0) s_rgb[kNanEntry] = 0u;
  }
  __syncthreads();

  const Geo& G = A.G;
  float vmin = A.vmin, vmax = A.vmax;
  if (A.range) {
    vmin = A.range[0];
    vmax = A.range[1];
  }
  const bool flat = vmin == vmax;
  const float d = __fsub_rn(vmax, vmin);
  float mn = 0.f, den = 1.f;
  if (A.xnorm) {
    mn = A.xnorm[0];
    den = __fsub_rn(A.xnorm[1], mn);
  }
  const bool want_d = A.out[1] != nullptr;
  const int hw = G.h * G.w;

  for (int t = blockIdx.x * kBlock + threadIdx.x; t < A.quads; t += gridDim.x * kBlock) {
    uint32_t rgb[2][4];  // packed RGB of the quad's pixels, per output
    int cur = -1, q0 = 0;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      if (!A.out[o]) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int s = A.shift[o][c];
        if (s != cur) {
          cur = s;
          q0 = 4 * t - s;  // first pixel of this thread's quad in a plane of shift s
          const int qf = q0 < 0 ? 0 : q0;
          int gy = qf / G.Wg, gx = qf - gy * G.Wg;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int q = q0 + j;
            rgb[0][j] = rgb[1][j] = 0u;
            if (q < 0 || q >= G.P) continue;
            const Src p = locate(G, gy, gx);
            float v = A.pad_value, dv = A.pad_value;
            if (p.k >= 0) {
              const int i = p.k * hw + p.off;
              v = A.x[i];
              if (A.xnorm) v = __fdiv_rn(__fsub_rn(v, mn), den);
              if (want_d) dv = fabsf(__fsub_rn(v, A.y[i]));
            }
            rgb[0][j] = s_rgb[color_entry(v, vmin, d, flat)];
            if (want_d) rgb[1][j] = s_rgb[color_entry(dv, vmin, d, flat)];
            if (++gx == G.Wg) {
              gx = 0;
              ++gy;
            }
          }
        }
        uint8_t* plane = A.out[o] + (int64_t)c * G.P;
        const int sh = 8 * c;
        const uint32_t b0 = (rgb[o][0] >> sh) & 255u, b1 = (rgb[o][1] >> sh) & 255u;
        const uint32_t b2 = (rgb[o][2] >> sh) & 255u, b3 = (rgb[o][3] >> sh) & 255u;
        if (q0 >= 0 && q0 + 3 < G.P) {
          *reinterpret_cast<uint32_t*>(plane + q0) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        } else {  // the plane's first or last quad
          const uint32_t b[4] = {b0, b1, b2, b3};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (q0 + j >= 0 && q0 + j < G.P) plane[q0 + j] = (uint8_t)b[j];
        }
      }
    }
  }
}

struct ImageArgs {
  const float* x;
  const float* range;
  float* out;
  float pad_value;
  int c;
  int shift[3];  // (address of plane c of out, in floats) mod 4
  int quads;
  Geo G;
};

__global__ void __launch_bounds__(kBlock)
    viz_image_grid_kernel(ImageArgs A) {
  const Geo& G = A.G;
  const float lo = A.range[0], hi = A.range[1];
  const float den = fmaxf(__fsub_rn(hi, lo), 1e-5f);
  const int hw = G.h * G.w;
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < A.quads; t += gridDim.x * kBlock) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int q0 = 4 * t - A.shift[c];
      const int qf = q0 < 0 ? 0 : q0;
      int gy = qf / G.Wg, gx = qf - gy * G.Wg;
      const float* xc = A.x + (A.c == 3 ? c : 0) * hw;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = q0 + j;
        v[j] = A.pad_value;
        if (q < 0 || q >= G.P) continue;
        const Src p = locate(G, gy, gx);
        if (p.k >= 0) {
          float u = xc[p.k * A.c * hw + p.off];
          u = u < lo ? lo : u;  // clamp that keeps a NaN, as ATen's
          u = u > hi ? hi : u;
          v[j] = __fdiv_rn(__fsub_rn(u, lo), den);
        }
        if (++gx == G.Wg) {
          gx = 0;
          ++gy;
        }
      }
      float* plane = A.out + (int64_t)c * G.P;
      if (q0 >= 0 && q0 + 3 < G.P) {
        mde::st4(plane + q0, make_float4(v[0], v[1], v[2], v[3]));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (q0 + j >= 0 && q0 + j < G.P) plane[q0 + j] = v[j];
      }
    }
  }
}

// The grid of valid arguments; false for anything mde_viz_abi.h calls an
// argument error.  No product here can wrap: every factor is below 2^31 before
// it is multiplied, and a side is checked before the sides are.
bool geometry(int64_t n, int64_t h, int64_t w, int64_t nrow, int64_t padding, Geo* G) {
  const int64_t lim31 = (int64_t)1 << 31;
  if (n <= 0 || h <= 0 || w <= 0 || nrow < 1 || padding < 0 || n >= lim31 || h >= lim31 ||
      w >= lim31 || padding >= lim31)
    return false;
  int64_t Hg = h, Wg = w, xmaps = 1;
  if (n > 1) {
    xmaps = nrow < n ? nrow : n;
    const int64_t ymaps = mde::cdiv(n, xmaps);
    Hg = ymaps * (h + padding) + padding;  // < 2^31 * 2^32
    Wg = xmaps * (w + padding) + padding;
  }
  if (Hg >= lim31 || Wg >= lim31) return false;
  G->n = (int)n, G->h = (int)h, G->w = (int)w;
  G->xmaps = (int)xmaps;
  G->ch = (int)(n > 1 ? h + padding : h), G->cw = (int)(n > 1 ? w + padding : w);
  G->padding = (int)(n > 1 ? padding : 0);
  G->Hg = (int)Hg, G->Wg = (int)Wg;
  G->single = n == 1;
  const int64_t P = Hg * Wg;  // < 2^62
  G->P = P < lim31 ? (int)P : 0;
  return true;
}

// 3 Hg Wg < 2^31: what the kernels index with 32-bit integers.
bool fits(const Geo& G) {
  return (int64_t)G.Hg * G.Wg <= (((int64_t)1 << 31) - 1) / 3;
}

// Quads per plane so that every shift's first and last partial quad has a thread.
int quads_of(const Geo& G) { return (G.P + 2) / 4 + 1; }

unsigned grid_for(int quads) {
  const int64_t blocks = mde::cdiv(quads, kBlock);
  return (unsigned)(blocks < kGridCap ? blocks : kGridCap);
}

}  // namespace

extern "C" {

int mde_viz_grid_shape(int64_t n, int64_t h, int64_t w, int64_t nrow, int64_t padding,
                       int64_t* Hg, int64_t* Wg) {
  Geo G{};
  if (!Hg || !Wg || !geometry(n, h, w, nrow, padding, &G)) return MDE_ERR_INVALID_ARG;
  *Hg = G.Hg;
  *Wg = G.Wg;
  return MDE_OK;
}

int mde_viz_cmap_lut(int cmap, uint8_t* rgb768) {
  if (!rgb768 || cmap < 0 || cmap >= kCmaps) return MDE_ERR_INVALID_ARG;
  for (int i = 0; i < 768; ++i) rgb768[i] = kCmapHost[cmap][i];
  return MDE_OK;
}

int mde_viz_colorize_grid(const void* x, const void* xnorm, const void* y, const void* range,
                          float vmin, float vmax, void* out_x, void* out_diff,
                          int64_t n, int64_t h, int64_t w, int64_t nrow, int64_t padding,
                          float pad_value, int cmap, int dtype, void* stream) {
  ColorArgs A{};
  if (!x || (!out_x && !out_diff) || (out_diff && !y) || cmap < 0 || cmap >= kCmaps ||
      !geometry(n, h, w, nrow, padding, &A.G) || !fits(A.G))
    return MDE_ERR_INVALID_ARG;
  if (dtype != MDE_F32) return MDE_ERR_UNSUPPORTED;
  A.x = (const float*)x, A.xnorm = (const float*)xnorm, A.y = (const float*)y;
  A.range = (const float*)range;
  A.vmin = vmin, A.vmax = vmax, A.pad_value = pad_value;
  A.out[0] = (uint8_t*)out_x, A.out[1] = (uint8_t*)out_diff;
  for (int o = 0; o < 2; ++o)
    for (int c = 0; c < 3; ++c)
      A.shift[o][c] = (int)(((uintptr_t)A.out[o] + (uintptr_t)c * (uintptr_t)A.G.P) & 3u);
  A.cmap = cmap;
  A.quads = quads_of(A.G);
  const double maps = 4.0 * (double)n * (double)h * (double)w;
  const double grid = 3.0 * (double)A.G.P;
  const double bytes = maps * (out_diff ? 2 : 1) + grid * ((out_x ? 1 : 0) + (out_diff ? 1 : 0));
  MDE_LAUNCH(mde::K_DEPTHNORM, bytes, (hipStream_t)stream, viz_colorize_grid_kernel,
             dim3(grid_for(A.quads)), dim3(kBlock), 0, A);
  return MDE_OK;
}

int mde_viz_image_grid(const void* x, const void* range, void* out, int64_t n, int64_t c,
                       int64_t h, int64_t w, int64_t nrow, int64_t padding, float pad_value,
                       int dtype, void* stream) {
  ImageArgs A{};
  if (!x || !range || !out || (c != 1 && c != 3) || !geometry(n, h, w, nrow, padding, &A.G) ||
      !fits(A.G))
    return MDE_ERR_INVALID_ARG;
  if (dtype != MDE_F32) return MDE_ERR_UNSUPPORTED;
  A.x = (const float*)x, A.range = (const float*)range, A.out = (float*)out;
  A.pad_value = pad_value;
  A.c = (int)c;
  for (int p = 0; p < 3; ++p)
    A.shift[p] = (int)(((uintptr_t)out / sizeof(float) + (uintptr_t)p * (uintptr_t)A.G.P) & 3u);
  A.quads = quads_of(A.G);
  const double bytes = 4.0 * 3.0 * (double)n * (double)h * (double)w + 12.0 * (double)A.G.P;
  MDE_LAUNCH(mde::K_DEPTHNORM, bytes, (hipStream_t)stream, viz_image_grid_kernel,
             dim3(grid_for(A.quads)), dim3(kBlock), 0, A);
  return MDE_OK;
}

}  // extern "C"
