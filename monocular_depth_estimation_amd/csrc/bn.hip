// BatchNorm2d (NCHW, fp32) with fused conv bias, activation and residual.
//
// Replaces nn.BatchNorm2d (+ the conv bias in front of it, + the ReLU /
// residual add after it) at the 73 BN sites of GuideDepth:
// src/GuideDepth/model/modules.py:43-49,53-59,68-74 and
// src/GuideDepth/model/DDRNet_23_slim.py:46-72,80-113,118-172,201-210,
// 229-265,294-298.  MIOpen's spatial BN was 88 of 153 ms of a 640x480 bs=32
// train step (profiles/r01_*), ~10% of HBM bandwidth.
//
//   z = x + b[c]                     (b: the preceding conv's bias, nullable)
//   y = act(scale[c] * z + shift[c] (+ residual))
// Training: batch mean / biased variance of z over (N,H,W); running stats
// updated with momentum and the unbiased variance; num_batches_tracked += 1.
// Eval: running statistics.  Folding the conv bias here removes the conv's
// broadcast bias add and its (N,H,W) bias-gradient reduction: d/db = sum of
// this BN's input gradient, which falls out of the backward's own sums.
//
// Launches: forward  = stats (per-slice shifted sums) + apply;
//           backward = reduce (sum dy', sum dy'(x-mean)) + apply.
// The per-channel finalisation (double precision, fixed order) is recomputed
// by every apply block from the slice partials — no separate tiny kernel —
// and one designated block per channel writes the saved / running statistics
// and the parameter gradients.  dy' = dy * [act'] is recomputed from x (and
// the residual), so y is never kept for the backward.
#include <cmath>

#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "mde_wgrad_fold_abi.h"

namespace {

constexpr int kTarget = 2048;    // blocks to aim for per reduction launch
constexpr int kMinSlice = 4096;  // elements per slice at least
constexpr int kPlaneChunk4 = 1024;  // float4 per apply block in plane mode
constexpr int64_t kMaxApplyRecords = 256;  // producer records a plane-mode apply block merges itself

struct Geo {
  int64_t c, hw, total;  // total = n * hw elements per channel
  int slices;
  int64_t slice_len;     // multiple of 4 when hw % 4 == 0
};

// MDE_BN_TARGET / MDE_BN_MINSLICE override the two constants (tools/bn_bench.py sweeps)
int64_t env_or(const char* name, int64_t dflt) {
  const char* v = std::getenv(name);
  return v && *v ? std::atoll(v) : dflt;
}

Geo geometry(int64_t n, int64_t c, int64_t hw) {
  static const int64_t target = env_or("MDE_BN_TARGET", kTarget);
  static const int64_t min_slice = env_or("MDE_BN_MINSLICE", kMinSlice);
  Geo g;
  g.c = c;
  g.hw = hw;
  g.total = n * hw;
  int64_t s = mde::cdiv(target, c);
  const int64_t by_size = mde::cdiv(g.total, min_slice);
  if (s > by_size) s = by_size;
  if (s < 1) s = 1;
  if (s > 128) s = 128;
  g.slices = (int)s;
  int64_t len = mde::cdiv(g.total, s);
  if (hw % 4 == 0) len = mde::cdiv(len, 4) * 4;
  g.slice_len = len;
  return g;
}

// Apply kernels run "plane mode" (one channel per block, grid (chunks,
// planes)) for large planes and "channel-table mode" (all channels'
// coefficients in LDS, grid-stride) for small ones.
bool plane_mode(int64_t hw) { return hw % 4 == 0 && hw / 4 >= 256; }

// act: 0 none, 1 relu, 2 hardswish (v * clamp(v + 3, 0, 6) / 6, ATen's order)
__device__ __forceinline__ float act_fn(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f;
  return v;
}

using mde::bf16;
using mde::ld1;
using mde::ld4;
using mde::st1;
using mde::st4;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum of the two partial arrays of channel ch, by one full wave (lane-strided,
// then a fixed butterfly) -> identical result in every block.
__device__ __forceinline__ void wave_slices(const float* part, int64_t ch,
                                            int slices, double* a, double* b) {
  const int lane = threadIdx.x & 63;
  double x = 0.0, y = 0.0;
  for (int s = lane; s < slices; s += 64) {
    x += (double)part[(ch * slices + s) * 2];
    y += (double)part[(ch * slices + s) * 2 + 1];
  }
  *a = wave_sum_d(x);
  *b = wave_sum_d(y);
}

// Shifted sums of channel ch about `ref` from producer records (shift r, count
// n, s1, s2): s1 + n d and s2 + d (2 s1 + n d), d = r - ref, in double, a
// fixed lane-strided order and butterfly (deterministic); every lane gets them.
__device__ __forceinline__ void wave_records(const float* rec, int64_t ch, int nrec, double ref,
                                             double* a, double* b) {
  const int lane = threadIdx.x & 63;
  double x = 0.0, y = 0.0;
  for (int k = lane; k < nrec; k += 64) {
    const float4 q = *reinterpret_cast<const float4*>(rec + (ch * nrec + k) * 4);
    const double n = (double)q.y, d = (double)q.x - ref, b1 = (double)q.z;
    x += b1 + n * d;
    y += (double)q.w + d * (2.0 * b1 + n * d);
  }
  *a = wave_sum_d(x);
  *b = wave_sum_d(y);
}

// Per-channel forward constants.  mean_x is the mean of the RAW input x
// (without the folded bias); scale/shift act on raw x.
struct FwdCh {
  float sc, sh, mean_x, invstd;
};

struct FwdArgs {
  const float* gamma;
  const float* beta;
  const float* prebias;  // nullable
  const float* part;     // training: slice partials
  int slices;
  int64_t total;
  int64_t hw;
  float eps, momentum;
  float* rmean;          // nullable (no running-stat tracking)
  float* rvar;
  int64_t* nbt;          // nullable
  float* save_mean;
  float* save_invstd;
  int training;
  // producer-emitted per-block records [c][nrec][4] = (shift, count, s1, s2),
  // merged by the plane-mode apply itself (nullable: then `part`)
  const float* rec;
  int nrec;
};

// Training: (s1, s2) are the shifted sums of channel ch (shift = its first
// element); writes the designated outputs when `owner`.
template <typename T>
__device__ FwdCh fwd_channel(const FwdArgs& A, const T* x, int64_t ch,
                             double s1, double s2, bool owner) {
  FwdCh r;
  const float pb = A.prebias ? A.prebias[ch] : 0.f;
  double mean_x, invstd;
  if (A.training) {
    const double n = (double)A.total;
    const double ref = (double)ld1(x + ch * A.hw);
    const double dm = s1 / n;
    double var = s2 / n - dm * dm;
    if (var < 0.0) var = 0.0;
    mean_x = ref + dm;
    invstd = 1.0 / std::sqrt(var + (double)A.eps);
    if (owner && A.rmean) {
      const double unb = A.total > 1 ? var * n / (n - 1.0) : var;
      const double m = (double)A.momentum;
      A.rmean[ch] = (float)((1.0 - m) * (double)A.rmean[ch] + m * (mean_x + (double)pb));
      A.rvar[ch] = (float)((1.0 - m) * (double)A.rvar[ch] + m * unb);
    }
  } else {
    mean_x = (double)A.rmean[ch] - (double)pb;
    invstd = 1.0 / std::sqrt((double)A.rvar[ch] + (double)A.eps);
  }
  r.mean_x = (float)mean_x;
  r.invstd = (float)invstd;
  if (owner) {
    A.save_mean[ch] = r.mean_x;
    A.save_invstd[ch] = r.invstd;
    if (ch == 0 && A.training && A.nbt) A.nbt[0] += 1;
  }
  r.sc = A.gamma[ch] * r.invstd;
  r.sh = A.beta[ch] - r.mean_x * r.sc;
  return r;
}

// Walks a channel's (N, H*W) elements with a fixed stride without a 64-bit
// division per step: (image, offset in plane) advance by `step` elements.
struct PlaneCursor {
  int64_t off;  // element offset of (nn, p) relative to the channel base
  int64_t p;
  __device__ PlaneCursor(int64_t i, int64_t hw, int64_t chw) {
    const int64_t nn = i / hw;
    p = i - nn * hw;
    off = nn * chw + p;
  }
  __device__ __forceinline__ void advance(int64_t step, int64_t hw, int64_t chw) {
    p += step;
    off += step;
    while (p >= hw) {
      p -= hw;
      off += chw - hw;
    }
  }
};

// Nontemporal loads / stores only in the backward apply (the last reader of
// gy and x): the same hint on the statistics, forward apply and backward
// reduce measured slower (the apply re-reads what the reduce just streamed),
// profiles/r04_nt_ab.txt.
using mde::ld4_nt;
using mde::st4_nt;

constexpr int kRedDepth = 4;  // independent float4 loads per thread per trip

// part[(c * slices + s) * 2 + {0,1}] = sum(x - ref), sum((x - ref)^2)
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
    bn_stats_kernel(const T* __restrict__ x, int64_t c, int64_t hw,
                    int64_t total, int64_t slice_len, int slices,
                    float* __restrict__ part) {
  __shared__ float red[4];
  const int64_t ch = blockIdx.y;
  const int s = blockIdx.x;
  const int64_t i0 = s * slice_len;
  const int64_t i1 = i0 + slice_len < total ? i0 + slice_len : total;
  const T* xc = x + ch * hw;
  const float ref = ld1(xc);  // shift for the variance (cancellation guard)
  const int64_t chw = c * hw;
  float s1 = 0.f, s2 = 0.f;
  if (VEC) {
    constexpr int64_t kStep = 4 * 256;
    int64_t i = i0 + 4 * threadIdx.x;
    if (i < i1) {
      PlaneCursor cur(i, hw, chw);
      auto acc = [&](const float4 v) {
        const float a = v.x - ref, b = v.y - ref, cc = v.z - ref, d = v.w - ref;
        s1 += (a + b) + (cc + d);
        s2 += (a * a + b * b) + (cc * cc + d * d);
      };
      for (; i + (kRedDepth - 1) * kStep < i1; i += kRedDepth * kStep) {
        float4 v[kRedDepth];
#pragma unroll
        for (int k = 0; k < kRedDepth; ++k) {
          v[k] = ld4(xc + cur.off);
          cur.advance(kStep, hw, chw);
        }
#pragma unroll
        for (int k = 0; k < kRedDepth; ++k) acc(v[k]);
      }
      for (; i < i1; i += kStep) {
        acc(ld4(xc + cur.off));
        cur.advance(kStep, hw, chw);
      }
    }
  } else {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      const int64_t nn = i / hw, p = i - nn * hw;
      const float a = ld1(xc + nn * chw + p) - ref;
      s1 += a;
      s2 += a * a;
    }
  }
  const float t1 = mde::block_sum256(s1, red);
  const float t2 = mde::block_sum256(s2, red);
  if (threadIdx.x == 0) {
    float* o = part + (ch * slices + s) * 2;
    o[0] = t1;
    o[1] = t2;
  }
}

__device__ __forceinline__ float4 fwd4(float4 v, float4 q, bool has_r, float sc,
                                       float sh, int act) {
  v.x = v.x * sc + sh;
  v.y = v.y * sc + sh;
  v.z = v.z * sc + sh;
  v.w = v.w * sc + sh;
  if (has_r) {
    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
  }
  v.x = act_fn(v.x, act); v.y = act_fn(v.y, act);
  v.z = act_fn(v.z, act); v.w = act_fn(v.w, act);
  return v;
}

// Plane mode: grid (ceil(hw4 / 1024), n*c); 4 float4 per thread.
template <typename T>
__global__ void __launch_bounds__(256)
    bn_apply_plane_kernel(const T* __restrict__ x, const T* __restrict__ r,
                          T* __restrict__ y, int64_t c, int64_t hw, int act,
                          FwdArgs A) {
  __shared__ float cf[2];
  const int64_t plane = blockIdx.y;
  const int64_t ch = plane % c;
  const int64_t hw4 = hw >> 2;
  const T* xp = x + plane * hw;
  const T* rp = r ? r + plane * hw : nullptr;
  T* yp = y + plane * hw;
  const int64_t b0 = blockIdx.x * (int64_t)kPlaneChunk4;
  // data loads before the coefficient prologue (see bn_bwd_apply_plane_kernel)
  constexpr int KK = kPlaneChunk4 / 256;
  float4 x4[KK], q4[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    const int64_t i = b0 + k * 256 + threadIdx.x;
    const int64_t ic = i < hw4 ? i : hw4 - 1;
    x4[k] = ld4(xp + 4 * ic);
    q4[k] = rp ? ld4(rp + 4 * ic) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (threadIdx.x < 64) {
    double s1 = 0.0, s2 = 0.0;
    if (A.training) {
      if (A.rec)
        wave_records(A.rec, ch, A.nrec, (double)ld1(x + ch * hw), &s1, &s2);
      else
        wave_slices(A.part, ch, A.slices, &s1, &s2);
    }
    if (threadIdx.x == 0) {
      const bool owner = blockIdx.x == 0 && plane < c;
      const FwdCh k = fwd_channel(A, x, ch, s1, s2, owner);
      cf[0] = k.sc;
      cf[1] = k.sh;
    }
  }
  __syncthreads();
  const float sc = cf[0], sh = cf[1];
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    const int64_t i = b0 + k * 256 + threadIdx.x;
    if (i < hw4) st4(yp + 4 * i, fwd4(x4[k], q4[k], rp != nullptr, sc, sh, act));
  }
}

// Table kernels take the float4 path when every group of four elements lies
// in one plane and the element count fits 32-bit index math.
__host__ __device__ __forceinline__ bool table_vec(int64_t total, int64_t hw) {
  return (hw & 3) == 0 && total < ((int64_t)1 << 31);
}

// Channel-table mode for small planes: block b owns the contiguous planes
// [p0, p1) of its share, builds the coefficients of just the channels those
// planes hold in LDS (not all c: the per-block prologue was the kernel's
// cost at 1-300-pixel planes), then streams its planes.  The designated
// writer of channel ch is the block holding plane ch (image 0).
struct PlaneShare {
  int64_t p0, p1, nch;  // planes [p0, p1), distinct channels min(p1 - p0, c)
  __device__ PlaneShare(int64_t planes, int64_t c) {
    const int64_t per = (planes + gridDim.x - 1) / gridDim.x;
    p0 = blockIdx.x * per;
    p1 = p0 + per < planes ? p0 + per : planes;
    if (p0 > p1) p0 = p1;
    nch = p1 - p0 < c ? p1 - p0 : c;
  }
  __device__ __forceinline__ int64_t channel(int64_t k, int64_t c) const { return (p0 + k) % c; }
  __device__ __forceinline__ bool owner(int64_t ch) const { return ch >= p0 && ch < p1; }
};

template <typename T>
__global__ void __launch_bounds__(256)
    bn_apply_table_kernel(const T* __restrict__ x, const T* __restrict__ r,
                          T* __restrict__ y, int64_t planes, int64_t c,
                          int64_t hw, int act, FwdArgs A) {
  extern __shared__ float tab[];  // [2][c]
  const PlaneShare ps(planes, c);
  for (int64_t k = threadIdx.x; k < ps.nch; k += blockDim.x) {
    const int64_t ch = ps.channel(k, c);
    double s1 = 0.0, s2 = 0.0;
    if (A.training) {
      for (int s = 0; s < A.slices; ++s) {
        s1 += (double)A.part[(ch * A.slices + s) * 2];
        s2 += (double)A.part[(ch * A.slices + s) * 2 + 1];
      }
    }
    const FwdCh kc = fwd_channel(A, x, ch, s1, s2, ps.owner(ch));
    tab[ch] = kc.sc;
    tab[c + ch] = kc.sh;
  }
  __syncthreads();
  if (table_vec(planes * hw, hw)) {
    // Four consecutive elements share a plane: float4 traffic, 32-bit index math.
    const uint32_t hw4 = (uint32_t)(hw >> 2), cc = (uint32_t)c;
    const uint32_t t1 = (uint32_t)(ps.p1 * (hw >> 2));
    for (uint32_t t = (uint32_t)(ps.p0 * (hw >> 2)) + threadIdx.x; t < t1; t += blockDim.x) {
      const uint32_t ch = (t / hw4) % cc;
      const float4 q = r ? ld4(r + 4 * (int64_t)t) : make_float4(0.f, 0.f, 0.f, 0.f);
      st4(y + 4 * (int64_t)t,
          fwd4(ld4(x + 4 * (int64_t)t), q, r != nullptr, tab[ch], tab[c + ch], act));
    }
    return;
  }
  for (int64_t t = ps.p0 * hw + threadIdx.x; t < ps.p1 * hw; t += blockDim.x) {
    const int64_t ch = (t / hw) % c;
    float v = ld1(x + t) * tab[ch] + tab[c + ch];
    if (r) v += ld1(r + t);
    st1(y + t, act_fn(v, act));
  }
}

// dy' = dy * act'(pre-activation), the pre-activation recomputed exactly as
// the forward; hardswish' follows ATen (0 below -3, x/3 + 1/2 up to 3, 1 above).
__device__ __forceinline__ float dy_eff(float g, float xv, float rv, float sc,
                                        float sh, int act) {
  if (act == 0) return g;
  const float pre = xv * sc + sh + rv;
  if (act == 1) return pre > 0.f ? g : 0.f;
  return pre < -3.f ? 0.f : (pre <= 3.f ? g * (pre / 3.f + 0.5f) : g);
}

// part[(c*slices+s)*2] = sum dy', sum dy' * (x - mean_x)
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
    bn_bwd_reduce_kernel(const T* __restrict__ gy, const T* __restrict__ x,
                         const T* __restrict__ r,
                         const float* __restrict__ gamma, const float* __restrict__ beta,
                         const float* __restrict__ mean, const float* __restrict__ invstd,
                         int64_t c, int64_t hw, int64_t total, int64_t slice_len,
                         int slices, int act, float* __restrict__ part) {
  __shared__ float red[4];
  const int64_t ch = blockIdx.y;
  const int s = blockIdx.x;
  const int64_t i0 = s * slice_len;
  const int64_t i1 = i0 + slice_len < total ? i0 + slice_len : total;
  const float is = invstd[ch];
  const float sc = gamma[ch] * is, mu = mean[ch];
  const float sh = beta[ch] - mu * sc;
  const int64_t chw = c * hw;
  const int64_t base = ch * hw;
  float s1 = 0.f, s2 = 0.f;
  if (VEC) {
    constexpr int64_t kStep = 4 * 256;
    int64_t i = i0 + 4 * threadIdx.x;
    if (i < i1) {
      PlaneCursor cur(i, hw, chw);
      auto acc = [&](const float4 g, const float4 v, const float4 q) {
        const float a = dy_eff(g.x, v.x, q.x, sc, sh, act);
        const float b = dy_eff(g.y, v.y, q.y, sc, sh, act);
        const float cc = dy_eff(g.z, v.z, q.z, sc, sh, act);
        const float d = dy_eff(g.w, v.w, q.w, sc, sh, act);
        s1 += (a + b) + (cc + d);
        s2 += (a * (v.x - mu) + b * (v.y - mu)) + (cc * (v.z - mu) + d * (v.w - mu));
      };
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      for (; i + (kRedDepth - 1) * kStep < i1; i += kRedDepth * kStep) {
        float4 g[kRedDepth], v[kRedDepth], q[kRedDepth];
#pragma unroll
        for (int k = 0; k < kRedDepth; ++k) {
          const int64_t off = base + cur.off;
          g[k] = ld4(gy + off);
          v[k] = ld4(x + off);
          q[k] = r ? ld4(r + off) : z4;
          cur.advance(kStep, hw, chw);
        }
#pragma unroll
        for (int k = 0; k < kRedDepth; ++k) acc(g[k], v[k], q[k]);
      }
      for (; i < i1; i += kStep) {
        const int64_t off = base + cur.off;
        acc(ld4(gy + off), ld4(x + off), r ? ld4(r + off) : z4);
        cur.advance(kStep, hw, chw);
      }
    }
  } else {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      const int64_t nn = i / hw, p = i - nn * hw;
      const int64_t off = base + nn * chw + p;
      const float v = ld1(x + off);
      const float a = dy_eff(ld1(gy + off), v, r ? ld1(r + off) : 0.f, sc, sh, act);
      s1 += a;
      s2 += a * (v - mu);
    }
  }
  const float t1 = mde::block_sum256(s1, red);
  const float t2 = mde::block_sum256(s2, red);
  if (threadIdx.x == 0) {
    float* o = part + (ch * slices + s) * 2;
    o[0] = t1;
    o[1] = t2;
  }
}

struct BwdArgs {
  const float* gamma;
  const float* beta;
  const float* mean;    // raw-x mean saved by the forward
  const float* invstd;
  const float* part;
  int slices;
  int64_t total;
  int training;
  float* ggamma;        // nullable
  float* gbeta;         // nullable
  float* gprebias;      // nullable
};

struct BwdCh {
  float sc, sh, A, B, D;
};

// dx = A dy' + B x + D;  ggamma = invstd * sum dy'(x-mean);  gbeta = sum dy';
// d(prebias) = sum dx (0 up to rounding in training, A*sum dy' in eval).
__device__ BwdCh bwd_channel(const BwdArgs& P, int64_t ch, double sdy,
                             double sdyx, bool owner) {
  BwdCh r;
  const double is = (double)P.invstd[ch];
  const double mu = (double)P.mean[ch];
  const double scale = (double)P.gamma[ch] * is;
  double A = scale, B = 0.0, D = 0.0;
  const double n = (double)P.total;
  if (P.training) {
    B = -scale * is * is * sdyx / n;
    D = -scale * sdy / n - B * mu;
  }
  if (owner) {
    if (P.ggamma) P.ggamma[ch] = (float)(sdyx * is);
    if (P.gbeta) P.gbeta[ch] = (float)sdy;
    if (P.gprebias) P.gprebias[ch] = (float)(A * sdy + B * n * mu + D * n);
  }
  r.sc = P.gamma[ch] * P.invstd[ch];
  r.sh = P.beta[ch] - P.mean[ch] * r.sc;
  r.A = (float)A;
  r.B = (float)B;
  r.D = (float)D;
  return r;
}

// The apply pass's per-channel coefficients alone (slices == 1: the caller's
// sums): tab [5][c] = sc, sh, A, B, D, and the parameter gradients the apply
// kernels' owner blocks write -- for a consumer that evaluates dx = A dy' +
// B x + D itself (mde_pointwise_bwd_bn_deferred).
__global__ void __launch_bounds__(256)
    bn_bwd_coef_kernel(int64_t c, BwdArgs P, float* __restrict__ tab) {
  const int64_t ch = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (ch >= c) return;
  const BwdCh k = bwd_channel(P, ch, (double)P.part[2 * ch], (double)P.part[2 * ch + 1], true);
  tab[ch] = k.sc;
  tab[c + ch] = k.sh;
  tab[2 * c + ch] = k.A;
  tab[3 * c + ch] = k.B;
  tab[4 * c + ch] = k.D;
}

// bn_bwd_coef_kernel from the reduce launch's slice partials: one wave per
// channel sums them as bn_bwd_apply_plane_kernel's prologue does (wave_slices,
// then bwd_channel by lane 0), so tab and the parameter gradients are the
// values that kernel's blocks compute.
__global__ void __launch_bounds__(256)
    bn_bwd_slices_coef_kernel(int64_t c, BwdArgs P, float* __restrict__ tab) {
  const int64_t ch = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
  if (ch >= c) return;  // wave-uniform
  double a, b;
  wave_slices(P.part, ch, P.slices, &a, &b);
  if ((threadIdx.x & 63) != 0) return;
  const BwdCh k = bwd_channel(P, ch, a, b, true);
  tab[ch] = k.sc;
  tab[c + ch] = k.sh;
  tab[2 * c + ch] = k.A;
  tab[3 * c + ch] = k.B;
  tab[4 * c + ch] = k.D;
}

template <typename T>
__global__ void __launch_bounds__(256)
    bn_bwd_apply_plane_kernel(const T* __restrict__ gy, const T* __restrict__ x,
                              const T* __restrict__ r, T* __restrict__ gx,
                              T* __restrict__ gr, int64_t c, int64_t hw, int act,
                              BwdArgs P) {
  __shared__ float cf[5];
  const int64_t plane = blockIdx.y;
  const int64_t ch = plane % c;
  const int64_t hw4 = hw >> 2;
  const T* gp = gy + plane * hw;
  const T* xp = x + plane * hw;
  const T* rp = r ? r + plane * hw : nullptr;
  T* op = gx + plane * hw;
  T* orp = gr ? gr + plane * hw : nullptr;
  const int64_t b0 = blockIdx.x * (int64_t)kPlaneChunk4;
  // the block's data loads are issued BEFORE the coefficient prologue (slice
  // sums + double math + barrier) so that their latencies overlap; clamped
  // indices keep every load unconditional (out-of-range lanes store nothing)
  constexpr int KK = kPlaneChunk4 / 256;
  float4 g4[KK], v4[KK], q4[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    const int64_t i = b0 + k * 256 + threadIdx.x;
    const int64_t ic = i < hw4 ? i : hw4 - 1;
    g4[k] = ld4_nt(gp + 4 * ic);
    v4[k] = ld4_nt(xp + 4 * ic);
    q4[k] = rp ? ld4_nt(rp + 4 * ic) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (threadIdx.x < 64) {
    double a, b;
    wave_slices(P.part, ch, P.slices, &a, &b);
    if (threadIdx.x == 0) {
      const BwdCh k = bwd_channel(P, ch, a, b, blockIdx.x == 0 && plane < c);
      cf[0] = k.sc; cf[1] = k.sh; cf[2] = k.A; cf[3] = k.B; cf[4] = k.D;
    }
  }
  __syncthreads();
  const float sc = cf[0], sh = cf[1], A = cf[2], B = cf[3], D = cf[4];
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    const int64_t i = b0 + k * 256 + threadIdx.x;
    if (i < hw4) {
      const float4 g = g4[k], v = v4[k], q = q4[k];
      const float4 e = make_float4(dy_eff(g.x, v.x, q.x, sc, sh, act),
                                   dy_eff(g.y, v.y, q.y, sc, sh, act),
                                   dy_eff(g.z, v.z, q.z, sc, sh, act),
                                   dy_eff(g.w, v.w, q.w, sc, sh, act));
      st4_nt(op + 4 * i, make_float4(A * e.x + B * v.x + D, A * e.y + B * v.y + D,
                                     A * e.z + B * v.z + D, A * e.w + B * v.w + D));
      if (orp) st4_nt(orp + 4 * i, e);
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
    bn_bwd_apply_table_kernel(const T* __restrict__ gy, const T* __restrict__ x,
                              const T* __restrict__ r, T* __restrict__ gx,
                              T* __restrict__ gr, int64_t planes, int64_t c,
                              int64_t hw, int act, BwdArgs P) {
  extern __shared__ float tab[];  // [5][c]
  const PlaneShare ps(planes, c);  // as bn_apply_table_kernel
  for (int64_t kk = threadIdx.x; kk < ps.nch; kk += blockDim.x) {
    const int64_t ch = ps.channel(kk, c);
    double a = 0.0, b = 0.0;
    for (int s = 0; s < P.slices; ++s) {
      a += (double)P.part[(ch * P.slices + s) * 2];
      b += (double)P.part[(ch * P.slices + s) * 2 + 1];
    }
    const BwdCh k = bwd_channel(P, ch, a, b, ps.owner(ch));
    tab[ch] = k.sc;
    tab[c + ch] = k.sh;
    tab[2 * c + ch] = k.A;
    tab[3 * c + ch] = k.B;
    tab[4 * c + ch] = k.D;
  }
  __syncthreads();
  const int64_t total = planes * hw;
  if (table_vec(total, hw)) {
    const uint32_t hw4 = (uint32_t)(hw >> 2), cc = (uint32_t)c;
    const uint32_t t1 = (uint32_t)(ps.p1 * (hw >> 2));
    for (uint32_t t = (uint32_t)(ps.p0 * (hw >> 2)) + threadIdx.x; t < t1; t += blockDim.x) {
      const uint32_t ch = (t / hw4) % cc;
      const int64_t o = 4 * (int64_t)t;
      const float sc = tab[ch], sh = tab[c + ch];
      const float A = tab[2 * c + ch], B = tab[3 * c + ch], D = tab[4 * c + ch];
      const float4 v = ld4(x + o), g = ld4(gy + o);
      const float4 q = r ? ld4(r + o) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 e, o4;
      e.x = dy_eff(g.x, v.x, q.x, sc, sh, act);
      e.y = dy_eff(g.y, v.y, q.y, sc, sh, act);
      e.z = dy_eff(g.z, v.z, q.z, sc, sh, act);
      e.w = dy_eff(g.w, v.w, q.w, sc, sh, act);
      o4.x = A * e.x + B * v.x + D;
      o4.y = A * e.y + B * v.y + D;
      o4.z = A * e.z + B * v.z + D;
      o4.w = A * e.w + B * v.w + D;
      st4(gx + o, o4);
      if (gr) st4(gr + o, e);
    }
    return;
  }
  for (int64_t t = ps.p0 * hw + threadIdx.x; t < ps.p1 * hw; t += blockDim.x) {
    const int64_t ch = (t / hw) % c;
    const float v = ld1(x + t);
    const float e = dy_eff(ld1(gy + t), v, r ? ld1(r + t) : 0.f, tab[ch], tab[c + ch], act);
    st1(gx + t, tab[2 * c + ch] * e + tab[3 * c + ch] * v + tab[4 * c + ch]);
    if (gr) st1(gr + t, e);
  }
}

// ---------------------------------------------------------------- small tensors
// One block per channel with the whole channel (n * hw <= kChanMax elements)
// in registers: statistics, finalisation and apply in ONE launch that reads x
// once (forward), and reduce + apply in one launch reading gy / x once
// (backward) -- DDRNet's 15x20 / 8x10 / 4x5 / 2x3 / 1x1 planes at bs 32,
// where the two-launch stats (or reduce) + table-apply pair was launch- and
// latency-bound (~15 us a BN for a few MB).  Unit j of the channel is element
// j (or float4 j when hw % 4 == 0) of the (image, pixel) order; sums per
// thread in float over <= kChanUnits units, then in double across the block
// (fixed order): deterministic.
constexpr int kChanThreads = 512;
constexpr int kChanUnits = 8;  // float4 (or elements) per thread
constexpr int64_t kChanMax = (int64_t)kChanThreads * kChanUnits * 4;

// Which storage types take the one-launch kernels: 0 none, 1 fp32, 2 fp32 and
// bf16 (mde_bn_chan_mode; the environment's MDE_BN_CHAN sets the start value).
// Round 4 kept bf16 on the two-launch path after the cfg3 golden's loss error
// moved 0.6 -> 1.7 %: both paths compute the same statistics in another
// summation order (tests/test_gpu_bn.py: every output within one bf16 ulp of
// the other path's, parameter gradients / running statistics within 1e-5),
// and that golden (64 x 96, bs 2) is ill-conditioned -- DAPPM's 1x1
// BatchNorms over two values turn one bf16 ulp into percents; with the r05
// kernels both bf16 goldens pass on this path (64x96 loss 0.34 % vs the
// oracle's own 0.31 %, gpurun_out/r05b/bf16_chan.log).
int g_chan_mode = [] {
  const char* e = std::getenv("MDE_BN_CHAN");
  return e ? std::atoi(e) : 2;
}();

template <typename T>
inline bool chan_mode(int64_t n, int64_t hw) {
  const bool on = std::is_same_v<T, float> ? g_chan_mode >= 1 : g_chan_mode >= 2;
  return on && !plane_mode(hw) && n * hw <= (hw % 4 == 0 ? kChanMax : kChanMax / 4);
}

// block-wide double sums of (a, b), fixed order; result valid in every thread
__device__ __forceinline__ void chan_sum2(double* a, double* b, double (*red)[kChanThreads / 64]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double x = wave_sum_d(*a), y = wave_sum_d(*b);
  if (lane == 0) {
    red[0][wv] = x;
    red[1][wv] = y;
  }
  __syncthreads();
  x = 0.0;
  y = 0.0;
#pragma unroll
  for (int k = 0; k < kChanThreads / 64; ++k) {
    x += red[0][k];
    y += red[1][k];
  }
  *a = x;
  *b = y;
}

template <typename T, bool VEC>
struct ChanView {
  // unit j -> element offset from the channel base (x + ch * hw)
  int64_t chw;
  uint32_t hwu;  // units per plane
  __device__ __forceinline__ int64_t off(uint32_t j) const {
    const uint32_t nn = j / hwu, p = j - nn * hwu;
    return (int64_t)nn * chw + (VEC ? 4 * (int64_t)p : (int64_t)p);
  }
  __device__ __forceinline__ float4 load(const T* base, uint32_t j) const {
    if constexpr (VEC) return ld4(base + off(j));
    return make_float4(ld1(base + off(j)), 0.f, 0.f, 0.f);
  }
  __device__ __forceinline__ void store(T* base, uint32_t j, float4 v) const {
    if constexpr (VEC)
      st4(base + off(j), v);
    else
      st1(base + off(j), v.x);
  }
};

template <typename T, bool VEC>
__global__ void __launch_bounds__(kChanThreads)
    bn_fwd_chan_kernel(const T* __restrict__ x, const T* __restrict__ r, T* __restrict__ y,
                       int64_t c, int64_t n, int64_t hw, int act, FwdArgs A) {
  __shared__ double red[2][kChanThreads / 64];
  __shared__ float cf[2];
  const int64_t ch = blockIdx.x;
  const ChanView<T, VEC> cv{c * hw, (uint32_t)(VEC ? hw >> 2 : hw)};
  const uint32_t units = (uint32_t)n * cv.hwu;
  const T* xc = x + ch * hw;
  const T* rc = r ? r + ch * hw : nullptr;
  float4 v[kChanUnits], q[kChanUnits];
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < kChanUnits; ++k) {
    const uint32_t j = threadIdx.x + k * kChanThreads;
    const uint32_t jc = j < units ? j : units - 1;  // unconditional loads
    v[k] = cv.load(xc, jc);
    q[k] = rc ? cv.load(rc, jc) : z4;
  }
  const float ref = ld1(xc);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < kChanUnits; ++k) {
    if (threadIdx.x + k * kChanThreads < units) {
      const float a = v[k].x - ref;
      if constexpr (VEC) {
        const float b = v[k].y - ref, cc = v[k].z - ref, d = v[k].w - ref;
        s1 += (a + b) + (cc + d);
        s2 += (a * a + b * b) + (cc * cc + d * d);
      } else {
        s1 += a;
        s2 += a * a;
      }
    }
  }
  double d1 = s1, d2 = s2;
  chan_sum2(&d1, &d2, red);
  if (threadIdx.x == 0) {
    const FwdCh kc = fwd_channel(A, x, ch, d1, d2, true);
    cf[0] = kc.sc;
    cf[1] = kc.sh;
  }
  __syncthreads();
  const float sc = cf[0], sh = cf[1];
  T* yc = y + ch * hw;
#pragma unroll
  for (int k = 0; k < kChanUnits; ++k) {
    const uint32_t j = threadIdx.x + k * kChanThreads;
    if (j < units) cv.store(yc, j, fwd4(v[k], q[k], rc != nullptr, sc, sh, act));
  }
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(kChanThreads)
    bn_bwd_chan_kernel(const T* __restrict__ gy, const T* __restrict__ x,
                       const T* __restrict__ r, T* __restrict__ gx, T* __restrict__ gr,
                       int64_t c, int64_t n, int64_t hw, int act, BwdArgs P) {
  __shared__ double red[2][kChanThreads / 64];
  __shared__ float cf[3];
  const int64_t ch = blockIdx.x;
  const ChanView<T, VEC> cv{c * hw, (uint32_t)(VEC ? hw >> 2 : hw)};
  const uint32_t units = (uint32_t)n * cv.hwu;
  const int64_t cb = ch * hw;
  float4 g[kChanUnits], v[kChanUnits], q[kChanUnits];
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < kChanUnits; ++k) {
    const uint32_t j = threadIdx.x + k * kChanThreads;
    const uint32_t jc = j < units ? j : units - 1;
    g[k] = cv.load(gy + cb, jc);
    v[k] = cv.load(x + cb, jc);
    q[k] = r ? cv.load(r + cb, jc) : z4;
  }
  const float is = P.invstd[ch];
  const float sc = P.gamma[ch] * is, mu = P.mean[ch];
  const float sh = P.beta[ch] - mu * sc;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < kChanUnits; ++k) {
    // g[k] becomes dy' in place
    g[k].x = dy_eff(g[k].x, v[k].x, q[k].x, sc, sh, act);
    if constexpr (VEC) {
      g[k].y = dy_eff(g[k].y, v[k].y, q[k].y, sc, sh, act);
      g[k].z = dy_eff(g[k].z, v[k].z, q[k].z, sc, sh, act);
      g[k].w = dy_eff(g[k].w, v[k].w, q[k].w, sc, sh, act);
    }
    if (threadIdx.x + k * kChanThreads < units) {
      if constexpr (VEC) {
        s1 += (g[k].x + g[k].y) + (g[k].z + g[k].w);
        s2 += (g[k].x * (v[k].x - mu) + g[k].y * (v[k].y - mu)) +
              (g[k].z * (v[k].z - mu) + g[k].w * (v[k].w - mu));
      } else {
        s1 += g[k].x;
        s2 += g[k].x * (v[k].x - mu);
      }
    }
  }
  double d1 = s1, d2 = s2;
  chan_sum2(&d1, &d2, red);
  if (threadIdx.x == 0) {
    const BwdCh kc = bwd_channel(P, ch, d1, d2, true);
    cf[0] = kc.A;
    cf[1] = kc.B;
    cf[2] = kc.D;
  }
  __syncthreads();
  const float A = cf[0], B = cf[1], D = cf[2];
#pragma unroll
  for (int k = 0; k < kChanUnits; ++k) {
    const uint32_t j = threadIdx.x + k * kChanThreads;
    if (j < units) {
      const float4 e = g[k], xv = v[k];
      cv.store(gx + cb, j, make_float4(A * e.x + B * xv.x + D, A * e.y + B * xv.y + D,
                                       A * e.z + B * xv.z + D, A * e.w + B * xv.w + D));
      if (gr) cv.store(gr + cb, j, e);
    }
  }
}

inline int stream_grid(int64_t work) {
  const int64_t b = mde::cdiv(work, 256);
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// blocks of the table kernels: ~4 float4 per thread, at most one per plane
inline int table_grid(int64_t total, int64_t hw) {
  const int64_t planes = total / hw;
  const int64_t b = mde::cdiv(table_vec(total, hw) ? total >> 2 : total, 1024);
  const int64_t g = b < 1 ? 1 : (b > planes ? planes : b);
  return (int)(g > 4096 ? 4096 : g);
}

inline dim3 plane_grid(int64_t planes, int64_t hw) {
  return dim3((unsigned)mde::cdiv(hw / 4, kPlaneChunk4), (unsigned)planes);
}

bool args_ok(int64_t n, int64_t c, int64_t h, int64_t w) {
  return n > 0 && c > 0 && h > 0 && w > 0 && c <= 4096 && n * c <= 65535 &&
         n * h * w < ((int64_t)1 << 40);
}

template <typename T>
int launch_stats(const T* x, int64_t n, int64_t c, int64_t hw, const Geo& g, float* part,
                 hipStream_t s) {
  const double bytes = (double)sizeof(T) * n * c * (double)hw;
  if (hw % 4 == 0) {
    MDE_LAUNCH(mde::K_BN_STATS, bytes, s, (bn_stats_kernel<T, true>), dim3(g.slices, (unsigned)c),
               dim3(256), 0, x, c, hw, g.total, g.slice_len, g.slices, part);
  } else {
    MDE_LAUNCH(mde::K_BN_STATS, bytes, s, (bn_stats_kernel<T, false>), dim3(g.slices, (unsigned)c),
               dim3(256), 0, x, c, hw, g.total, g.slice_len, g.slices, part);
  }
  return MDE_OK;
}

// Producer-emitted statistics -> this file's partial format with ONE slice:
// part[ch * 2] = {sum (x - ref), sum (x - ref)^2}, ref = x[ch, 0] (the shift
// fwd_channel uses).  Block b's (shift r, count n, s1, s2) contributes
// s1 + n d and s2 + d (2 s1 + n d), d = r - ref -- plain double sums; the
// thread-strided order, the wave butterfly and the 4-wave order are fixed:
// deterministic.
// COEF: the same block then finalises its channel as bn_coef_kernel does (the
// merged sums rounded to float first, exactly the values bn_coef_kernel would
// read back from `part` with one slice): one launch instead of two.
template <typename T, bool COEF = false>
__global__ void __launch_bounds__(256)
    bn_stats_merge_kernel(const T* __restrict__ x, const float* __restrict__ stats, int G,
                          int64_t hw, float* __restrict__ part, FwdArgs A,
                          float* __restrict__ scale, float* __restrict__ shift) {
  __shared__ double red[2][4];
  const int64_t ch = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const double ref = (double)ld1(x + ch * hw);
  double s1 = 0.0, s2 = 0.0;
  auto acc = [&](const float* p) {
    const double n = (double)p[1], d = (double)p[0] - ref, b1 = (double)p[2];
    s1 += b1 + n * d;
    s2 += (double)p[3] + d * (2.0 * b1 + n * d);
  };
  int b = t;
  // four records in flight per lane (the loads of a latency-bound loop hoisted
  // ahead of the double chain); the per-lane summation order is unchanged
  for (; b + 3 * 256 < G; b += 4 * 256) {
    float q[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float* p = stats + (ch * G + b + k * 256) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) q[k][j] = p[j];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc(q[k]);
  }
  for (; b < G; b += 256) acc(stats + (ch * G + b) * 4);
  s1 = wave_sum_d(s1);
  s2 = wave_sum_d(s2);
  if (lane == 0) {
    red[0][wv] = s1;
    red[1][wv] = s2;
  }
  __syncthreads();
  if (t == 0) {
    const float p0 = (float)((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
    const float p1 = (float)((red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
    part[ch * 2] = p0;
    part[ch * 2 + 1] = p1;
    if constexpr (COEF) {
      const FwdCh k = fwd_channel(A, x, ch, (double)p0, (double)p1, true);
      scale[ch] = k.sc;
      shift[ch] = k.sh;
    }
  }
}

// Per-channel scale / shift only (the apply is fused into the consumer's
// operand load): one wave per channel, the same finalisation as the apply
// kernels, every wave the designated writer of its channel.
template <typename T>
__global__ void __launch_bounds__(256)
    bn_coef_kernel(const T* __restrict__ x, int64_t c, FwdArgs A,
                   float* __restrict__ scale, float* __restrict__ shift) {
  const int64_t ch = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ch >= c) return;  // whole waves
  double s1 = 0.0, s2 = 0.0;
  if (A.training) wave_slices(A.part, ch, A.slices, &s1, &s2);
  if ((threadIdx.x & 63) == 0) {
    const FwdCh k = fwd_channel(A, x, ch, s1, s2, true);
    scale[ch] = k.sc;
    shift[ch] = k.sh;
  }
}

template <typename T>
int launch_fwd_apply(const T* x, const T* r, T* y, int64_t n, int64_t c, int64_t hw, int act,
                     const FwdArgs& A, hipStream_t s) {
  const double bytes = (double)sizeof(T) * n * c * (double)hw * (r ? 3.0 : 2.0);
  if (plane_mode(hw)) {
    MDE_LAUNCH(mde::K_BN_APPLY, bytes, s, bn_apply_plane_kernel<T>, plane_grid(n * c, hw),
               dim3(256), 0, x, r, y, c, hw, act, A);
  } else {
    MDE_LAUNCH(mde::K_BN_APPLY_SMALL, bytes, s, bn_apply_table_kernel<T>,
               dim3(table_grid(n * c * hw, hw)), dim3(256), sizeof(float) * 2 * c, x, r, y, n * c, c,
               hw, act, A);
  }
  return MDE_OK;
}

template <typename T>
int fwd_train(const void* x, const void* residual, void* y, int64_t n, int64_t c, int64_t hw,
              int act, const Geo& g, const FwdArgs& A, hipStream_t s) {
  if (chan_mode<T>(n, hw)) {
    const double bytes = (double)sizeof(T) * n * c * (double)hw * (residual ? 3.0 : 2.0);
    if (hw % 4 == 0)
      MDE_LAUNCH(mde::K_BN_APPLY_SMALL, bytes, s, (bn_fwd_chan_kernel<T, true>), dim3((unsigned)c),
                 dim3(kChanThreads), 0, (const T*)x, (const T*)residual, (T*)y, c, n, hw, act, A);
    else
      MDE_LAUNCH(mde::K_BN_APPLY_SMALL, bytes, s, (bn_fwd_chan_kernel<T, false>), dim3((unsigned)c),
                 dim3(kChanThreads), 0, (const T*)x, (const T*)residual, (T*)y, c, n, hw, act, A);
    return MDE_OK;
  }
  const int st = launch_stats((const T*)x, n, c, hw, g, (float*)A.part, s);
  if (st) return st;
  return launch_fwd_apply((const T*)x, (const T*)residual, (T*)y, n, c, hw, act, A, s);
}

template <typename T>
int bwd_apply(const void* gy, const void* x, const void* residual, void* gx, void* gresidual,
              int64_t n, int64_t c, int64_t hw, int act, const BwdArgs& P, hipStream_t s) {
  const T* rr = act ? (const T*)residual : nullptr;
  const double big = (double)sizeof(T) * n * c * (double)hw;
  const double rb = rr ? big : 0.0;
  const double abytes = 3.0 * big + rb + (gresidual ? big : 0.0);
  if (plane_mode(hw)) {
    MDE_LAUNCH(mde::K_BN_BWD_APPLY, abytes, s, bn_bwd_apply_plane_kernel<T>,
               plane_grid(n * c, hw), dim3(256), 0, (const T*)gy, (const T*)x, rr, (T*)gx,
               (T*)gresidual, c, hw, act, P);
  } else {
    MDE_LAUNCH(mde::K_BN_BWD_APPLY_SMALL, abytes, s, bn_bwd_apply_table_kernel<T>,
               dim3(table_grid(n * c * hw, hw)), dim3(256), sizeof(float) * 5 * c, (const T*)gy,
               (const T*)x, rr, (T*)gx, (T*)gresidual, n * c, c, hw, act, P);
  }
  return MDE_OK;
}

// The backward's reduce launch: part [c][slices][2] = sum dy', sum dy' (x - mean)
template <typename T>
int bwd_reduce(const T* gy, const T* x, const T* rr, int64_t n, int64_t c, int64_t hw, int act,
               const Geo& g, float* part, const float* gamma, const float* beta,
               const float* mean, const float* invstd, hipStream_t s) {
  const double big = (double)sizeof(T) * n * c * (double)hw;
  const double rb = rr ? big : 0.0;
  if (hw % 4 == 0) {
    MDE_LAUNCH(mde::K_BN_BWD_REDUCE, 2.0 * big + rb, s, (bn_bwd_reduce_kernel<T, true>),
               dim3(g.slices, (unsigned)c), dim3(256), 0, gy, x, rr, gamma, beta, mean, invstd, c,
               hw, g.total, g.slice_len, g.slices, act, part);
  } else {
    MDE_LAUNCH(mde::K_BN_BWD_REDUCE, 2.0 * big + rb, s, (bn_bwd_reduce_kernel<T, false>),
               dim3(g.slices, (unsigned)c), dim3(256), 0, gy, x, rr, gamma, beta, mean, invstd, c,
               hw, g.total, g.slice_len, g.slices, act, part);
  }
  return MDE_OK;
}

template <typename T>
int bwd(const void* gy, const void* x, const void* residual, void* gx, void* gresidual,
        int64_t n, int64_t c, int64_t hw, int act, const Geo& g, const BwdArgs& P,
        const float* gamma, const float* beta, const float* mean, const float* invstd,
        hipStream_t s) {
  float* part = (float*)P.part;
  const T* rr = act ? (const T*)residual : nullptr;
  const double big = (double)sizeof(T) * n * c * (double)hw;
  const double rb = rr ? big : 0.0;
  if (chan_mode<T>(n, hw)) {
    const double abytes = 3.0 * big + rb + (gresidual ? big : 0.0);
    if (hw % 4 == 0)
      MDE_LAUNCH(mde::K_BN_BWD_APPLY_SMALL, abytes, s, (bn_bwd_chan_kernel<T, true>),
                 dim3((unsigned)c), dim3(kChanThreads), 0, (const T*)gy, (const T*)x, rr, (T*)gx,
                 (T*)gresidual, c, n, hw, act, P);
    else
      MDE_LAUNCH(mde::K_BN_BWD_APPLY_SMALL, abytes, s, (bn_bwd_chan_kernel<T, false>),
                 dim3((unsigned)c), dim3(kChanThreads), 0, (const T*)gy, (const T*)x, rr, (T*)gx,
                 (T*)gresidual, c, n, hw, act, P);
    return MDE_OK;
  }
  if (const int e = bwd_reduce<T>((const T*)gy, (const T*)x, rr, n, c, hw, act, g, part, gamma,
                                  beta, mean, invstd, s))
    return e;
  return bwd_apply<T>(gy, x, residual, gx, gresidual, n, c, hw, act, P, s);
}

bool dtype_ok(int dtype) { return dtype == MDE_F32 || dtype == MDE_BF16; }

}  // namespace

extern "C" {

int mde_batchnorm_stats_route(int64_t n, int64_t c, int64_t h, int64_t w, int64_t stats_blocks,
                              int dtype) {
  if (!dtype_ok(dtype) || !args_ok(n, c, h, w)) return -1;
  const int64_t hw = h * w;
  if (dtype == MDE_BF16 ? chan_mode<bf16>(n, hw) : chan_mode<float>(n, hw)) return 0;
  return plane_mode(hw) && stats_blocks > 0 && stats_blocks <= kMaxApplyRecords ? 1 : 2;
}

int mde_bn_chan_mode(int mode) {
  const int old = g_chan_mode;
  if (mode >= 0) g_chan_mode = mode > 2 ? 2 : mode;
  return old;
}

size_t mde_batchnorm_workspace(int64_t n, int64_t c, int64_t h, int64_t w) {
  const Geo g = geometry(n, c, h * w);
  return sizeof(float) * 2 * (size_t)c * g.slices;
}

int mde_batchnorm_fwd_train(const void* x, const float* gamma, const float* beta,
                            const float* prebias, float* running_mean,
                            float* running_var, int64_t* num_batches_tracked,
                            float momentum, float eps, const void* residual,
                            void* y, float* save_mean, float* save_invstd,
                            int64_t n, int64_t c, int64_t h, int64_t w, int act,
                            void* workspace, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return MDE_ERR_UNSUPPORTED;
  if (!x || !gamma || !beta || !y || !save_mean || !save_invstd || !workspace ||
      (!running_mean != !running_var) || act < 0 || act > 2 || !args_ok(n, c, h, w))
    return MDE_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t hw = h * w;
  const Geo g = geometry(n, c, hw);
  FwdArgs A{gamma, beta, prebias, (float*)workspace, g.slices, g.total, hw, eps, momentum,
            running_mean, running_var, num_batches_tracked, save_mean, save_invstd, 1};
  return dtype == MDE_BF16 ? fwd_train<bf16>(x, residual, y, n, c, hw, act, g, A, s)
                           : fwd_train<float>(x, residual, y, n, c, hw, act, g, A, s);
}

int mde_batchnorm_fwd_eval(const void* x, const float* gamma, const float* beta,
                           const float* prebias, const float* running_mean,
                           const float* running_var, float eps,
                           const void* residual, void* y, float* save_mean,
                           float* save_invstd, int64_t n, int64_t c, int64_t h,
                           int64_t w, int act, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return MDE_ERR_UNSUPPORTED;
  if (!x || !gamma || !beta || !running_mean || !running_var || !y ||
      !save_mean || !save_invstd || act < 0 || act > 2 || !args_ok(n, c, h, w))
    return MDE_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t hw = h * w;
  FwdArgs A{gamma, beta, prebias, nullptr, 0, n * hw, hw, eps, 0.f,
            (float*)running_mean, (float*)running_var, nullptr, save_mean,
            save_invstd, 0};
  if (dtype == MDE_BF16)
    return launch_fwd_apply((const bf16*)x, (const bf16*)residual, (bf16*)y, n, c, hw, act, A, s);
  return launch_fwd_apply((const float*)x, (const float*)residual, (float*)y, n, c, hw, act, A,
                          s);
}

int mde_batchnorm_fwd_coef(const void* x, const float* gamma, const float* beta,
                           const float* prebias, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, float momentum, float eps,
                           int training, float* scale, float* shift, float* save_mean,
                           float* save_invstd, int64_t n, int64_t c, int64_t h, int64_t w,
                           void* workspace, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return MDE_ERR_UNSUPPORTED;
  if (!x || !gamma || !beta || !scale || !shift || !save_mean || !save_invstd ||
      (!running_mean != !running_var) || !args_ok(n, c, h, w) ||
      (training && !workspace) || (!training && !running_mean))
    return MDE_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t hw = h * w;
  const Geo g = geometry(n, c, hw);
  float* part = (float*)workspace;
  if (training) {
    const int st = dtype == MDE_BF16 ? launch_stats((const bf16*)x, n, c, hw, g, part, s)
                                     : launch_stats((const float*)x, n, c, hw, g, part, s);
    if (st) return st;
  }
  FwdArgs A{gamma, beta, prebias, training ? part : nullptr, training ? g.slices : 0,
            g.total, hw, eps, momentum, running_mean, running_var,
            training ? num_batches_tracked : nullptr, save_mean, save_invstd, training ? 1 : 0};
  if (dtype == MDE_BF16)
    MDE_LAUNCH(mde::K_BN_FINAL, 8.0 * (double)c * (training ? g.slices : 1), s,
               bn_coef_kernel<bf16>, dim3((unsigned)mde::cdiv(c, 4)), dim3(256), 0,
               (const bf16*)x, c, A, scale, shift);
  else
    MDE_LAUNCH(mde::K_BN_FINAL, 8.0 * (double)c * (training ? g.slices : 1), s,
               bn_coef_kernel<float>, dim3((unsigned)mde::cdiv(c, 4)), dim3(256), 0,
               (const float*)x, c, A, scale, shift);
  return MDE_OK;
}

int mde_batchnorm_bwd(const void* gy, const void* x, const void* residual,
                      const float* gamma, const float* beta, const float* mean,
                      const float* invstd, int training, void* gx,
                      void* gresidual, float* ggamma, float* gbeta,
                      float* gprebias, int64_t n, int64_t c, int64_t h,
                      int64_t w, int act, void* workspace, int dtype,
                      void* stream) {
  if (!dtype_ok(dtype)) return MDE_ERR_UNSUPPORTED;
  if (!gy || !x || !gamma || !beta || !mean || !invstd || !gx || !workspace ||
      act < 0 || act > 2 || !args_ok(n, c, h, w) || (gresidual && !residual && act))
    return MDE_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t hw = h * w;
  const Geo g = geometry(n, c, hw);
  BwdArgs P{gamma, beta, mean, invstd, (float*)workspace, g.slices, g.total, training,
            ggamma, gbeta, gprebias};
  return dtype == MDE_BF16
             ? bwd<bf16>(gy, x, residual, gx, gresidual, n, c, hw, act, g, P, gamma, beta, mean,
                         invstd, s)
             : bwd<float>(gy, x, residual, gx, gresidual, n, c, hw, act, g, P, gamma, beta, mean,
                          invstd, s);
}

/* Training forward with the statistics emitted by the producing conv's
 * epilogue (mde_pointwise_fwd_stats / mde_conv3x3_fwd_stats): stats
 * [c][stats_blocks][4] = (shift, count, s1, s2) of the raw x; no statistics
 * pass over x.  Everything else as mde_batchnorm_fwd_train (fp32 or bf16 x;
 * statistics, coefficients and accumulation fp32). */
int mde_batchnorm_fwd_train_stats(const void* x, const float* gamma, const float* beta,
                                  const float* prebias, float* running_mean, float* running_var,
                                  int64_t* num_batches_tracked, float momentum, float eps,
                                  const void* residual, void* y, float* save_mean,
                                  float* save_invstd, int64_t n, int64_t c, int64_t h, int64_t w,
                                  int act, const float* stats, int64_t stats_blocks,
                                  void* workspace, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return MDE_ERR_UNSUPPORTED;
  if (!x || !gamma || !beta || !y || !save_mean || !save_invstd || !workspace || !stats ||
      stats_blocks <= 0 || stats_blocks > 0x7fffffff || (!running_mean != !running_var) ||
      act < 0 || act > 2 || !args_ok(n, c, h, w))
    return MDE_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t hw = h * w;
  // small tensors: the one-launch kernel (statistics + apply reading x once)
  // beats a merge launch + apply; the emitted records go unused
  if (dtype == MDE_BF16 ? chan_mode<bf16>(n, hw) : chan_mode<float>(n, hw))
    return mde_batchnorm_fwd_train(x, gamma, beta, prebias, running_mean, running_var,
                                   num_batches_tracked, momentum, eps, residual, y, save_mean,
                                   save_invstd, n, c, h, w, act, workspace, dtype, stream);
  float* part = (float*)workspace;
  if (plane_mode(hw) && stats_blocks <= kMaxApplyRecords) {
    // few records a channel: the plane-mode apply merges them in its prologue
    // (no merge launch)
    FwdArgs A{gamma, beta, prebias, part, 0, n * hw, hw, eps, momentum, running_mean,
              running_var, num_batches_tracked, save_mean, save_invstd, 1, stats,
              (int)stats_blocks};
    if (dtype == MDE_BF16)
      return launch_fwd_apply((const bf16*)x, (const bf16*)residual, (bf16*)y, n, c, hw, act, A, s);
    return launch_fwd_apply((const float*)x, (const float*)residual, (float*)y, n, c, hw, act, A, s);
  }
  const double mb = 16.0 * (double)c * stats_blocks;
  if (dtype == MDE_BF16)
    MDE_LAUNCH(mde::K_BN_FINAL, mb, s, (bn_stats_merge_kernel<bf16, false>), dim3((unsigned)c),
               dim3(256), 0, (const bf16*)x, stats, (int)stats_blocks, hw, part, FwdArgs{},
               nullptr, nullptr);
  else
    MDE_LAUNCH(mde::K_BN_FINAL, mb, s, (bn_stats_merge_kernel<float, false>), dim3((unsigned)c),
               dim3(256), 0, (const float*)x, stats, (int)stats_blocks, hw, part, FwdArgs{},
               nullptr, nullptr);
  FwdArgs A{gamma, beta, prebias, part, 1, n * hw, hw, eps, momentum,
            running_mean, running_var, num_batches_tracked, save_mean, save_invstd, 1};
  if (dtype == MDE_BF16)
    return launch_fwd_apply((const bf16*)x, (const bf16*)residual, (bf16*)y, n, c, hw, act, A, s);
  return launch_fwd_apply((const float*)x, (const float*)residual, (float*)y, n, c, hw, act, A, s);
}

/* mde_batchnorm_fwd_coef (training) with producer-emitted statistics. */
int mde_batchnorm_fwd_coef_stats(const void* x, const float* gamma, const float* beta,
                                 const float* prebias, float* running_mean, float* running_var,
                                 int64_t* num_batches_tracked, float momentum, float eps,
                                 float* scale, float* shift, float* save_mean, float* save_invstd,
                                 int64_t n, int64_t c, int64_t h, int64_t w, const float* stats,
                                 int64_t stats_blocks, void* workspace, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return MDE_ERR_UNSUPPORTED;
  if (!x || !gamma || !beta || !scale || !shift || !save_mean || !save_invstd || !workspace ||
      !stats || stats_blocks <= 0 || stats_blocks > 0x7fffffff ||
      (!running_mean != !running_var) || !args_ok(n, c, h, w))
    return MDE_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t hw = h * w;
  float* part = (float*)workspace;
  const double mb = 16.0 * (double)c * stats_blocks;
  FwdArgs A{gamma, beta, prebias, part, 1, n * hw, hw, eps, momentum, running_mean, running_var,
            num_batches_tracked, save_mean, save_invstd, 1};
  // merge + finalisation in one launch (bn_stats_merge_kernel<T, true>)
  if (dtype == MDE_BF16) {
    MDE_LAUNCH(mde::K_BN_FINAL, mb + 8.0 * (double)c, s, (bn_stats_merge_kernel<bf16, true>),
               dim3((unsigned)c), dim3(256), 0, (const bf16*)x, stats, (int)stats_blocks, hw,
               part, A, scale, shift);
  } else {
    MDE_LAUNCH(mde::K_BN_FINAL, mb + 8.0 * (double)c, s, (bn_stats_merge_kernel<float, true>),
               dim3((unsigned)c), dim3(256), 0, (const float*)x, stats, (int)stats_blocks, hw,
               part, A, scale, shift);
  }
  return MDE_OK;
}

/* The apply pass alone, with the reduce's sums supplied by the caller (e.g.
 * mde_pointwise_bwd_bn's in_sums): sums [c][2] = sum dy', sum dy' (x - mean). */
int mde_batchnorm_bwd_apply(const void* gy, const void* x, const void* residual,
                            const float* gamma, const float* beta, const float* mean,
                            const float* invstd, int training, const float* sums, void* gx,
                            void* gresidual, float* ggamma, float* gbeta, float* gprebias,
                            int64_t n, int64_t c, int64_t h, int64_t w, int act, int dtype,
                            void* stream) {
  if (!dtype_ok(dtype)) return MDE_ERR_UNSUPPORTED;
  if (!gy || !x || !gamma || !beta || !mean || !invstd || !sums || !gx || act < 0 || act > 2 ||
      !args_ok(n, c, h, w) || (gresidual && !residual && act))
    return MDE_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t hw = h * w;
  BwdArgs P{gamma, beta, mean, invstd, sums, 1, n * hw, training, ggamma, gbeta, gprebias};
  return dtype == MDE_BF16
             ? bwd_apply<bf16>(gy, x, residual, gx, gresidual, n, c, hw, act, P, s)
             : bwd_apply<float>(gy, x, residual, gx, gresidual, n, c, hw, act, P, s);
}

/* mde_batchnorm_bwd_apply's per-channel part without the apply pass: tab
 * [5][c] = scale, shift, A, B, D (dx = A dy' + B x + D) from the caller's
 * sums [c][2], and ggamma / gbeta / gprebias.  One launch, double math. */
int mde_batchnorm_bwd_coef(const float* gamma, const float* beta, const float* mean,
                           const float* invstd, int training, const float* sums, float* tab,
                           float* ggamma, float* gbeta, float* gprebias, int64_t n, int64_t c,
                           int64_t h, int64_t w, void* stream) {
  if (!gamma || !beta || !mean || !invstd || !sums || !tab || !args_ok(n, c, h, w))
    return MDE_ERR_INVALID_ARG;
  BwdArgs P{gamma, beta, mean, invstd, sums, 1, n * h * w, training, ggamma, gbeta, gprebias};
  MDE_LAUNCH(mde::K_BN_BWD_FINAL, 4.0 * 14.0 * (double)c, (hipStream_t)stream, bn_bwd_coef_kernel,
             dim3((unsigned)mde::cdiv(c, 256)), dim3(256), 0, c, P, tab);
  return MDE_OK;
}

/* include/mde_wgrad_fold_abi.h: mde_batchnorm_bwd's reduce launch, then the
 * coefficients and parameter gradients its apply pass would have computed. */
int mde_batchnorm_bwd_reduce_coef(const void* gy, const void* x, const float* gamma,
                                  const float* beta, const float* mean, const float* invstd,
                                  int training, float* tab, float* ggamma, float* gbeta,
                                  float* gprebias, int64_t n, int64_t c, int64_t h, int64_t w,
                                  int act, void* workspace, int dtype, void* stream) {
  if (dtype != MDE_F32) return MDE_ERR_UNSUPPORTED;
  if (!gy || !x || !gamma || !beta || !mean || !invstd || !tab || !workspace || act < 0 ||
      act > 2 || !args_ok(n, c, h, w))
    return MDE_ERR_INVALID_ARG;
  const int64_t hw = h * w;
  if (!plane_mode(hw)) return MDE_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const Geo g = geometry(n, c, hw);
  float* part = (float*)workspace;
  if (const int e = bwd_reduce<float>((const float*)gy, (const float*)x, nullptr, n, c, hw, act, g,
                                      part, gamma, beta, mean, invstd, s))
    return e;
  BwdArgs P{gamma, beta, mean, invstd, part, g.slices, g.total, training, ggamma, gbeta, gprebias};
  MDE_LAUNCH(mde::K_BN_BWD_FINAL, 4.0 * (2.0 * g.slices + 12.0) * (double)c, s,
             bn_bwd_slices_coef_kernel, dim3((unsigned)mde::cdiv(c, 4)), dim3(256), 0, c, P, tab);
  return MDE_OK;
}

}  // extern "C"
