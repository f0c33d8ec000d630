/*
 * mde_fold_abi.h — the full-resolution fold entries of libmde_hip.so.
 *
 * A further header beside mde_abi.h (see mde_eval_abi.h for the pattern):
 * mde_abi.h stays the frozen training ABI; this header adds to it and changes
 * nothing in it.  The symbols live in the same library and follow the same
 * conventions (mde_abi.h "Conventions"): plain DEVICE pointers owned by the
 * caller, `dtype` selects the element type (MDE_F32 only here, anything else
 * returns MDE_ERR_UNSUPPORTED), `stream` is a hipStream_t and the last
 * argument, scratch is sized by the matching *_workspace() query of mde_abi.h,
 * 0 on success / positive hipError_t / negative MDE_ERR_*, and nothing is
 * launched when an argument error is returned.  The Python mirror is
 * _abi.FOLD_SIGNATURES.
 *
 * The entries serve GuideDepth's decoder block at full resolution (up_3,
 * 16 channels at the input size).  Its 16 -> 1 `reduce` conv has the skip
 * gradient gs[n][c][p] = W[c] * g[n][0][p]: an outer product of the one-channel
 * loss gradient with 16 scalars.  mde_skip_reduce_bn_bwd stores it only so
 * that two later kernels read it back; here it is never written, and each
 * reader forms the product itself -- one fp32 multiply, rounded on its own,
 * exactly the value that was stored -- so every result is bit for bit the one
 * the mde_abi.h entries give.
 */
#ifndef MDE_FOLD_ABI_H
#define MDE_FOLD_ABI_H

#include "mde_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * mde_skip_reduce_bn_bwd without its `gs` output: cin == 16, cout == 1,
 * h * w % 4 == 0, in_sums required (else MDE_ERR_UNSUPPORTED).  gw [1][16],
 * gb [1] and in_sums [16][2] equal mde_skip_reduce_bn_bwd's bit for bit; the
 * workspace is mde_skip_reduce_bn_workspace's.
 * ------------------------------------------------------------------------- */
int mde_skip_reduce_bn_bwd_nogs(const void* gout, const void* r, const void* d,
                                const float* in_scale, const float* in_shift,
                                const float* in_mean, const float* wt, float* gw, float* gb,
                                float* in_sums, int64_t n, int64_t cin, int64_t cout, int64_t h,
                                int64_t w, void* workspace, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * mde_pointwise_bwd_bn_deferred in its BatchNorm mode (se_s == se_dm == NULL)
 * whose upstream gradient is g[n][o][p] = w1[o] * g1[n][p]:
 *   g1 [n, 1, h, w] fp32, w1 [cout] fp32; y_out, tab [5][cout], x, in_*, wt,
 *   gx, gw, in_sums and workspace as in mde_pointwise_bwd_bn_deferred.
 * cin == cout == 16 and h * w % 64 == 0, else MDE_ERR_UNSUPPORTED.  gx, gw and
 * in_sums equal those of mde_pointwise_bwd_bn_deferred fed the materialised
 * product, bit for bit.
 * ------------------------------------------------------------------------- */
int mde_pointwise_bwd_bn_rank1(const void* g1, const float* w1, const void* y_out,
                               const float* tab, const void* x, const float* in_scale,
                               const float* in_shift, const float* in_mean, const float* wt,
                               void* gx, float* gw, float* in_sums, int64_t n, int64_t cin,
                               int64_t cout, int64_t h, int64_t w, void* workspace, int dtype,
                               void* stream);

/* ---------------------------------------------------------------------------
 * mde_bilinear_bwd2 whose second gradient is gy2[n][ch][.] = w1[ch] * g1[n][.]:
 *   gy [n, c, ho, wo], g1 [n, 1, ho, wo], w1 [c], gx [n, c, hi, wi], fp32.
 * The shapes mde_bilinear_bwd2_supported accepts, else MDE_ERR_UNSUPPORTED.
 * gx equals mde_bilinear_bwd2's on the materialised product, bit for bit.
 * ------------------------------------------------------------------------- */
int mde_bilinear_bwd2_rank1(const void* gy, const void* g1, const float* w1, void* gx, int64_t n,
                            int64_t c, int64_t hi, int64_t wi, int64_t ho, int64_t wo,
                            float scale_h, float scale_w, int align_corners, int dtype,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDE_FOLD_ABI_H */
