/*
 * mde_wgrad_fold_abi.h — the guide convs' weight-gradient fold entries of
 * libmde_hip.so.
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
 * _abi.WGRAD_FOLD_SIGNATURES.
 *
 * The entries serve the guide branch of GuideDepth's guided-upsampling block:
 * 3x3 conv (3 -> E) -> BatchNorm + ReLU -> 1x1 conv.  The 3x3 conv reads the
 * image, which needs no gradient, so d/dy (y: the 3x3 conv's output) has one
 * reader, the conv's weight gradient.  mde_batchnorm_bwd_apply writes d/dy only
 * to hand it to that reader; here it is never written: the weight gradient
 * reads the gradient g upstream of the BatchNorm + ReLU and y, and evaluates
 *   d/dy = A [y sc + sh > 0] g + B y + D
 * on its operand load, in the fp32 operations of the apply kernel, so every
 * result is bit for bit the one the mde_abi.h entries give.
 */
#ifndef MDE_WGRAD_FOLD_ABI_H
#define MDE_WGRAD_FOLD_ABI_H

#include "mde_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * 1 iff mde_conv3x3_wgrad_bn_deferred takes the shape: cin == 3, cout in
 * {16, 32, 64}, h * w % 4 == 0 and h * w >= 1024 (the planes on which
 * mde_batchnorm_bwd_apply runs the kernel whose rounding is reproduced), and
 * mde_conv3x3_wgrad's 32-bit offset limits (64 * h * w < 2^31).
 * ------------------------------------------------------------------------- */
int mde_conv3x3_wgrad_bn_deferred_supported(int64_t n, int64_t cin, int64_t cout, int64_t h,
                                            int64_t w);

/* ---------------------------------------------------------------------------
 * mde_conv3x3_wgrad(gy, x, ...) with gy = mde_batchnorm_bwd_apply(g, y, act =
 * relu, no residual) formed on load:
 *   g, y [n, cout, h, w] fp32 (upstream gradient, the conv's output);
 *   tab [5][cout] = scale, shift, A, B, D (mde_batchnorm_bwd_coef or
 *   mde_batchnorm_bwd_reduce_coef); x [n, cin, h, w]; gweight [cout, cin, 3, 3];
 *   workspace: mde_conv3x3_wgrad_workspace(n, cin, cout, h, w, MDE_F32) bytes.
 * Shapes the query refuses return MDE_ERR_UNSUPPORTED.  gweight equals the
 * pair's bit for bit.
 * ------------------------------------------------------------------------- */
int mde_conv3x3_wgrad_bn_deferred(const void* g, const void* y, const float* tab, const void* x,
                                  float* gweight, int64_t n, int64_t cin, int64_t cout, int64_t h,
                                  int64_t w, void* workspace, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * mde_batchnorm_bwd (no residual) without its apply pass: the same reduce
 * launch over (gy, x), then one launch that sums the slices as the apply
 * kernel's prologue does and writes tab [5][c] = scale, shift, A, B, D and
 * ggamma / gbeta / gprebias (each nullable), equal to mde_batchnorm_bwd's bit
 * for bit.  h * w % 4 == 0 and h * w >= 1024 (mde_batchnorm_bwd's apply is
 * then the plane kernel), else MDE_ERR_UNSUPPORTED.  act as mde_batchnorm_bwd;
 * workspace: mde_batchnorm_workspace(n, c, h, w) bytes.
 * ------------------------------------------------------------------------- */
int mde_batchnorm_bwd_reduce_coef(const void* gy, const void* x, const float* gamma,
                                  const float* beta, const float* mean, const float* invstd,
                                  int training, float* tab, float* ggamma, float* gbeta,
                                  float* gprebias, int64_t n, int64_t c, int64_t h, int64_t w,
                                  int act, void* workspace, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDE_WGRAD_FOLD_ABI_H */
