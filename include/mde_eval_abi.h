/*
 * mde_eval_abi.h — the evaluation entries of libmde_hip.so.
 *
 * A second header beside mde_abi.h, for the entries that serve evaluation of a
 * trained GuideDepth checkpoint (src/GuideDepth/evaluate.py) rather than the
 * training hot path.  mde_abi.h stays the frozen training ABI; this header adds
 * to it and changes nothing in it.  The symbols live in the same library and
 * follow the same conventions (mde_abi.h "Conventions"): plain DEVICE pointers
 * owned by the caller, `dtype` selects the element type (MDE_F32 only here,
 * anything else returns MDE_ERR_UNSUPPORTED), `stream` is a hipStream_t and the
 * last argument, scratch is sized by the matching *_workspace() query, 0 on
 * success / positive hipError_t / negative MDE_ERR_*, and nothing is launched
 * when an argument error is returned.  The Python mirror is
 * _abi.EVAL_SIGNATURES.
 */
#ifndef MDE_EVAL_ABI_H
#define MDE_EVAL_ABI_H

#include "mde_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * Evaluation tail of both views of a test image in one pass.  Replaces, in
 * Evaluater.evaluate (src/GuideDepth/evaluate.py:93-142, the same loop in
 * src/GuideDepth/inference.py:208-280): torch.flip of gt (:94),
 * inverse_depth_norm of both predictions (:105,108,174-177), the bilinear
 * upscale to the ground-truth resolution (:113-116), the four crop slices
 * (:129-132) and the two Result.evaluate calls (:137,141;
 * src/GuideDepth/metrics.py:41-62).
 *   inv_pred, inv_pred_flip [n, ph, pw] fp32: the network's raw output for the
 *     image and for the horizontally flipped image (a [n,1,ph,pw] map is the
 *     same memory).  inv_pred_flip may be NULL: view 1's sums are then zeros.
 *   gt [n, H, W] fp32, metres.
 *   D(v) = clamp(max_depth / v, max_depth / 100, max_depth) with torch.clamp's
 *     semantics (v = 0 -> max_depth, v < 0 -> max_depth / 100, NaN stays NaN),
 *     applied to the four source samples BEFORE the interpolation.  The
 *     quotient is rounded as torch rounds `maxDepth / depth` for a Python
 *     number over a tensor (Tensor.__rtruediv__): fl(fl(1 / v) * max_depth).
 *   bilinear: align_corners=False, scales ph / H and pw / W in fp32
 *     (F.interpolate(size=...)); ph == H and pw == W gives the sample itself.
 *   view 0: pixel (y, j) compares bilinear(D(inv_pred_i))(y, j) with gt_i(y, j).
 *   view 1: pixel (y, x) of the flipped frame compares
 *     bilinear(D(inv_pred_flip_i))(y, x) with gt_i(y, W-1-x).
 *   crop: HOST int32[4], rows [crop[0], crop[1]) x cols [crop[2], crop[3]) of
 *     each frame's own coordinates are counted; NULL counts every pixel.
 *     0 <= crop[0] <= crop[1] <= H and 0 <= crop[2] <= crop[3] <= W, else
 *     MDE_ERR_INVALID_ARG.  An empty window gives zeros.
 *   sums: DEVICE double [n, 2, 16], per image and view the 16 sums of
 *     mde_eval_sums (mde_abi.h) in its layout: fp32 per-pixel terms,
 *     double accumulation.  Fixed reduction order, no atomics: deterministic,
 *     and image i's 32 numbers depend on image i's data only (not on n or i).
 *   n * H, n * ph < 2^31; W, pw < 2^30.
 * ------------------------------------------------------------------------- */
size_t mde_eval_pair_workspace(int64_t n, int64_t H, int64_t W);
int mde_eval_pair_sums(const void* inv_pred, const void* inv_pred_flip, const void* gt,
                       int64_t n, int64_t ph, int64_t pw, int64_t H, int64_t W,
                       float max_depth, const int32_t* crop, void* workspace, double* sums,
                       int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDE_EVAL_ABI_H */
