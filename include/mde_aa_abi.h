/*
 * mde_aa_abi.h — the antialiased bilinear resize of libmde_hip.so.
 *
 * A fourth header beside mde_abi.h (the frozen training ABI), mde_eval_abi.h
 * (the evaluation tail) and mde_infer_abi.h (the two ends of the deployed
 * path), each of which is pinned to its entries.  It adds to them and changes
 * nothing in them.  The symbols live in the same library and follow the same
 * conventions (mde_abi.h "Conventions"): plain DEVICE pointers owned by the
 * caller for the launching entries, `dtype` selects the element type, `stream`
 * is a hipStream_t and the last argument, 0 on success / positive hipError_t /
 * negative MDE_ERR_*, and nothing is launched when an argument error is
 * returned.  No entry needs scratch.  The launching entries are one kernel
 * launch with no host synchronisation and no allocation, so both may be
 * captured into a hipGraph.  The Python mirror is _abi.AA_SIGNATURES.
 *
 * The filter is F.interpolate(mode='bilinear', antialias=True,
 * align_corners=False) of torch, which torchvision >= 0.17's transforms.Resize
 * applies to float tensors by default (src/GuideDepth/evaluate.py:68,97-98,
 * src/GuideDepth/inference.py:121,226-227).  Separable, a triangle per axis,
 * every step in fp32.  For an axis with `in` source and `out` destination
 * samples: scale = (float)in / (float)out, support = max(scale, 1), invscale =
 * scale >= 1 ? 1 / scale : 1; for output index i:
 *   center = scale * (i + 0.5f)
 *   xmin   = max((int)(center - support + 0.5f), 0)
 *   xsize  = min((int)(center + support + 0.5f), in) - xmin
 *   w_j    = max(0, 1 - |(j + xmin - center + 0.5f) * invscale|),  j < xsize,
 *   each divided by the sequential sum of all of them,
 * every product, sum and quotient rounded to fp32 on its own.  Horizontal pass
 * first, fp32 intermediate, then the vertical pass; within a pass the taps are
 * summed sequentially from j = 0: fl(t_0 w_0), then acc = fma(t_j, w_j, acc),
 * as ATen's AVX2 / AVX512 CPU kernels evaluate `output += t * w`.  An axis
 * with in == out copies its samples.  An upscaling axis (scale < 1) has support
 * 1: the plain bilinear filter up to the last bit.
 *
 * Supported: scale <= 8 on each axis (at most 17 taps); a larger one returns
 * MDE_ERR_UNSUPPORTED before any launch.
 */
#ifndef MDE_AA_ABI_H
#define MDE_AA_ABI_H

#include "mde_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * mde_infer_prep (mde_infer_abi.h) with the filter above in place of the plain
 * bilinear one; everything else is that entry's contract.
 *   frames, layout 0: uint8 [n, H, W, 3]; a sample u becomes fl((float)u / 255).
 *   frames, layout 1: fp32 [n, 3, H, W] in [0, 1].
 *   out: fp32 [views * n, 3, h, w], views 1 or 2.  Rows 0 .. n-1 are view 0,
 *     the frames; rows n .. 2n-1 are view 1, the horizontally flipped frames:
 *     the order of cat([image, flip(image, [3])]).
 *   view 1 is the resize OF THE FLIPPED FRAME: output pixel (y, x) uses column
 *     x's xmin, xsize and weights on the frame's columns W-1-(xmin+j).
 *   n * H, views * n * 3 * h < 2^31; W, w < 2^30.  NULL pointers, non-positive
 *     sizes, a layout other than 0 / 1 or views other than 1 / 2 return
 *     MDE_ERR_INVALID_ARG; H / h or W / w above 8 returns MDE_ERR_UNSUPPORTED.
 *   Algorithmic bytes, layout 0: n (3 H W + 4 views 3 h w).
 * ------------------------------------------------------------------------- */
int mde_aa_prep(const void* frames, void* out, int64_t n, int64_t H, int64_t W, int64_t h,
                int64_t w, int layout, int views, void* stream);

/* ---------------------------------------------------------------------------
 * The same kernel on planes: x fp32 [planes, H, W] -> y fp32 [planes, h, w]
 * (an [n, c, H, W] tensor has planes = n c).  Forward only.
 *   dtype: MDE_F32, anything else returns MDE_ERR_UNSUPPORTED.
 *   planes * H, planes * h < 2^31; W, w < 2^30; else MDE_ERR_INVALID_ARG, as
 *     for NULL pointers and non-positive sizes.  H / h or W / w above 8 returns
 *     MDE_ERR_UNSUPPORTED.
 *   Algorithmic bytes: 4 planes (H W + h w).
 * ------------------------------------------------------------------------- */
int mde_aa_resize_fwd(const void* x, void* y, int64_t planes, int64_t H, int64_t W, int64_t h,
                      int64_t w, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * HOST function, HOST pointers: the tables of one axis, from the arithmetic the
 * kernel runs (one shared inline function).  For i < out: xmin[i], xsize[i] and
 * weights[i * stride + j], j < xsize[i]; the floats from xsize[i] up to stride
 * are set to zero.  End taps may carry weight zero.
 *   Returns the largest xsize (<= 17), which `stride` must reach; negative:
 *   MDE_ERR_INVALID_ARG for NULL pointers, non-positive sizes, in or out
 *   >= 2^31 or a stride below the largest xsize (nothing is written then),
 *   MDE_ERR_UNSUPPORTED for in / out above 8.
 * ------------------------------------------------------------------------- */
int mde_aa_axis_weights(int64_t in, int64_t out, int32_t* xmin, int32_t* xsize, float* weights,
                        int64_t stride);

#ifdef __cplusplus
}
#endif

#endif /* MDE_AA_ABI_H */
