/*
 * mde_infer_abi.h — the inference entries of libmde_hip.so.
 *
 * A third header beside mde_abi.h (the frozen training ABI) and mde_eval_abi.h
 * (the evaluation tail), for the two ends of the deployed GuideDepth path
 * (src/GuideDepth/inference.py): camera frame -> network input, and network
 * output -> metric depth map.  It adds to the other two and changes nothing in
 * them.  The symbols live in the same library and follow the same conventions
 * (mde_abi.h "Conventions"): plain DEVICE pointers owned by the caller, `dtype`
 * selects the element type (MDE_F32 only here, anything else returns
 * MDE_ERR_UNSUPPORTED), `stream` is a hipStream_t and the last argument, 0 on
 * success / positive hipError_t / negative MDE_ERR_*, and nothing is launched
 * when an argument error is returned.  Neither entry needs scratch.  Both are
 * one kernel launch with no host synchronisation and no allocation, so both may
 * be captured into a hipGraph.  The Python mirror is _abi.INFER_SIGNATURES.
 */
#ifndef MDE_INFER_ABI_H
#define MDE_INFER_ABI_H

#include "mde_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * Front end: frames to the network's input, both evaluation views in one pass.
 * Replaces, in Inference_Engine.tensorRT_evaluate
 * (src/GuideDepth/inference.py:215-227): to_tensor (:218), torch.flip of the
 * image (:223) and downscale_image of the image and of its flip (:225-227).
 *   frames, layout 0: uint8 [n, H, W, 3], what a camera or the dataset gives.
 *     A sample u becomes fl((float)u / 255), torchvision's to_tensor
 *     (byte.permute(2, 0, 1).float().div(255)).
 *   frames, layout 1: fp32 [n, 3, H, W] in [0, 1], an image already a tensor.
 *   out: fp32 [views * n, 3, h, w], views 1 or 2.  Rows 0 .. n-1 are view 0,
 *     the frames; rows n .. 2n-1 are view 1, the horizontally flipped frames:
 *     the order of cat([image, flip(image, [3])]).
 *   bilinear: align_corners=False, scales H / h and W / w in fp32
 *     (F.interpolate(size=...)), mde_bilinear_fwd's generic arithmetic:
 *     horizontal pairs first, each l0 a + l1 b as fma(l1, b, fl(l0 a)).
 *     h == H and w == W gives the sample itself (no 0 * x term).
 *   view 1 is the resize OF THE FLIPPED FRAME, not the flip of view 0: output
 *     pixel (y, x) interpolates the flipped frame's columns i0, i1 with weights
 *     l0, l1, that is the frame's columns W-1-i0 and W-1-i1.  (The two differ
 *     in the last bit: fma(l1, b, fl(l0 a)) is not symmetric in a and b.)
 *   For every size at which mde_bilinear_fwd takes its generic kernel (every
 *     downscale, every non-dyadic upscale) out is bit for bit
 *     bilinear(cat([image, flip(image)])) of the fp32 image.
 *   n * H, views * n * 3 * h < 2^31; W, w < 2^30.  NULL pointers, non-positive
 *     sizes, a layout other than 0 / 1 or views other than 1 / 2 return
 *     MDE_ERR_INVALID_ARG.
 *   Algorithmic bytes, layout 0: n (3 H W + 4 views 3 h w).
 * ------------------------------------------------------------------------- */
int mde_infer_prep(const void* frames, void* out, int64_t n, int64_t H, int64_t W, int64_t h,
                   int64_t w, int layout, int views, void* stream);

/* ---------------------------------------------------------------------------
 * Back end: the network's output to a metric depth map at the frame's
 * resolution.  Replaces inverse_depth_norm (src/GuideDepth/inference.py:234,
 * 300-303) and upscale_depth (:245-247).  What mde_eval_pair_sums
 * (mde_eval_abi.h) only compares with the ground truth, this entry writes.
 *   inv [n, ph, pw] fp32: the network's raw output (a [n,1,ph,pw] map is the
 *     same memory).
 *   depth [n, H, W] fp32, metres: bilinear(D(inv)).
 *   D(v) = clamp(max_depth / v, max_depth / 100, max_depth) with torch.clamp's
 *     semantics (v = 0 -> max_depth, v < 0 -> max_depth / 100, NaN stays NaN),
 *     applied to the four source samples BEFORE the interpolation, the
 *     quotient rounded as fl(fl(1 / v) * max_depth): mde_eval_pair_sums' D.
 *   bilinear: align_corners=False, scales ph / H and pw / W in fp32, the
 *     generic arithmetic at EVERY ratio; ph == H and pw == W gives D of the
 *     sample itself (a NaN does not reach its neighbours).
 *   At every pixel the value is the prediction mde_eval_pair_sums compares
 *     with gt for view 0, bit for bit, also at the dyadic ratios where
 *     mde_bilinear_fwd takes its exact x2 / x4 / x8 kernels (which round
 *     differently in the last bit).
 *   n * H, n * ph < 2^31; W, pw < 2^30; else MDE_ERR_INVALID_ARG, as for NULL
 *     pointers and non-positive sizes.
 *   Algorithmic bytes: 4 n (ph pw + H W).
 * ------------------------------------------------------------------------- */
int mde_infer_depth(const void* inv, void* depth, int64_t n, int64_t ph, int64_t pw, int64_t H,
                    int64_t W, float max_depth, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDE_INFER_ABI_H */
