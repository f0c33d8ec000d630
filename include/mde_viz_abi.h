/*
 * mde_viz_abi.h — the image-logging kernels of libmde_hip.so: torchvision's
 * make_grid fused with the reference's colorize (src/train.py:160-194,
 * src/utils.py:69-96).
 *
 * A seventh header beside mde_abi.h (the frozen training ABI), mde_eval_abi.h,
 * mde_infer_abi.h, mde_aa_abi.h, mde_fold_abi.h and mde_wgrad_fold_abi.h, each
 * of which is pinned to its entries.  It adds to them and changes nothing in
 * them.  The symbols live in the same library and follow the same conventions
 * (mde_abi.h "Conventions"): plain DEVICE pointers owned by the caller for the
 * launching entries, `dtype` selects the element type, `stream` is a
 * hipStream_t and the last argument, 0 on success / positive hipError_t /
 * negative MDE_ERR_*, and nothing is launched when an argument error is
 * returned.  No entry needs scratch.  Each launching entry is one kernel launch
 * with no host synchronisation and no allocation, so it may be captured into a
 * hipGraph.  The Python mirror is _abi.VIZ_SIGNATURES.
 *
 * Grid geometry (torchvision.utils.make_grid) of n maps of h x w with `nrow`
 * maps per grid row, `padding` pixels between and around them:
 *   n == 1: the grid is the map, Hg = h, Wg = w, no padding (make_grid returns
 *     tensor.squeeze(0)).
 *   otherwise xmaps = min(nrow, n), ymaps = ceil(n / xmaps),
 *     Hg = ymaps (h + padding) + padding, Wg = xmaps (w + padding) + padding;
 *     map k occupies rows (k / xmaps)(h + padding) + padding ... + h and columns
 *     (k % xmaps)(w + padding) + padding ... + w; every other pixel, the cells
 *     after map n-1 included, holds pad_value.
 *   [7, 1, 240, 320] with nrow 6, padding 2 gives 486 x 1934.
 *
 * colorize (matplotlib's Colormap.__call__(X, bytes=True) on the normalised
 * value), every step fp32 and rounded on its own:
 *   d = fl(vmax - vmin);  t = fl(fl(v - vmin) / d), IEEE division, or
 *   t = fl(v * 0) when vmin == vmax;  xa = fl(t * 256);
 *   NaN -> RGB (0, 0, 0);  xa == 256 -> entry 255;  xa < 0 (-inf too) -> entry
 *   0;  xa >= 256 (+inf too) -> entry 255;  otherwise entry (int)xa, truncated
 *   (-0.0 is entry 0).
 * The entries are the uint8 RGB of matplotlib's 256-entry table,
 * (lut[:256, :3] * 255) truncated (csrc/cmaps.h, mde_viz_cmap_lut).  Pad pixels
 * go through the same arithmetic with v = pad_value.
 */
#ifndef MDE_VIZ_ABI_H
#define MDE_VIZ_ABI_H

#include "mde_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Colormaps (`cmap`). */
#define MDE_CMAP_PLASMA 0
#define MDE_CMAP_VIRIDIS 1
#define MDE_CMAP_REDS 2

/* ---------------------------------------------------------------------------
 * colorize(make_grid(x')) and / or colorize(make_grid(|x' - y|)) in one launch.
 *   x: fp32 [n, h, w] maps.
 *   xnorm: NULL, or a device float[2] {mn, mx}: x' = fl(fl(x - mn) / fl(mx - mn)),
 *     the arithmetic of mde_depthnorm_apply, so DepthNorm(x) is never written;
 *     NULL: x' = x.
 *   y: NULL, or fp32 [n, h, w]; dv = |fl(x' - y)|.
 *   range: NULL, or a device float[2] {vmin, vmax} that replaces the scalars
 *     (nothing is read back to the host); it applies to both outputs.
 *   out_x, out_diff: uint8 [3, Hg, Wg], colorize of x' / of dv; either may be
 *     NULL, not both; out_diff needs y.  Every byte of a given grid is written,
 *     pad pixels (colorize(pad_value), not normalised by xnorm) included.  Any
 *     byte alignment.
 *   cmap: MDE_CMAP_*.  dtype: MDE_F32.
 *   NULL x, NULL out_x and out_diff, out_diff without y, non-positive n / h / w,
 *     nrow < 1, padding < 0, an unknown cmap, Hg or Wg >= 2^31 or
 *     3 Hg Wg >= 2^31 return MDE_ERR_INVALID_ARG; otherwise a dtype other than
 *     MDE_F32 returns MDE_ERR_UNSUPPORTED.
 *   Algorithmic bytes: 4 n h w per input read (x, y) + 3 Hg Wg per grid written.
 * ------------------------------------------------------------------------- */
int mde_viz_colorize_grid(const void* x, const void* xnorm, const void* y, const void* range,
                          float vmin, float vmax, void* out_x, void* out_diff,
                          int64_t n, int64_t h, int64_t w, int64_t nrow, int64_t padding,
                          float pad_value, int cmap, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * make_grid(x, nrow, normalize=True): x fp32 [n, c, h, w], c 1 or 3 (one channel
 * is replicated to three), out fp32 [3, Hg, Wg].
 *   range: a device float[2] {lo, hi}, the minimum and maximum of x (mde_minmax);
 *     a sample becomes fl(fl(clamp(x, lo, hi) - lo) / max(fl(hi - lo), 1e-5f)).
 *   Pad pixels hold pad_value, not normalised.
 *   NULL pointers, non-positive sizes, nrow < 1, padding < 0, c other than 1 / 3,
 *     Hg or Wg >= 2^31 or 3 Hg Wg >= 2^31 return MDE_ERR_INVALID_ARG; otherwise a
 *     dtype other than MDE_F32 returns MDE_ERR_UNSUPPORTED.
 *   Algorithmic bytes: 4 n c h w read (3 n h w at c == 1: each plane re-reads
 *     the map) + 12 Hg Wg written.
 * ------------------------------------------------------------------------- */
int mde_viz_image_grid(const void* x, const void* range, void* out, int64_t n, int64_t c,
                       int64_t h, int64_t w, int64_t nrow, int64_t padding, float pad_value,
                       int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * HOST function, HOST pointers: the grid's size by the geometry above.
 *   MDE_ERR_INVALID_ARG for NULL pointers, non-positive n / h / w, nrow < 1,
 *   padding < 0 or a side >= 2^31 (nothing is written then).
 * ------------------------------------------------------------------------- */
int mde_viz_grid_shape(int64_t n, int64_t h, int64_t w, int64_t nrow, int64_t padding,
                       int64_t* Hg, int64_t* Wg);

/* ---------------------------------------------------------------------------
 * HOST function, HOST pointer: the 256 RGB entries of a colormap, the bytes the
 * kernel looks up (rgb768[3 k + channel]).  MDE_ERR_INVALID_ARG for a NULL
 * pointer or an unknown cmap.
 * ------------------------------------------------------------------------- */
int mde_viz_cmap_lut(int cmap, uint8_t* rgb768);

#ifdef __cplusplus
}
#endif

#endif /* MDE_VIZ_ABI_H */
