"""Hot-path utilities of src/utils.py on MI355X.

DepthNorm (utils.py:7-8) runs on HIP kernels (device min/max reduction +
normalise, no host sync).  AverageMeter (:10-24) is host bookkeeping.
compute_errors (:45-66) and the per-batch evaluation of src/test.py:96-124
(clamp, range mask, Eigen crop) run on one HIP reduction (mde_eval_sums):
only the sixteen sums come back to the host.  colorize (:69-96) runs on the
fused grid + colormap HIP kernel for a device tensor (functional.colorize_grid;
LogProgress in train.py uses that kernel on whole batches) and in numpy, with
the library's table and the same fp32 arithmetic, for a host tensor.
colorizeCPU (:98-109) is host only.  hconcat_resize (:26-41) is not provided:
it is cv2 resizing.
"""
from __future__ import annotations

import math

import numpy as np

from .functional import cmap_lut, colorize_grid, depth_norm, eigen_crop, eval_sums


def DepthNorm(depth):  # noqa: N802  (reference name)
    """(depth - depth.min()) / (depth.max() - depth.min()), batch-global."""
    return depth_norm(depth)


class AverageMeter:
    """Running value / sum / count / average (utils.py:10-24)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def errors_from_sums(s) -> list[float]:
    """[silog, abs_rel, log10, rms, sq_rel, log_rms, d1, d2, d3] (utils.py:45-66) from
    the mde_eval_sums sums; NaN when no pixel was selected (numpy's mean of [])."""
    s = [float(v) for v in (s.tolist() if hasattr(s, "tolist") else s)]
    n = s[0]
    if n == 0:
        return [math.nan] * 9
    d1, d2, d3 = s[1] / n, s[2] / n, s[3] / n
    rms = math.sqrt(s[4] / n)
    log_rms = math.sqrt(s[5] / n)
    abs_rel = s[6] / n
    sq_rel = s[7] / n
    mean_err = s[8] / n
    silog = math.sqrt(max(s[5] / n - mean_err * mean_err, 0.0)) * 100
    log10 = s[9] / n
    return [silog, abs_rel, log10, rms, sq_rel, log_rms, d1, d2, d3]


def compute_errors(gt, pred):
    """utils.py:45-66 on the GPU over the given (already selected) pixels.

    gt / pred: CUDA tensors of equal shape.  Returns the reference's list
    [silog, abs_rel, log10, rms, sq_rel, log_rms, d1, d2, d3] (Python floats).
    """
    return errors_from_sums(eval_sums(pred, gt))


def eval_batch_errors(gt_depth, pred_depth, min_depth_eval=1e-3, max_depth_eval=80.0,
                      crop=True):
    """One batch of src/test.py:96-118 on the GPU: pred clamped to
    [min_depth_eval, max_depth_eval] (NaN -> min), pixels with
    min_depth_eval < gt < max_depth_eval inside the Eigen crop, then
    compute_errors.  gt_depth / pred_depth: [n, 1, h, w] or [n, h, w] maps
    (gt already DepthNorm'ed, as test.py:91 does)."""
    h, w = gt_depth.shape[-2], gt_depth.shape[-1]
    c = eigen_crop(h, w) if crop else None
    return errors_from_sums(eval_sums(pred_depth, gt_depth, min_depth_eval, max_depth_eval,
                                      clamp_and_mask=True, crop=c))


def _color_entries(t):
    """matplotlib's Colormap.__call__ index of fp32 values t in [0, 1]: 0 .. 255, and 256
    for a NaN (the 'bad' colour).  xa = fl(t * 256); 256 -> 255; below 0 -> the under
    colour (entry 0), 256 and above -> the over colour (entry 255); else truncated."""
    with np.errstate(all="ignore"):
        xa = np.asarray(t, dtype=np.float32) * np.float32(256)
        nan = np.isnan(xa)
        idx = np.where(nan, np.float32(0), np.clip(xa, np.float32(0), np.float32(255)))
    return np.where(nan, 256, idx.astype(np.int64))


def colorize(value, vmin=10, vmax=1000, cmap="plasma"):
    """utils.py:69-96, drop-in: value is a [C, H, W] tensor, channel 0 is normalised to
    (value - vmin) / (vmax - vmin) (None: its own minimum / maximum; value * 0 when the
    two are equal) and mapped through the colormap; returns numpy uint8 [3, H, W].

    A device tensor runs the HIP kernel (one map, so the grid is the map) and the bytes
    come back; a host tensor runs the same fp32 arithmetic in numpy with the library's
    table.  Both equal matplotlib's cmap(value, bytes=True)[..., :3] byte for byte."""
    import torch
    if not torch.is_tensor(value) or value.dim() != 3:
        raise ValueError("colorize: expected a [C, H, W] tensor")
    if value.is_cuda:
        return colorize_grid(value[0:1].float(), vmin=vmin, vmax=vmax, cmap=cmap).cpu().numpy()
    v = value.detach()[0].float().numpy()
    with np.errstate(all="ignore"):
        lo = v.min() if vmin is None else np.float32(vmin)
        hi = v.max() if vmax is None else np.float32(vmax)
        t = (v - lo) / (hi - lo) if lo != hi else v * np.float32(0)
    table = np.concatenate([cmap_lut(cmap), np.zeros((1, 3), np.uint8)])
    return np.ascontiguousarray(table[_color_entries(t)].transpose(2, 0, 1))


def colorizeCPU(value, cmap="plasma"):  # noqa: N802  (reference name)
    """utils.py:98-109, host only: a numpy [H, W] map, shifted to minimum 0 and divided by
    its maximum, through the colormap; returns an RGBA PIL image (alpha 255; 0 where the
    value is NaN, matplotlib's 'bad' colour)."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("colorizeCPU returns a PIL image and PIL is not installed; "
                           "colorize() returns numpy and needs no extra library") from e
    image = np.array(value, dtype=np.float32)
    with np.errstate(all="ignore"):
        image -= image.min()
        image /= image.max()
    idx = _color_entries(image)
    rgba = np.concatenate([cmap_lut(cmap), np.full((256, 1), 255, np.uint8)], axis=1)
    rgba = np.concatenate([rgba, np.zeros((1, 4), np.uint8)])
    return Image.fromarray(rgba[idx])
