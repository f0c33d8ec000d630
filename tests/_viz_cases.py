"""Cases and the numpy oracle of the image-logging kernels (csrc/viz.hip,
include/mde_viz_abi.h), shared by tests/test_viz_abi.py and tests/test_gpu_viz.py.

The oracle is the reference's path written out in numpy fp32: torchvision's make_grid
geometry (torchvision is not installed with this project), then colorize
(src/utils.py:69-96) with matplotlib's Colormap.__call__(X, bytes=True) arithmetic and
the colormap table from tests/golden/viz_cmaps.npz, which tools/make_viz_golden.py wrote
from matplotlib.  The fixture also holds matplotlib's own bytes on an edge vector, so
the oracle is checked against matplotlib even where matplotlib is absent.  Nothing here
calls the library under test.
"""
import os

import numpy as np

from tests.conftest import GOLDEN

CMAPS = ("plasma", "viridis", "Reds")
VMIN, VMAX = 10.0, 1000.0

# (n, h, w, nrow, padding, pad_value)
CASES = {
    "two_rows": (7, 5, 9, 6, 2, 0.0),        # two rows, five empty cells, odd sizes
    "squeeze": (1, 5, 9, 6, 2, 0.0),         # n == 1: the grid is the map
    "one_row": (6, 4, 8, 6, 2, 0.0),         # exactly one row
    "coloured_pad": (13, 3, 5, 4, 3, 500.0),
    "no_padding": (5, 6, 7, 8, 0, 0.0),
    "blocks": (3, 70, 130, 2, 2, 0.0),       # more than one block per map
}

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(GOLDEN, "viz_cmaps.npz"), allow_pickle=False) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def lut(name):
    """uint8 [257, 3]: the 256 entries, then the NaN colour (0, 0, 0)."""
    return np.concatenate([golden()[name], np.zeros((1, 3), np.uint8)])


# ------------------------------------------------------------------ geometry
def grid_shape(n, h, w, nrow=8, padding=2):
    if n == 1:
        return h, w
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    return ymaps * (h + padding) + padding, xmaps * (w + padding) + padding


def make_grid(maps, nrow=8, padding=2, pad_value=0.0):
    """maps [n, C, h, w] -> [C, Hg, Wg]: make_grid's placement, without its
    one-to-three-channel replication (the callers index or replicate themselves)."""
    maps = np.asarray(maps, dtype=np.float32)
    n, c, h, w = maps.shape
    if n == 1:
        return maps[0].copy()
    hg, wg = grid_shape(n, h, w, nrow, padding)
    xmaps = min(nrow, n)
    grid = np.full((c, hg, wg), np.float32(pad_value), dtype=np.float32)
    for k in range(n):
        y0 = (k // xmaps) * (h + padding) + padding
        x0 = (k % xmaps) * (w + padding) + padding
        grid[:, y0:y0 + h, x0:x0 + w] = maps[k]
    return grid


# ------------------------------------------------------------------ colorize
def entries(t):
    """Table entry of normalised fp32 values: matplotlib's Colormap.__call__ for floats."""
    t = np.asarray(t, dtype=np.float32)
    with np.errstate(all="ignore"):
        xa = t * np.float32(256)
        finite = np.nan_to_num(xa, nan=0.0, posinf=300.0, neginf=-300.0)
        trunc = np.clip(finite, -1.0, 300.0).astype(np.int64)   # truncation toward zero
        idx = np.where(xa == 256, 255, np.where(xa < 0, 0, np.where(xa >= 256, 255, trunc)))
    return np.where(np.isnan(xa), 256, idx)


def colorize(value, vmin=VMIN, vmax=VMAX, cmap="plasma"):
    """src/utils.py:69-96 on a [H, W] fp32 array -> uint8 [3, H, W]."""
    value = np.asarray(value, dtype=np.float32)
    with np.errstate(all="ignore"):
        lo = value.min() if vmin is None else np.float32(vmin)
        hi = value.max() if vmax is None else np.float32(vmax)
        t = (value - lo) / (hi - lo) if lo != hi else value * np.float32(0)
    return np.ascontiguousarray(lut(cmap)[entries(t)].transpose(2, 0, 1))


def depth_norm(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (x - x.min()) / (x.max() - x.min())


def colorize_grid(x, y=None, xnorm=False, vmin=VMIN, vmax=VMAX, cmap="plasma", nrow=8, padding=2,
                  pad_value=0.0):
    """What LogProgress logs, the reference's way.  x, y: [n, h, w] fp32.  Returns
    (colorize(make_grid(x')), colorize(make_grid(|x' - y|)) or None)."""
    x = np.asarray(x, dtype=np.float32)
    xp = depth_norm(x) if xnorm else x
    gx = colorize(make_grid(xp[:, None], nrow, padding, pad_value)[0], vmin, vmax, cmap)
    gd = None
    if y is not None:
        with np.errstate(all="ignore"):
            dv = np.abs(xp - np.asarray(y, dtype=np.float32))
        gd = colorize(make_grid(dv[:, None], nrow, padding, pad_value)[0], vmin, vmax, cmap)
    return gx, gd


def image_grid(x, nrow=8, padding=2, pad_value=0.0):
    """make_grid(x, nrow, normalize=True): x [n, c, h, w], c 1 or 3 -> fp32 [3, Hg, Wg]."""
    x = np.asarray(x, dtype=np.float32)
    lo, hi = x.min(), x.max()
    norm = (np.clip(x, lo, hi) - lo) / max(np.float32(hi - lo), np.float32(1e-5))
    if x.shape[1] == 1:
        norm = np.repeat(norm, 3, axis=1)
    return make_grid(norm.astype(np.float32), nrow, padding, pad_value)


# -------------------------------------------------------------------- inputs
def edge_vector(vmin=VMIN, vmax=VMAX, specials=True):
    """Every bin edge vmin + k / 256 (vmax - vmin) with its fp32 neighbours, both ends,
    values beyond them, +-0 and (specials) NaN and the infinities."""
    vmin, vmax = np.float32(vmin), np.float32(vmax)
    on = vmin + np.arange(257, dtype=np.float32) / np.float32(256) * (vmax - vmin)
    tail = [vmin, vmax, vmin - 1, vmin - 50, vmax + 1, vmax + 50, 0.0, -0.0]
    if specials:
        tail += [np.nan, np.inf, -np.inf]
    return np.concatenate([on, np.nextafter(on, np.float32(-np.inf)),
                           np.nextafter(on, np.float32(np.inf)),
                           np.float32(tail)]).astype(np.float32)


def unit_edge_vector():
    """The same for maps normalised to [0, 1]: every k / 256 and its neighbours."""
    return edge_vector(0.0, 1.0, specials=False)


def maps(name, seed=0, lo=VMIN - 50, hi=VMAX + 50, edges=None):
    """[n, h, w] fp32: uniform values in [lo, hi] with a third of the pixels replaced by
    edge values (each special value at least once when the map has room)."""
    n, h, w = CASES[name][:3]
    rng = np.random.default_rng([seed, n, h, w])
    x = rng.uniform(lo, hi, size=n * h * w).astype(np.float32)
    if edges is not None and len(edges):
        k = max(len(x) // 3, min(len(x), 16))
        pos = rng.choice(len(x), size=k, replace=False)
        x[pos] = rng.choice(edges, size=k)
        m = min(11, k)
        x[pos[:m]] = edges[-m:]        # the tail of the edge vector: ends, zeros, specials
    return x.reshape(n, h, w)


def images(name, c, seed=0):
    n, h, w = CASES[name][:3]
    rng = np.random.default_rng([seed, n, c, h, w])
    return rng.uniform(-3.0, 5.0, size=(n, c, h, w)).astype(np.float32)


# ------------------------------------------------- the reference-style log point
def aten_make_grid(t, nrow=8, padding=2, pad_value=0.0, normalize=False):
    """torchvision.utils.make_grid spelled out in ATen, op for op: the optional
    clone / clamp_ / sub_ / div_ of normalize, cat to three channels, full, and one
    narrow().copy_() per map.  t: a torch [n, c, h, w] tensor on any device."""
    import torch
    if t.size(1) == 1:
        t = torch.cat((t, t, t), 1)
    if normalize:
        t = t.clone()
        lo, hi = float(t.min()), float(t.max())
        t.clamp_(min=lo, max=hi)
        t.sub_(lo).div_(max(hi - lo, 1e-5))
    if t.size(0) == 1:
        return t.squeeze(0)
    n = t.size(0)
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    height, width = t.size(2) + padding, t.size(3) + padding
    grid = t.new_full((3, height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= n:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(
                2, x * width + padding, width - padding).copy_(t[k])
            k += 1
    return grid


def reference_style_pictures(image, depth, pred):
    """The image part of the reference's LogProgress (src/train.py:170-187) on device
    tensors: each grid built by aten_make_grid, copied to the host as fp32, then
    colorize in numpy with the oracle above.  Returns the four pictures."""
    import torch
    image_grid_ = aten_make_grid(image, nrow=6, normalize=True).cpu().numpy()
    gt = colorize(aten_make_grid(depth, nrow=6).cpu().numpy()[0])
    p = (pred - pred.min()) / (pred.max() - pred.min())
    ours = colorize(aten_make_grid(p, nrow=6).cpu().numpy()[0])
    diff = colorize(aten_make_grid(torch.abs(p - depth), nrow=6).cpu().numpy()[0])
    return image_grid_, gt, ours, diff
