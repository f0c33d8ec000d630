#!/usr/bin/env python3
"""Image logging on the device against the reference-style path ("Image logging").

    python tools/viz_bench.py [--n 7 --height 480 --width 640 --reps 30]

Prints, for a batch of n maps:
  * the colorize kernel (one launch for 'Ours' + 'Diff', DepthNorm applied on load) and
    the image-grid kernel: time per launch from the timing registry (HIP events around
    each launch) and the achieved GB/s over their algorithmic bytes
    (include/mde_viz_abi.h).  Both are filed under the registry id `depthnorm_apply`,
    so each is timed in a window of its own;
  * the wall time of the image part of a log point (everything after the forward: the
    reductions, the three launches, the copies into one pinned buffer, one
    synchronise) against the reference-style path of tests/_viz_cases.py (make_grid in
    ATen, the fp32 grids copied to the host, colorize in numpy), the two alternating in
    one process; and that the pictures agree.
Needs a ROCm GPU.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from monocular_depth_estimation_amd import _abi  # noqa: E402
from monocular_depth_estimation_amd import functional as F  # noqa: E402
from tests import _viz_cases as V  # noqa: E402


def fused_pictures(image, depth, pred):
    """train.LogProgress after the forward, at epoch 0 (all four pictures)."""
    pics = [F.image_grid(image, nrow=6), F.colorize_grid(depth, nrow=6)]
    pics += F.colorize_grid(pred, y=depth, xnorm=F.minmax(pred), nrow=6, want=("x", "diff"))
    sizes = [(t.numel() * t.element_size() + 15) // 16 * 16 for t in pics]
    host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
    views, off = [], 0
    for t, nbytes in zip(pics, sizes):
        v = host[off:off + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
        v.copy_(t, non_blocking=True)
        views.append(v.numpy())
        off += nbytes
    torch.cuda.current_stream().synchronize()
    return views


def registry(fn, reps):
    torch.cuda.synchronize()
    _abi.timing_reset()
    _abi.timing_enable(True)
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        t = _abi.timing_collect()
    finally:
        _abi.timing_enable(False)
        _abi.timing_reset()
    ms, launches, nbytes, _ = t["depthnorm_apply"]
    return ms / launches * 1e3, nbytes / launches, nbytes / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=7)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("viz_bench.py needs a ROCm GPU")
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    image = torch.rand((a.n, 3, a.height, a.width), generator=g).to(dev)
    depth = (0.1 + 9.9 * torch.rand((a.n, 1, a.height, a.width), generator=g)).to(dev)
    pred = (5.0 * torch.rand((a.n, 1, a.height, a.width), generator=g)).to(dev)
    hg, wg = F.grid_shape(a.n, a.height, a.width, 6, 2)
    print(f"n={a.n} {a.height}x{a.width} nrow=6: grid {hg} x {wg}")

    mm = F.minmax(pred)
    ox = torch.empty((3, hg, wg), dtype=torch.uint8, device=dev)
    od = torch.empty_like(ox)
    oi = torch.empty((3, hg, wg), device=dev)
    for _ in range(3):  # warm up every shape the timed windows use
        F.colorize_grid(pred, y=depth, xnorm=mm, nrow=6, want=("x", "diff"), out=(ox, od))
        F.colorize_grid(depth, nrow=6, out=ox)
        F.image_grid(image, nrow=6, out=oi)
        fused_pictures(image, depth, pred)
        V.reference_style_pictures(image, depth, pred)
    rows = (("colorize x + diff", lambda: F.colorize_grid(pred, y=depth, xnorm=mm, nrow=6,
                                                           want=("x", "diff"), out=(ox, od))),
            ("colorize x alone", lambda: F.colorize_grid(depth, nrow=6, out=ox)))
    for what, fn in rows:
        us, nbytes, gbs = registry(fn, 200)
        print(f"{what:20s} {us:8.2f} us / launch  {nbytes / 1e6:7.2f} MB  {gbs:8.1f} GB/s")
    imm = F.minmax(image)
    us, nbytes, gbs = registry(lambda: _abi.call(
        "mde_viz_image_grid", _abi.ptr(image), _abi.ptr(imm), _abi.ptr(oi), a.n, 3, a.height,
        a.width, 6, 2, 0.0, _abi.MDE_F32, _abi.stream_of(image)), 200)
    print(f"{'image grid':20s} {us:8.2f} us / launch  {nbytes / 1e6:7.2f} MB  {gbs:8.1f} GB/s")

    fused, ref = [], []
    for _ in range(a.reps):  # alternating, each ending in a synchronise / a host copy
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mine = fused_pictures(image, depth, pred)
        t1 = time.perf_counter()
        theirs = V.reference_style_pictures(image, depth, pred)
        t2 = time.perf_counter()
        fused.append(t1 - t0)
        ref.append(t2 - t1)
    for what, t in (("fused log point", fused), ("reference-style", ref)):
        t = np.array(t) * 1e3
        print(f"{what:20s} median {np.median(t):8.3f} ms  min {t.min():8.3f}  max {t.max():8.3f}  "
              f"({a.reps} alternating runs)")
    print(f"ratio of medians: {np.median(ref) / np.median(fused):.1f}x")
    err = float(np.abs(mine[0] - theirs[0]).max())
    same = all(np.array_equal(m, t) for m, t in zip(mine[1:], theirs[1:]))
    print(f"pictures: image grid max |diff| {err:.3e}, colorized grids equal: {same}")


if __name__ == "__main__":
    main()
