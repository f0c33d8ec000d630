"""Shared by test_aa_abi.py (CPU) and test_gpu_aa.py (GPU): the cases of the antialiased
resize, their seeded frames, the yardstick, and a numpy fp32 emulation of aa.hip's
arithmetic built on the library's own host weights (mde_aa_axis_weights).

The yardstick is torch on the CPU:
    F.interpolate(cat([img, flip(img, [3])]), size, mode='bilinear', antialias=True)
of img = the host to_tensor of the frames.  That is what torchvision's
transforms.Resize runs on float tensors from 0.17 on; torchvision itself is not a
dependency of this repository, so the tests call F.interpolate directly.
"""
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as TF

# name: (n, H, W, h, w)
CASES = {
    "half": (2, 12, 16, 6, 8),
    "generic": (3, 13, 18, 5, 7),
    "thirds": (1, 37, 53, 11, 17),
    "mixed_up_down": (1, 16, 16, 20, 8),
    "identity": (3, 5, 7, 5, 7),
    "upscale": (1, 5, 7, 13, 18),
    "row_wider_than_tile": (1, 6, 1300, 3, 650),
    "far_columns": (1, 4, 1242, 2, 640),
    "far_rows": (1, 375, 6, 192, 3),
    "scale_8": (1, 40, 64, 5, 8),
    # 66000 (frame, tile) pairs, 65536 blocks launched: the kernel strides over the rest
    "more_tiles_than_blocks": (66000, 4, 4, 2, 2),
}

# 2 x the largest deviation of the emulation below from the yardstick over CASES, frames and
# planes(), measured on the CPU before the first GPU run
# (test_aa_abi.py::test_emulation_against_the_yardstick prints it per case): 0 at every case
# but `generic`, where ATen's 18 -> 7 weights differ from the fp32 formula's by 2.6e-8 and the
# result by 1.5 * 2^-24 = 8.9e-8.  So the bound is 3 * 2^-24 = 1.79e-7.
TOL = 3 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def frames(name):
    """Seeded uint8 [n, H, W, 3] on the host: random over 0..255, 0 and 255 forced into
    the four corners and the last column (as test_gpu_infer_kernels.py does)."""
    n, H, W, _, _ = CASES[name]
    gen = torch.Generator().manual_seed(5000 + sorted(CASES).index(name))
    f = torch.randint(0, 256, (n, H, W, 3), generator=gen, dtype=torch.uint8)
    f[:, :, W - 1, :] = torch.tensor([0, 255, 0], dtype=torch.uint8)
    f[:, 0, 0, :] = torch.tensor([0, 255, 255], dtype=torch.uint8)
    f[:, 0, W - 1, :] = torch.tensor([255, 0, 255], dtype=torch.uint8)
    f[:, H - 1, 0, :] = torch.tensor([255, 255, 0], dtype=torch.uint8)
    f[:, H - 1, W - 1, :] = torch.tensor([0, 0, 255], dtype=torch.uint8)
    return f


def to_tensor(fr):
    """torchvision's to_tensor for a batch of HWC uint8 frames (host arithmetic)."""
    assert not fr.is_cuda
    return fr.permute(0, 3, 1, 2).float().div(255).contiguous()


def aten_aa(x, size):
    assert not x.is_cuda
    return TF.interpolate(x, size=size, mode="bilinear", antialias=True)


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """[2n, 3, h, w] on the host, computed once."""
    _, _, _, h, w = CASES[name]
    img = to_tensor(frames(name))
    return aten_aa(torch.cat([img, torch.flip(img, [3])]), (h, w))


def axis_tables(n_in, n_out, stride=17):
    """(xmin, xsize, weights [n_out, stride], most taps) from mde_aa_axis_weights."""
    from monocular_depth_estimation_amd import _abi
    xmin = np.zeros(n_out, dtype=np.int32)
    xsize = np.zeros(n_out, dtype=np.int32)
    wts = np.full((n_out, stride), np.nan, dtype=np.float32)
    i32p, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    most = _abi.load().mde_aa_axis_weights(n_in, n_out, xmin.ctypes.data_as(i32p),
                                           xsize.ctypes.data_as(i32p), wts.ctypes.data_as(fp),
                                           stride)
    return xmin, xsize, wts, most


def _pass_last_axis(x, n_out):
    """One separable pass of aa.hip along the last axis of fp32 x: fl(t_0 w_0), then
    acc = fma(t_j, w_j, acc); an axis that keeps its size is copied.  The fma is taken in
    float64 and rounded to fp32: the product of two fp32 numbers is exact in float64, and
    the sum is rounded twice only where it falls within 2^-29 relative of an fp32 tie."""
    n_in = x.shape[-1]
    if n_in == n_out:
        return x.copy()
    xmin, xsize, wts, most = axis_tables(n_in, n_out)
    assert most > 0
    acc = x[..., xmin] * wts[:, 0]
    assert acc.dtype == np.float32
    w64 = wts.astype(np.float64)
    for j in range(1, most):
        live = xsize > j
        idx = np.where(live, xmin + j, 0)
        fused = (acc.astype(np.float64) + x[..., idx].astype(np.float64) * w64[:, j])
        acc = np.where(live, fused.astype(np.float32), acc)
    return acc


def emulate(x, size):
    """aa.hip's result for fp32 [..., H, W] numpy x: horizontal pass, fp32 intermediate,
    vertical pass."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hor = _pass_last_axis(x, size[1])
    ver = _pass_last_axis(np.ascontiguousarray(np.swapaxes(hor, -1, -2)), size[0])
    return np.ascontiguousarray(np.swapaxes(ver, -1, -2))


@functools.lru_cache(maxsize=None)
def planes(name):
    """Seeded fp32 [2, 5, H, W] in [0, 1) on the host for the tensor path (5 planes per
    sample: not the frames' 3; the frames' range, so that TOL holds for both)."""
    _, H, W, _, _ = CASES[name]
    gen = torch.Generator().manual_seed(6000 + sorted(CASES).index(name))
    return torch.rand((2, 5, H, W), generator=gen)


def emulate_case(name):
    _, _, _, h, w = CASES[name]
    img = to_tensor(frames(name))
    return torch.from_numpy(emulate(torch.cat([img, torch.flip(img, [3])]).numpy(), (h, w)))
