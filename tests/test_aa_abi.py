"""The antialiased-resize ABI (include/mde_aa_abi.h, _abi.AA_SIGNATURES) on the CPU: header,
table and exports; the argument checks of the launching entries, which return before any
HIP call; and mde_aa_axis_weights, the host function that runs the kernel's own weight
arithmetic (csrc/aaweights.h), against ATen's weights.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import _aa_cases as A
from tests.conftest import REPO

HEADER = os.path.join(REPO, "include", "mde_aa_abi.h")
NAMES = {"mde_aa_prep", "mde_aa_resize_fwd", "mde_aa_axis_weights"}
AXIS_PAIRS = [(16, 8), (18, 7), (53, 17), (16, 20), (7, 7), (1242, 640), (1300, 650), (64, 8),
              (375, 192)]


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int64_t|int|size_t|double|const char\*)\s+(mde_\w+)\s*\(([^)]*)\)\s*;",
                         text):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return decls


def test_header_and_table_agree_and_are_exported():
    from monocular_depth_estimation_amd import _abi
    lib = _abi.load()
    d = declared_functions()
    assert set(d) == NAMES
    assert set(_abi.AA_SIGNATURES) == set(d)
    for name, nargs in d.items():
        assert hasattr(lib, name), f"{name} not exported by {_abi.LIB_PATH}"
        res, args = _abi.AA_SIGNATURES[name]
        assert len(args) == nargs, f"{name}: ctypes arity != header arity"
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)  # load() applied the table
    assert '#include "mde_abi.h"' in open(HEADER).read()
    # the host query takes typed pointers, so the guard harness does not wrap it as a launch
    assert ctypes.c_void_p not in _abi.AA_SIGNATURES["mde_aa_axis_weights"][1]


def test_four_tables_are_disjoint():
    from monocular_depth_estimation_amd import _abi
    tables = [set(_abi.SIGNATURES), set(_abi.EVAL_SIGNATURES), set(_abi.INFER_SIGNATURES),
              set(_abi.AA_SIGNATURES)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert not tables[i] & tables[j], (i, j)
    assert len(tables[3]) == 3


def test_prep_invalid_arguments_are_rejected_before_launch():
    """Every call below returns from the argument checks: the non-null pointers are never
    dereferenced (they are not device memory) and nothing is launched."""
    from monocular_depth_estimation_amd import _abi
    f = _abi.load().mde_aa_prep
    p = 0x1000  # non-null
    ok = (2, 13, 18, 5, 7)  # n, H, W, h, w
    assert f(None, p, *ok, 0, 2, None) == -1
    assert f(p, None, *ok, 0, 2, None) == -1
    for k in range(5):
        for bad in (0, -3):
            sizes = list(ok)
            sizes[k] = bad
            assert f(p, p, *sizes, 0, 2, None) == -1, sizes
    for layout in (-1, 2, 7):
        assert f(p, p, *ok, layout, 2, None) == -1, layout
    for views in (-1, 0, 3):
        assert f(p, p, *ok, 1, views, None) == -1, views
    # n * H < 2^31, views * n * 3 * h < 2^31, W < 2^30, w < 2^30
    assert f(p, p, 1 << 20, 1 << 11, 18, 5, 7, 0, 1, None) == -1
    assert f(p, p, 1 << 20, 13, 18, 1 << 11, 7, 0, 1, None) == -1
    assert f(p, p, 1 << 27, 1, 18, 3, 7, 1, 2, None) == -1      # 2 * 2^27 * 3 * 3 >= 2^31
    assert f(p, p, 1, 13, 1 << 30, 5, 7, 0, 2, None) == -1
    assert f(p, p, 1, 13, 18, 5, 1 << 30, 0, 2, None) == -1
    assert f(p, p, 1 << 40, 1 << 40, 18, 1 << 40, 7, 0, 2, None) == -1  # no wrap-around
    # scale 8.5 on either axis: unsupported, and an argument error still comes first
    assert f(p, p, 2, 17, 18, 2, 7, 0, 2, None) == -2
    assert f(p, p, 2, 13, 17, 5, 2, 1, 1, None) == -2
    assert f(None, p, 2, 17, 18, 2, 7, 0, 2, None) == -1


def test_resize_invalid_arguments_are_rejected_before_launch():
    from monocular_depth_estimation_amd import _abi
    f = _abi.load().mde_aa_resize_fwd
    p = 0x1000
    ok = (10, 13, 18, 5, 7)  # planes, H, W, h, w
    assert f(None, p, *ok, 0, None) == -1
    assert f(p, None, *ok, 0, None) == -1
    for k in range(5):
        for bad in (0, -3):
            sizes = list(ok)
            sizes[k] = bad
            assert f(p, p, *sizes, 0, None) == -1, sizes
    # dtype: MDE_F32 only
    assert f(p, p, *ok, 1, None) == -2
    assert f(p, p, *ok, 7, None) == -2
    # planes * H, planes * h < 2^31; W, w < 2^30
    assert f(p, p, 1 << 20, 1 << 11, 18, 5, 7, 0, None) == -1
    assert f(p, p, 1 << 20, 13, 18, 1 << 11, 7, 0, None) == -1
    assert f(p, p, 1, 13, 1 << 30, 5, 7, 0, None) == -1
    assert f(p, p, 1, 13, 18, 5, 1 << 30, 0, None) == -1
    assert f(p, p, 1 << 40, 1 << 40, 18, 1 << 40, 7, 0, None) == -1
    assert f(p, p, 10, 17, 18, 2, 7, 0, None) == -2             # scale 8.5
    assert f(p, p, 10, 13, 17, 5, 2, 0, None) == -2


def test_scale_limit_is_eight_inclusive():
    """8.5 is refused by every entry; exactly 8 passes the check.  The three entries share
    one predicate (aaweights.h, aa_axis_supported), and passing it is shown on the host
    query: a launching entry that passes its checks launches, which no CPU test may do
    with fake pointers (test_gpu_aa.py runs scale 8 on the device)."""
    from monocular_depth_estimation_amd import _abi
    lib = _abi.load()
    p = 0x1000
    assert lib.mde_aa_prep(p, p, 1, 17, 64, 2, 8, 0, 2, None) == -2
    assert lib.mde_aa_resize_fwd(p, p, 1, 40, 17, 5, 2, 0, None) == -2
    assert A.axis_tables(17, 2)[3] == -2
    xmin, xsize, wts, most = A.axis_tables(64, 8)
    assert 0 < most <= 17
    xmin, xsize, wts, most = A.axis_tables(40, 5)
    assert 0 < most <= 17


def test_axis_weights_argument_checks():
    from monocular_depth_estimation_amd import _abi
    f = _abi.load().mde_aa_axis_weights
    xmin = (ctypes.c_int32 * 8)()
    xsize = (ctypes.c_int32 * 8)()
    w = (ctypes.c_float * (8 * 17))()
    assert f(16, 8, None, xsize, w, 17) == -1
    assert f(16, 8, xmin, None, w, 17) == -1
    assert f(16, 8, xmin, xsize, None, 17) == -1
    assert f(0, 8, xmin, xsize, w, 17) == -1
    assert f(16, 0, xmin, xsize, w, 17) == -1
    assert f(1 << 31, 8, xmin, xsize, w, 17) == -1
    assert f(16, 8, xmin, xsize, w, 0) == -1
    for k in range(8 * 17):
        w[k] = -7.0
    assert f(16, 8, xmin, xsize, w, 3) == -1                    # 4 taps needed
    assert all(v == -7.0 for v in w) and not any(xsize)         # and nothing was written
    assert f(16, 8, xmin, xsize, w, 4) == 4


@pytest.mark.parametrize("n_in,n_out", AXIS_PAIRS)
def test_axis_weights_are_atens(n_in, n_out):
    """ATen's own weights, recovered on the CPU: resizing the identity matrix along its
    columns only (the rows keep their size, and an axis that keeps its size is copied)
    puts output i's weight vector into column i.  xmin / xsize must cover exactly the
    support of ATen's nonzero weights (zero-weight end taps allowed) and the weights must
    agree within 2^-23; the arithmetic is the same, so they are mostly equal."""
    ref = TF.interpolate(torch.eye(n_in)[None, None], size=(n_in, n_out), mode="bilinear",
                         antialias=True)[0, 0].numpy()
    xmin, xsize, wts, most = A.axis_tables(n_in, n_out)
    assert most == int(xsize.max()) and 1 <= most <= 17
    dense = np.zeros((n_in, n_out), dtype=np.float32)
    for i in range(n_out):
        assert 0 <= xmin[i] and xsize[i] >= 1 and xmin[i] + xsize[i] <= n_in
        dense[xmin[i]:xmin[i] + xsize[i], i] = wts[i, :xsize[i]]
        assert not wts[i, xsize[i]:].any()                      # the rest of the stride is zero
        nz = np.flatnonzero(ref[:, i])
        assert xmin[i] <= nz[0] and nz[-1] < xmin[i] + xsize[i], (i, xmin[i], xsize[i], nz)
        # nothing but zero-weight END taps beyond ATen's support
        mine = np.flatnonzero(dense[:, i])
        assert mine[0] == nz[0] and mine[-1] == nz[-1], (i, mine, nz)
    err = float(np.abs(dense - ref).max())
    print(f"{n_in} -> {n_out}: {most} taps, max |w - ATen| = {err:.3e}, "
          f"equal: {bool((dense == ref).all())}")
    assert err <= 2.0 ** -23, err


@pytest.mark.parametrize("name", list(A.CASES))
def test_emulation_against_the_yardstick(name):
    """The numpy fp32 emulation of aa.hip's arithmetic (tests/_aa_cases.py: the library's
    host weights, horizontal then vertical, sequential fused taps) against ATen on the CPU,
    for the frames and the planes of every case.  This is where test_gpu_aa.py's bound
    comes from: TOL = 2 x the largest figure printed here (1.5 * 2^-24, at `generic`)."""
    _, _, _, h, w = A.CASES[name]
    d_frames = float((A.yardstick(name) - A.emulate_case(name)).abs().max())
    x = A.planes(name)
    d_planes = float((A.aten_aa(x, (h, w)) - torch.from_numpy(A.emulate(x.numpy(), (h, w))))
                     .abs().max())
    print(f"{name}: frames {d_frames / 2.0 ** -24:.2f}, planes {d_planes / 2.0 ** -24:.2f} "
          f"x 2^-24")
    assert max(d_frames, d_planes) <= A.TOL / 2
    if name == "identity":
        assert d_frames == 0 and d_planes == 0


def test_python_refusals_need_no_device():
    """What antialias=True refuses is refused before anything touches a device."""
    from monocular_depth_estimation_amd import functional as F
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.infer_prep(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), (2, 2), antialias=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.bilinear_resize(torch.zeros((1, 1, 4, 4)), size=(2, 2), antialias=True)
    with pytest.raises(ValueError):
        F.interpolate(torch.zeros((1, 1, 4, 4)), size=(2, 2), mode="nearest", antialias=True)


def test_get_args_has_no_antialias_option_and_the_namespace_carries_it():
    from monocular_depth_estimation_amd.GuideDepth.inference import get_args
    a = get_args([])
    assert "antialias" not in vars(a)
    with pytest.raises(SystemExit):
        get_args(["--antialias"])
