"""The image-logging ABI (include/mde_viz_abi.h, _abi.VIZ_SIGNATURES) on the CPU: header,
table and exports; the argument checks of the launching entries, which return before any
HIP call; the two host entries; the numpy oracle of tests/_viz_cases.py and the library's
colormap tables against the golden file and, where it imports, matplotlib itself; and
the host-side Python of the feature (utils.colorize on a CPU tensor, --log-images,
ImageDirWriter).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _viz_cases as V
from tests.conftest import REPO

HEADER = os.path.join(REPO, "include", "mde_viz_abi.h")
NAMES = {"mde_viz_colorize_grid", "mde_viz_image_grid", "mde_viz_grid_shape", "mde_viz_cmap_lut"}
LAUNCHING = {"mde_viz_colorize_grid", "mde_viz_image_grid"}
INVALID, UNSUPPORTED = -1, -2


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
    assert set(_abi.VIZ_SIGNATURES) == set(d)
    for name, nargs in d.items():
        assert hasattr(lib, name), f"{name} not exported by {_abi.LIB_PATH}"
        res, args = _abi.VIZ_SIGNATURES[name]
        assert len(args) == nargs, f"{name}: ctypes arity != header arity"
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)  # load() applied the table
    assert '#include "mde_abi.h"' in open(HEADER).read()
    # the host entries take typed pointers, so the guard harness does not wrap them as launches
    from tests._abi_guard import launching_entries
    assert launching_entries(_abi.VIZ_SIGNATURES) == LAUNCHING
    text = open(HEADER).read()
    for name, code in _abi.MDE_CMAPS.items():
        assert re.search(rf"#define MDE_CMAP_{name.upper()} {code}\b", text), name


def test_seven_tables_are_disjoint():
    from monocular_depth_estimation_amd import _abi
    tables = [set(t) for t in (_abi.SIGNATURES, _abi.EVAL_SIGNATURES, _abi.INFER_SIGNATURES,
                               _abi.AA_SIGNATURES, _abi.FOLD_SIGNATURES,
                               _abi.WGRAD_FOLD_SIGNATURES, _abi.VIZ_SIGNATURES)]
    for i in range(7):
        for j in range(i + 1, 7):
            assert not tables[i] & tables[j], (i, j)
    assert len(tables[6]) == 4


def test_colorize_grid_invalid_arguments_are_rejected_before_launch():
    """Every call below returns from the argument checks: the non-null pointers are never
    dereferenced (they are not device memory) and nothing is launched."""
    from monocular_depth_estimation_amd import _abi
    f = _abi.load().mde_viz_colorize_grid
    p = 0x1000  # non-null
    ok = (7, 5, 9, 6, 2)  # n, h, w, nrow, padding

    def call(x=p, xnorm=None, y=None, rng=None, ox=p, od=None, sizes=ok, cmap=0, dtype=0):
        return f(x, xnorm, y, rng, 10.0, 1000.0, ox, od, *sizes, 0.0, cmap, dtype, None)

    assert call(x=None) == INVALID
    assert call(ox=None, od=None) == INVALID               # at least one output
    assert call(od=p, y=None) == INVALID                   # out_diff requires y
    assert call(ox=None, od=p, y=None) == INVALID
    for k in range(3):                                     # n, h, w positive
        for bad in (0, -3):
            s = list(ok)
            s[k] = bad
            assert call(sizes=s) == INVALID, s
    for nrow in (0, -1):
        assert call(sizes=(7, 5, 9, nrow, 2)) == INVALID
    assert call(sizes=(7, 5, 9, 6, -1)) == INVALID
    for cmap in (-1, 3, 99):
        assert call(cmap=cmap) == INVALID, cmap
    # 3 Hg Wg >= 2^31, and sizes that would wrap a 64-bit product
    assert call(sizes=(1, 1 << 15, 1 << 15, 8, 2)) == INVALID          # 3 * 2^30
    assert call(sizes=(1, 26755, 26755, 8, 2)) == INVALID              # 3 * 26755^2 = 2^31 + ...
    assert call(sizes=(4, 1 << 14, 1 << 14, 2, 0)) == INVALID          # 3 * (2^15)^2
    assert call(sizes=(1 << 40, 1 << 40, 1 << 40, 1 << 40, 1 << 40)) == INVALID
    assert call(sizes=(2, (1 << 31) - 1, (1 << 31) - 1, 1, (1 << 31) - 1)) == INVALID
    assert call(sizes=((1 << 31) - 1, (1 << 31) - 1, 1, 1, (1 << 31) - 1)) == INVALID
    # dtype: MDE_F32 only, and an argument error wins
    assert call(dtype=1) == UNSUPPORTED
    assert call(dtype=7) == UNSUPPORTED
    assert call(dtype=1, x=None) == INVALID
    assert call(dtype=1, cmap=5) == INVALID
    assert call(dtype=1, sizes=(7, 5, 9, 0, 2)) == INVALID


def test_image_grid_invalid_arguments_are_rejected_before_launch():
    from monocular_depth_estimation_amd import _abi
    f = _abi.load().mde_viz_image_grid
    p = 0x1000
    ok = (7, 3, 5, 9, 6, 2)  # n, c, h, w, nrow, padding

    def call(x=p, rng=p, out=p, sizes=ok, dtype=0):
        return f(x, rng, out, *sizes, 0.0, dtype, None)

    assert call(x=None) == INVALID
    assert call(rng=None) == INVALID
    assert call(out=None) == INVALID
    for k in (0, 2, 3):                                    # n, h, w positive
        for bad in (0, -3):
            s = list(ok)
            s[k] = bad
            assert call(sizes=s) == INVALID, s
    for c in (0, 2, 4, -1):
        assert call(sizes=(7, c, 5, 9, 6, 2)) == INVALID, c
    assert call(sizes=(7, 3, 5, 9, 0, 2)) == INVALID
    assert call(sizes=(7, 3, 5, 9, 6, -1)) == INVALID
    assert call(sizes=(1, 3, 1 << 15, 1 << 15, 8, 2)) == INVALID
    assert call(sizes=(1 << 40, 3, 1 << 40, 1 << 40, 1 << 40, 1 << 40)) == INVALID
    assert call(dtype=1) == UNSUPPORTED
    assert call(dtype=1, out=None) == INVALID
    assert call(dtype=1, sizes=(7, 2, 5, 9, 6, 2)) == INVALID


def test_grid_shape():
    from monocular_depth_estimation_amd import _abi
    from monocular_depth_estimation_amd import functional as F
    assert F.grid_shape(7, 240, 320, 6, 2) == (486, 1934)   # the reference's own comment
    assert F.grid_shape(7, 480, 640, 6, 2) == (966, 3854)
    assert F.grid_shape(1, 5, 9, 6, 2) == (5, 9)            # n == 1: the map itself
    assert F.grid_shape(5, 6, 7, 8, 0) == (6, 35)           # no padding
    assert F.grid_shape(13, 3, 5, 4, 3) == (4 * 6 + 3, 4 * 8 + 3)
    for name, (n, h, w, nrow, padding, _) in V.CASES.items():
        assert F.grid_shape(n, h, w, nrow, padding) == V.grid_shape(n, h, w, nrow, padding), name
    f = _abi.load().mde_viz_grid_shape
    hg, wg = ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert f(7, 5, 9, 6, 2, None, ctypes.byref(wg)) == INVALID
    assert f(7, 5, 9, 6, 2, ctypes.byref(hg), None) == INVALID
    for bad in ((0, 5, 9, 6, 2), (7, -1, 9, 6, 2), (7, 5, 0, 6, 2), (7, 5, 9, 0, 2), (7, 5, 9, 6, -1),
                (1 << 31, 5, 9, 6, 2), (2, (1 << 31) - 1, 9, 6, 2)):
        assert f(*bad, ctypes.byref(hg), ctypes.byref(wg)) == INVALID, bad
    assert (hg.value, wg.value) == (-7, -7)                 # nothing was written
    with pytest.raises(_abi.MdeError):
        F.grid_shape(7, 5, 9, 0, 2)


@pytest.mark.parametrize("name", V.CMAPS)
def test_cmap_lut_is_the_golden_table(name):
    from monocular_depth_estimation_amd import _abi
    from monocular_depth_estimation_amd import functional as F
    table = F.cmap_lut(name)
    assert table.dtype == np.uint8 and table.shape == (256, 3)
    np.testing.assert_array_equal(table, V.golden()[name])
    f = _abi.load().mde_viz_cmap_lut
    buf = (ctypes.c_uint8 * 768)()
    assert f(_abi.MDE_CMAPS[name], None) == INVALID
    for cmap in (-1, 3):
        assert f(cmap, buf) == INVALID
    with pytest.raises(ValueError):
        F.cmap_lut("jet")


@pytest.mark.parametrize("name", V.CMAPS)
def test_oracle_is_matplotlibs_bytes_on_the_recorded_edge_vector(name):
    """The fixture holds matplotlib's cmap(x, bytes=True)[..., :3] on the edge vector
    (tools/make_viz_golden.py): the oracle and utils.colorize on a CPU tensor equal it."""
    from monocular_depth_estimation_amd.utils import colorize
    g = V.golden()
    x = g["edge_x"]
    np.testing.assert_array_equal(x, V.edge_vector())       # bit patterns too, NaN == NaN
    want = g["edge_" + name]                                # [len, 3]
    got = V.colorize(x[None], cmap=name)                    # [3, 1, len]
    np.testing.assert_array_equal(got[:, 0].T, want)
    lib = colorize(torch.from_numpy(x.copy())[None, None], cmap=name)
    assert lib.dtype == np.uint8 and lib.shape == (3, 1, len(x))
    np.testing.assert_array_equal(lib[:, 0].T, want)


@pytest.mark.parametrize("name", V.CMAPS)
def test_against_matplotlib_itself(name):
    """With matplotlib installed: the library's table, the oracle and utils.colorize
    against matplotlib.colormaps[name](x, bytes=True)[..., :3], for the default range,
    another range, the automatic range and vmin == vmax."""
    matplotlib = pytest.importorskip("matplotlib")
    from monocular_depth_estimation_amd import functional as F
    from monocular_depth_estimation_amd.utils import colorize
    cm = matplotlib.colormaps[name]
    k = np.arange(256, dtype=np.float32) / np.float32(256)
    np.testing.assert_array_equal(F.cmap_lut(name), cm(k, bytes=True)[:, :3])
    finite = V.edge_vector(specials=False)
    for x, vmin, vmax in ((V.edge_vector(), 10, 1000), (V.edge_vector(-3.5, 7.25), -3.5, 7.25),
                          (finite, None, None), (finite, None, 700), (finite, 20, None),
                          (V.edge_vector(), 500, 500), (V.unit_edge_vector(), 0, 1)):
        with np.errstate(all="ignore"):
            lo = x.min() if vmin is None else np.float32(vmin)
            hi = x.max() if vmax is None else np.float32(vmax)
            t = (x - lo) / (hi - lo) if lo != hi else x * 0.
            want = cm(t, bytes=True)[..., :3]
        got = V.colorize(x[None], vmin, vmax, name)
        np.testing.assert_array_equal(got[:, 0].T, want, err_msg=f"oracle {vmin} {vmax}")
        lib = colorize(torch.from_numpy(x.copy())[None, None], vmin, vmax, name)
        np.testing.assert_array_equal(lib[:, 0].T, want, err_msg=f"utils.colorize {vmin} {vmax}")


def test_colorize_cpu_tensor_is_the_oracle():
    """utils.colorize on a host [C, H, W] tensor: channel 0 only, the oracle's bytes."""
    from monocular_depth_estimation_amd.utils import colorize
    x = V.maps("two_rows", edges=V.edge_vector())[:3]       # [3, 5, 9]: C = 3, channel 0 is used
    for kw in (dict(), dict(vmin=None, vmax=None), dict(vmin=500, vmax=500), dict(cmap="Reds")):
        xx = np.nan_to_num(x, nan=1.0, posinf=2.0, neginf=3.0) if "vmin" in kw else x
        got = colorize(torch.from_numpy(xx.copy()), **kw)
        want = V.colorize(xx[0], kw.get("vmin", 10), kw.get("vmax", 1000), kw.get("cmap", "plasma"))
        assert got.dtype == np.uint8 and got.shape == (3, 5, 9)
        np.testing.assert_array_equal(got, want)
    with pytest.raises(ValueError):
        colorize(torch.zeros(5, 9))
    with pytest.raises(ValueError):
        colorize(torch.zeros(1, 5, 9), cmap="jet")


def test_colorize_cpu_is_an_rgba_image():
    """colorizeCPU (src/utils.py:98-109): minimum to 0, maximum to 1, RGBA out."""
    pytest.importorskip("PIL")
    from monocular_depth_estimation_amd.utils import colorizeCPU
    v = np.random.default_rng(3).uniform(1.0, 4.0, size=(5, 7)).astype(np.float32)
    im = colorizeCPU(v)
    assert im.mode == "RGBA" and im.size == (7, 5)
    a = np.asarray(im)
    t = v - v.min()
    t /= t.max()
    np.testing.assert_array_equal(a[..., :3], V.lut("plasma")[V.entries(t)])
    assert (a[..., 3] == 255).all()
    assert tuple(a[np.unravel_index(v.argmax(), v.shape)][:3]) == tuple(V.golden()["plasma"][255])


def test_oracle_geometry_matches_the_reference_comment():
    """make_grid of [7, 1, 240, 320] with nrow=6 is (486, 1934) (src/train.py:173); the
    maps sit where torchvision puts them and every other pixel is the pad value."""
    g = V.make_grid(np.ones((7, 1, 240, 320), np.float32), 6, 2, 0.0)
    assert g.shape == (1, 486, 1934)
    assert g[0, 2, 2] == 1 and g[0, 1, 2] == 0 and g[0, 241, 321] == 1 and g[0, 242, 321] == 0
    assert g[0, 244, 2] == 1 and g[0, 244, 324] == 0       # map 6 starts row two, cell 7 is empty
    assert int(g.sum()) == 7 * 240 * 320


def test_parser_has_log_images_off_by_default():
    from monocular_depth_estimation_amd.train import build_parser
    a = build_parser().parse_args([])
    assert a.log_images == ""
    assert build_parser().parse_args(["--log-images", "pics"]).log_images == "pics"


def test_image_dir_writer_round_trips(tmp_path):
    from monocular_depth_estimation_amd.train import ImageDirWriter
    w = ImageDirWriter(tmp_path / "pics")
    img = np.random.default_rng(1).integers(0, 256, size=(3, 5, 7), dtype=np.uint8)
    w.add_image("Train.3.Ours", img, 12)
    raw = open(tmp_path / "pics" / "Train.3.Ours_12.ppm", "rb").read()
    head = b"P6\n7 5\n255\n"
    assert raw.startswith(head) and len(raw) == len(head) + 3 * 5 * 7
    back = np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(5, 7, 3).transpose(2, 0, 1)
    np.testing.assert_array_equal(back, img)
    # a float picture in [0, 1] (the RGB grid) and a tensor
    f = torch.tensor([0.0, 0.5, 1.0, 2.0, -1.0]).repeat(3, 2, 1)
    w.add_image("Train.1.Image", f, 0)
    raw = open(w.path("Train.1.Image", 0), "rb").read()
    px = np.frombuffer(raw[len(b"P6\n5 2\n255\n"):], dtype=np.uint8).reshape(2, 5, 3)
    assert px[0, :, 0].tolist() == [0, 127, 255, 255, 0]
    with pytest.raises(ValueError):
        w.add_image("bad", np.zeros((5, 7), np.uint8), 0)


def test_python_refusals_need_no_device():
    from monocular_depth_estimation_amd import functional as F
    x = torch.zeros(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.colorize_grid(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.image_grid(torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError, match="automatic range"):
        F.colorize_grid(x, y=x, vmin=None, want=("x", "diff"))
    with pytest.raises(ValueError, match="needs y"):
        F.colorize_grid(x, want=("diff",))
    with pytest.raises(ValueError):
        F.colorize_grid(x, want=("x", "x"))
