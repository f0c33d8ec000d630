"""The image-logging kernels on the device (csrc/viz.hip, include/mde_viz_abi.h):
functional.colorize_grid / image_grid, utils.colorize on a device tensor, and
train.LogProgress.

The yardstick is the numpy oracle of tests/_viz_cases.py: make_grid's geometry, then
colorize with matplotlib's arithmetic and table.  Every byte output must be EXACTLY the
oracle's: each step is one IEEE fp32 operation on both sides, so there is no tolerance,
and no element is left out of a comparison.  The float grid of image_grid is compared
within 2^-22: its values are at most 1, the subtraction and the division are each
correctly rounded on the device, and an ATen build that multiplies by the reciprocal
instead differs by under 2^-23; the bound is twice that.  (Against the numpy oracle,
which divides, the kernel measured 0 at every case on the device.)
"""
import numpy as np
import pytest
import torch

from tests import _viz_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = list(V.CASES)
TOL_IMAGE = 2.0 ** -22


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")


def _geo(name):
    n, h, w, nrow, padding, pad_value = V.CASES[name]
    return dict(nrow=nrow, padding=padding, pad_value=pad_value)


def _eq(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (f"{what}: {len(bad)} of {want.size} bytes differ, first at "
                          f"{bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("name", CASES)
def test_out_x_alone_and_the_pair_from_one_launch(name):
    from monocular_depth_estimation_amd import functional as F
    geo = _geo(name)
    x = V.maps(name, 0, edges=V.edge_vector())
    y = V.maps(name, 1, lo=0.0, hi=V.VMAX, edges=V.edge_vector())
    want_x, want_d = V.colorize_grid(x, y, **geo)
    n, h, w = x.shape
    assert want_x.shape == (3,) + V.grid_shape(n, h, w, geo["nrow"], geo["padding"])
    _eq(F.colorize_grid(_dev(x), **geo), want_x, "out_x alone")
    _eq(F.colorize_grid(_dev(x)[:, None], **geo), want_x, "[n, 1, h, w] input")
    gx, gd = F.colorize_grid(_dev(x), y=_dev(y), want=("x", "diff"), **geo)
    _eq(gx, want_x, "out_x of the pair")
    _eq(gd, want_d, "out_diff of the pair")
    _eq(F.colorize_grid(_dev(x), y=_dev(y), want="diff", **geo), want_d, "out_diff alone")
    for cmap in ("viridis", "Reds"):
        _eq(F.colorize_grid(_dev(x), cmap=cmap, **geo), V.colorize_grid(x, cmap=cmap, **geo)[0], cmap)


@pytest.mark.parametrize("name", CASES)
def test_pair_with_xnorm_is_depth_norm_then_the_plain_path(name):
    """DepthNorm applied on load: equal to the oracle, and to depth_norm (the training
    path's own kernel) followed by the plain launch.  The maps are normalised to [0, 1],
    so the range is (0, 1) here; LogProgress keeps the reference's (10, 1000)."""
    from monocular_depth_estimation_amd import functional as F
    geo = _geo(name)
    geo["pad_value"] = 0.25 if geo["pad_value"] else 0.0
    x = V.maps(name, 2, edges=V.edge_vector(specials=False))
    y = V.maps(name, 3, lo=-0.25, hi=1.25, edges=V.unit_edge_vector())
    kw = dict(vmin=0.0, vmax=1.0, **geo)
    want_x, want_d = V.colorize_grid(x, y, xnorm=True, **kw)
    assert len(np.unique(want_x.reshape(3, -1), axis=1).T) > 8      # not one flat colour
    dx, dy = _dev(x), _dev(y)
    mm = F.minmax(dx)
    gx, gd = F.colorize_grid(dx, y=dy, xnorm=mm, want=("x", "diff"), **kw)
    _eq(gx, want_x, "xnorm out_x")
    _eq(gd, want_d, "xnorm out_diff")
    px, pd = F.colorize_grid(F.depth_norm(dx), y=dy, want=("x", "diff"), **kw)
    assert torch.equal(px, gx) and torch.equal(pd, gd)
    # the automatic range of the normalised map: its ends are exactly 0 and 1
    _eq(F.colorize_grid(dx, xnorm=mm, vmin=None, vmax=None, **geo),
        V.colorize_grid(x, xnorm=True, vmin=None, vmax=None, **geo)[0], "xnorm auto range")


@pytest.mark.parametrize("name", CASES)
def test_auto_range_and_flat_range(name):
    """vmin / vmax None: the minimum / maximum of the GRID (pad pixels included), each
    end alone and both; then vmin == vmax, where the value is multiplied by zero."""
    from monocular_depth_estimation_amd import functional as F
    geo = _geo(name)
    x = V.maps(name, 4, lo=20.0, hi=900.0, edges=V.edge_vector(specials=False))
    for vmin, vmax in ((None, None), (None, 700.0), (35.5, None)):
        want = V.colorize_grid(x, vmin=vmin, vmax=vmax, **geo)[0]
        _eq(F.colorize_grid(_dev(x), vmin=vmin, vmax=vmax, **geo), want, f"auto {vmin} {vmax}")
    # values below the pad value too: the pad no longer sets the minimum
    x2 = x - np.float32(600.0)
    _eq(F.colorize_grid(_dev(x2), vmin=None, vmax=None, **geo),
        V.colorize_grid(x2, vmin=None, vmax=None, **geo)[0], "auto, negative values")
    xs = V.maps(name, 5, edges=V.edge_vector())             # NaN and the infinities included
    y = V.maps(name, 6, lo=0.0, hi=V.VMAX)
    want_x, want_d = V.colorize_grid(xs, y, vmin=500.0, vmax=500.0, **geo)
    gx, gd = F.colorize_grid(_dev(xs), y=_dev(y), vmin=500.0, vmax=500.0, want=("x", "diff"), **geo)
    _eq(gx, want_x, "vmin == vmax, out_x")
    _eq(gd, want_d, "vmin == vmax, out_diff")
    const = np.full_like(x, 3.0)                            # an automatic range that is flat
    geo0 = dict(geo, pad_value=3.0)
    _eq(F.colorize_grid(_dev(const), vmin=None, vmax=None, **geo0),
        V.colorize_grid(const, vmin=None, vmax=None, **geo0)[0], "flat auto range")


@pytest.mark.parametrize("name", ["two_rows", "coloured_pad", "squeeze"])
def test_unaligned_outputs(name):
    """Outputs at every byte alignment (the planes' word grids shift with it): equal to
    the aligned result, and not a byte outside the output is touched."""
    from monocular_depth_estimation_amd import functional as F
    geo = _geo(name)
    x = V.maps(name, 7, edges=V.edge_vector())
    y = V.maps(name, 8, lo=0.0, hi=V.VMAX)
    want_x, want_d = V.colorize_grid(x, y, **geo)
    size = want_x.size
    for off in (1, 2, 3):
        bufs = [torch.full((size + 64,), 0x5A, dtype=torch.uint8, device=DEV) for _ in range(2)]
        outs = [b[16 + off + o:16 + off + o + size].view(want_x.shape) for o, b in enumerate(bufs)]
        F.colorize_grid(_dev(x), y=_dev(y), want=("x", "diff"), out=outs, **geo)
        _eq(outs[0], want_x, f"out_x at +{off}")
        _eq(outs[1], want_d, f"out_diff at +{off + 1}")
        for o, b in enumerate(bufs):
            lo = 16 + off + o
            assert bool((b[:lo] == 0x5A).all()) and bool((b[lo + size:] == 0x5A).all())


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("c", [1, 3])
def test_image_grid(name, c):
    from monocular_depth_estimation_amd import functional as F
    geo = _geo(name)
    x = V.images(name, c)
    want = V.image_grid(x, **geo)
    got = F.image_grid(_dev(x), **geo).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    err = float(np.abs(got - want).max())
    print(f"{name} c={c}: max |got - oracle| = {err:.3e} = {err / 2.0 ** -23:.2f} x 2^-23")
    assert err <= TOL_IMAGE
    assert got.min() == 0.0 or geo["pad_value"] < 0
    if name == "two_rows":  # a float4-misaligned output, and a constant image (the 1e-5 floor)
        n, h, w = x.shape[0], x.shape[2], x.shape[3]
        for off in (1, 2, 3):
            buf = torch.full((want.size + 16,), 7.0, device=DEV)
            out = buf[off:off + want.size].view(want.shape)
            F.image_grid(_dev(x), out=out, **geo)
            assert float(np.abs(out.cpu().numpy() - want).max()) <= TOL_IMAGE
            assert bool((buf[:off] == 7.0).all()) and bool((buf[off + want.size:] == 7.0).all())
        const = np.full((n, c, h, w), 2.5, np.float32)
        got = F.image_grid(_dev(const), **geo).cpu().numpy()
        np.testing.assert_array_equal(got, V.image_grid(const, **geo))
        assert got.max() == 0.0


def test_utils_colorize_on_a_device_tensor():
    from monocular_depth_estimation_amd.utils import colorize
    x = V.maps("blocks", 9, edges=V.edge_vector())          # [3, 70, 130] as [C, H, W]
    got = colorize(_dev(x))
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, V.colorize(x[0]))
    xf = np.nan_to_num(x, nan=1.0, posinf=2.0, neginf=3.0)
    np.testing.assert_array_equal(colorize(_dev(xf), None, None, "viridis"),
                                  V.colorize(xf[0], None, None, "viridis"))
    np.testing.assert_array_equal(colorize(_dev(xf)), colorize(torch.from_numpy(xf)))


def test_guard_harness_and_refusals():
    """Both launching entries on relocated, guard-banded buffers, run twice from poisoned
    outputs (tests/_abi_guard.py): no write outside a buffer, every output byte written,
    results equal to the plain run.  Refused calls launch nothing."""
    from monocular_depth_estimation_amd import _abi
    from monocular_depth_estimation_amd import functional as F
    from tests._abi_guard import guarded_abi, launching_entries
    assert launching_entries(_abi.VIZ_SIGNATURES) == {"mde_viz_colorize_grid", "mde_viz_image_grid"}
    sig = {**_abi.SIGNATURES, **_abi.VIZ_SIGNATURES}
    for name in ("two_rows", "coloured_pad", "squeeze"):
        geo = _geo(name)
        x, y = _dev(V.maps(name, 0, edges=V.edge_vector())), _dev(V.maps(name, 1, lo=0.0, hi=V.VMAX))
        im = _dev(V.images(name, 3))
        plain = F.colorize_grid(x, y=y, want=("x", "diff"), **geo)
        mm = F.minmax(x)
        plain_n = F.colorize_grid(x, y=y, xnorm=mm, vmin=0.0, vmax=1.0, want=("x", "diff"), **geo)
        plain_i = F.image_grid(im, **geo)
        with guarded_abi(signatures=sig) as guard:
            g = F.colorize_grid(x, y=y, want=("x", "diff"), **geo)
            gn = F.colorize_grid(x, y=y, xnorm=F.minmax(x), vmin=0.0, vmax=1.0, want=("x", "diff"),
                                 **geo)
            g1 = F.colorize_grid(x, **geo)
            gi = F.image_grid(im, **geo)
        assert guard.calls["mde_viz_colorize_grid"] == 3 and guard.calls["mde_viz_image_grid"] == 1
        assert all(torch.equal(a, b) for a, b in zip(g + gn, plain + plain_n))
        assert torch.equal(g1, plain[0]) and torch.equal(gi, plain_i)
    with guarded_abi(signatures=sig) as guard:
        with pytest.raises(ValueError, match="automatic range"):
            F.colorize_grid(x, y=y, vmax=None, want=("x", "diff"))
        with pytest.raises(ValueError, match="needs y"):
            F.colorize_grid(x, want=("diff",))
        with pytest.raises(ValueError):
            F.colorize_grid(x, cmap="jet")
        with pytest.raises(ValueError):
            F.colorize_grid(x, y=y[:, :, :-1], want=("x", "diff"))
        with pytest.raises(ValueError):
            F.colorize_grid(x, out=torch.empty(3, 4, 4, dtype=torch.uint8, device=DEV))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            F.colorize_grid(x.cpu())
        with pytest.raises(ValueError):
            F.image_grid(im[:, :2])
        with pytest.raises(TypeError):
            F.image_grid(im.double())
        with pytest.raises(_abi.MdeError):
            F.colorize_grid(x, nrow=0)
    assert not guard.calls, guard.calls


def test_graph_replay():
    """One capture of colorize_grid(..., out=static) on one stream, replayed after the
    inputs changed in place: the replay's pictures are the oracle's of the new inputs."""
    from monocular_depth_estimation_amd import _abi
    from monocular_depth_estimation_amd import functional as F
    name = "two_rows"
    geo = _geo(name)
    x0, y0 = V.maps(name, 10, edges=V.edge_vector()), V.maps(name, 11, lo=0.0, hi=V.VMAX)
    x1, y1 = V.maps(name, 12, edges=V.edge_vector()), V.maps(name, 13, lo=0.0, hi=V.VMAX)
    sx, sy = _dev(x0), _dev(y0)
    shape = (3,) + V.grid_shape(*x0.shape, geo["nrow"], geo["padding"])
    outs = [torch.zeros(shape, dtype=torch.uint8, device=DEV) for _ in range(2)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def run():
        F.colorize_grid(sx, y=sy, want=("x", "diff"), out=outs, **geo)

    with torch.cuda.stream(s):
        run()
    torch.cuda.synchronize()
    g, _, _ = _abi.capture_graph(run, s)
    assert g.node_counts["kernel"] == 1 and g.node_counts["total"] == 1
    for xs, ys in ((x1, y1), (x0, y0)):
        sx.copy_(_dev(xs))
        sy.copy_(_dev(ys))
        for o in outs:
            o.fill_(0x5A)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_x, want_d = V.colorize_grid(xs, ys, **geo)
        _eq(outs[0], want_x, "replayed out_x")
        _eq(outs[1], want_d, "replayed out_diff")
    g.reset()


# ---------------------------------------------------------------- LogProgress
class _StubWriter:
    def __init__(self):
        self.images = []

    def add_image(self, tag, img, step):
        self.images.append((tag, np.array(img), step))


@pytest.fixture(scope="module")
def logged():
    """A GuideDepth at 64 x 96 with the oracle's deterministic weights, one batch of 7,
    LogProgress at epoch 0 and at epoch 5."""
    import monocular_depth_estimation_amd as mde
    from monocular_depth_estimation_amd.train import LogProgress, synthetic_batch
    from oracle.weights import fill_
    model = fill_(mde.GuideDepth(pretrained=False)).to(DEV).train()
    image, depth = synthetic_batch(7, 64, 96, 0, 3, torch.device(DEV))
    loader = [{"image": image.cpu(), "depth": depth}]       # a host image, a device depth
    w0, w5 = _StubWriter(), _StubWriter()
    LogProgress(model, w0, loader, 0)
    mode_after = model.training
    LogProgress(model, w5, loader, 5)
    with torch.no_grad():
        pred = model(image)
    return dict(model=model, image=image, depth=depth, pred=pred, w0=w0, w5=w5,
                mode_after=mode_after)


def test_log_progress_tags_order_shapes_and_mode(logged):
    assert [(t, s) for t, _, s in logged["w0"].images] == [
        ("Train.1.Image", 0), ("Train.2.Depth", 0), ("Train.3.Ours", 0), ("Train.3.Diff", 0)]
    assert [(t, s) for t, _, s in logged["w5"].images] == [("Train.3.Ours", 5), ("Train.3.Diff", 5)]
    shape = (3, 2 * 66 + 2, 6 * 98 + 2)
    for tag, img, _ in logged["w0"].images + logged["w5"].images:
        assert img.shape == shape, (tag, img.shape)
        assert img.dtype == (np.float32 if tag == "Train.1.Image" else np.uint8), tag
    assert logged["mode_after"] is False and logged["model"].training is False  # left in eval mode
    assert logged["pred"].shape == (7, 1, 64, 96)


def test_log_progress_pictures_are_the_oracles(logged):
    """Ours / Diff: the oracle on the GPU model's own prediction; Depth and Image: the
    oracle on the batch.  (With the reference's range (10, 1000) a DepthNorm'ed map is
    below vmin everywhere: the reference logs one flat colour, and so does this.)"""
    pred = logged["pred"][:, 0].cpu().numpy()
    depth = logged["depth"][:, 0].cpu().numpy()
    want_x, want_d = V.colorize_grid(pred, depth, xnorm=True, nrow=6)
    for w in (logged["w0"], logged["w5"]):
        pics = {t: img for t, img, _ in w.images}
        np.testing.assert_array_equal(pics["Train.3.Ours"], want_x)
        np.testing.assert_array_equal(pics["Train.3.Diff"], want_d)
    pics = {t: img for t, img, _ in logged["w0"].images}
    np.testing.assert_array_equal(pics["Train.2.Depth"], V.colorize_grid(depth, nrow=6)[0])
    want_i = V.image_grid(logged["image"].cpu().numpy(), nrow=6)
    err = float(np.abs(pics["Train.1.Image"] - want_i).max())
    print(f"Train.1.Image: max |got - oracle| = {err:.3e}")
    assert err <= TOL_IMAGE
    # the same launch with a range that shows the prediction: still the oracle's bytes
    from monocular_depth_estimation_amd import functional as F
    gx, gd = F.colorize_grid(logged["pred"], y=logged["depth"], xnorm=F.minmax(logged["pred"]),
                             vmin=0.0, vmax=1.0, nrow=6, want=("x", "diff"))
    ox, od = V.colorize_grid(pred, depth, xnorm=True, vmin=0.0, vmax=1.0, nrow=6)
    _eq(gx, ox, "Ours in (0, 1)")
    _eq(gd, od, "Diff in (0, 1)")
    assert len(np.unique(ox.reshape(3, -1), axis=1).T) > 8


def test_train_cli_writes_the_pictures(tmp_path):
    """--log-images: step 0 of epoch 0 logs the four pictures (niter 0), the end of the
    epoch logs Ours / Diff again at niter 1; PPM files of the grid's size."""
    from monocular_depth_estimation_amd.train import main
    pics = tmp_path / "pics"
    main(["--epochs", "1", "--steps-per-epoch", "2", "--bs", "2", "--height", "64", "--width", "96",
          "--log-images", str(pics), "--checkpoint", str(tmp_path / "ckpt.pth")])
    names = sorted(p.name for p in pics.iterdir())
    assert names == sorted(["Train.1.Image_0.ppm", "Train.2.Depth_0.ppm", "Train.3.Ours_0.ppm",
                            "Train.3.Diff_0.ppm", "Train.3.Ours_1.ppm", "Train.3.Diff_1.ppm"])
    hg, wg = V.grid_shape(2, 64, 96, 6, 2)
    head = b"P6\n%d %d\n255\n" % (wg, hg)
    for n in names:
        raw = (pics / n).read_bytes()
        assert raw.startswith(head) and len(raw) == len(head) + 3 * hg * wg, n
