"""mde_infer_prep / mde_infer_depth (functional.infer_prep, depth_from_inverse) against
the compositions of the package's own ops they replace, bit for bit.

infer_prep: F.bilinear_resize(cat([img, flip(img, [3])]), size) of the float image;
for uint8 frames the float image is torchvision's to_tensor,
byte.permute(0, 3, 1, 2).float().div(255), taken ON THE HOST as to_tensor takes it
(a true division; ATen's device kernel for a division by a host scalar multiplies
by the rounded reciprocal instead, which differs in the last bit).  Every case here
is one at which bilinear_resize runs its generic kernel.

depth_from_inverse: F.bilinear_resize(inverse_depth_norm(inv), size) at generic
ratios.  At the exact x2 ratio bilinear_resize takes a kernel with another
rounding order, so the yardstick there is the float64 interpolation of the fp32
depths D, with the bound 4 * 2^-24 * max_depth: each lerp2 = fma(l1, b, fl(l0 a))
rounds twice, each rounding is at most half an ulp (2^-24 relative) of a value
<= max_depth, the interpolation has two levels and the second level carries
the first level's error through weights that sum to 1; the x2 weights 1/4 and
3/4 are exact.  A numpy emulation of the kernel's arithmetic measured at most
0.85 * 2^-24 * max_depth at these shapes (1.25 at 32 x 48 -> 64 x 96) before the
first GPU run.  The identity with
evalpair.hip at x2 is checked through the integer sums of eval_pair_sums.
"""
import functools

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name: (n, H, W, h, w)
PREP_CASES = {
    "generic": (3, 13, 18, 5, 7),
    "exact_half": (1, 12, 16, 6, 8),
    "identity": (3, 5, 7, 5, 7),
    "upscale": (1, 5, 7, 13, 18),
    "row_wider_than_block": (3, 3, 600, 2, 300),
    "more_frames_than_blocks": (70000, 3, 3, 2, 2),   # 70000 blocks of work, 65536 launched
}
# name: (n, ph, pw, H, W, planted NaN)
DEPTH_CASES = {
    "generic": (3, 5, 7, 13, 18, True),
    "generic_2": (1, 6, 8, 15, 20, True),
    "identity": (3, 5, 7, 5, 7, True),
    "x2": (3, 5, 7, 10, 14, False),
    "x2_2": (1, 6, 8, 12, 16, False),
}
MAXDS = (10.0, 80.0)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")


# ----------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def _frames(name):
    """Seeded uint8 [n, H, W, 3] on the host: random over 0..255, 0 and 255 forced into
    the four corners and the last column."""
    n, H, W, _, _ = PREP_CASES[name]
    gen = torch.Generator().manual_seed(2000 + sorted(PREP_CASES).index(name))
    f = torch.randint(0, 256, (n, H, W, 3), generator=gen, dtype=torch.uint8)
    f[:, :, W - 1, :] = torch.tensor([0, 255, 0], dtype=torch.uint8)
    f[:, 0, 0, :] = torch.tensor([0, 255, 255], dtype=torch.uint8)
    f[:, 0, W - 1, :] = torch.tensor([255, 0, 255], dtype=torch.uint8)
    f[:, H - 1, 0, :] = torch.tensor([255, 255, 0], dtype=torch.uint8)
    f[:, H - 1, W - 1, :] = torch.tensor([0, 0, 255], dtype=torch.uint8)
    return f


def _to_tensor(frames):
    """torchvision's to_tensor for a batch of HWC uint8 frames (host arithmetic)."""
    assert not frames.is_cuda
    return frames.permute(0, 3, 1, 2).float().div(255).contiguous()


@functools.lru_cache(maxsize=None)
def _prep_reference(name):
    """bilinear_resize(cat([img, flip(img)])) of the case, computed once (device tensor)."""
    from monocular_depth_estimation_amd.functional import bilinear_resize
    _, _, _, h, w = PREP_CASES[name]
    img = _to_tensor(_frames(name)).to(DEV)
    return bilinear_resize(torch.cat([img, torch.flip(img, [3])]), size=(h, w))


@functools.lru_cache(maxsize=None)
def _inv(name, maxd):
    """Seeded inv [n, 1, ph, pw] on the host, uniform in [0.3, 40], with a 0, a negative
    value, 1e-30, 1e30 and (where the case says so) a NaN planted in every map."""
    n, ph, pw, _, _, nan = DEPTH_CASES[name]
    gen = torch.Generator().manual_seed(3000 + 10 * sorted(DEPTH_CASES).index(name) + int(maxd))
    inv = 0.3 + 39.7 * torch.rand((n, 1, ph, pw), generator=gen)
    flat = inv.view(n, -1)
    m = flat.shape[1]
    flat[:, 1] = 0.0
    flat[:, m // 3] = -0.7
    flat[:, m // 2] = 1e-30
    flat[:, (2 * m) // 3] = 1e30
    if nan:
        flat[:, m - 2 * pw - 3] = float("nan")
    return inv


def _inverse_depth_norm(inv, maxd):
    from monocular_depth_estimation_amd.GuideDepth.evaluate import Evaluater
    ev = Evaluater.__new__(Evaluater)
    ev.maxDepth = maxd
    return ev.inverse_depth_norm(inv)


def _same_bits(a, b):
    """torch.equal with NaNs in the same places counted as equal."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def _run_prep(name, layout, views):
    from monocular_depth_estimation_amd.functional import infer_prep
    _, _, _, h, w = PREP_CASES[name]
    frames = _frames(name)
    src = frames.to(DEV) if layout == 0 else _to_tensor(frames).to(DEV)
    return infer_prep(src, (h, w), views=views)


def _run_depth(name, maxd, out=None):
    from monocular_depth_estimation_amd.functional import depth_from_inverse
    _, _, _, H, W, _ = DEPTH_CASES[name]
    return depth_from_inverse(_inv(name, maxd).to(DEV), (H, W), maxd, out=out)


# ------------------------------------------------------------------ infer_prep
@pytest.mark.parametrize("views", (1, 2))
@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("name", list(PREP_CASES))
def test_prep_is_the_resize_of_image_and_flip(name, layout, views):
    n, _, _, h, w = PREP_CASES[name]
    want = _prep_reference(name)
    got = _run_prep(name, layout, views)
    assert got.shape == (views * n, 3, h, w) and got.dtype == torch.float32
    assert torch.equal(got[:n], want[:n]), (got[:n] - want[:n]).abs().max()
    if views == 2:
        assert torch.equal(got[n:], want[n:]), (got[n:] - want[n:]).abs().max()


def test_prep_view_1_is_the_resize_of_the_flipped_frame():
    """An asymmetric ramp at an odd generic ratio: view 1 == resize(flip(x)).  Whether that
    differs from flip(resize(x)) in some last bit on this input is printed, not required."""
    from monocular_depth_estimation_amd.functional import bilinear_resize, infer_prep
    H, W, h, w = 13, 18, 5, 7
    ramp = (torch.arange(W, dtype=torch.float32) / W) ** 1.7
    rows = 1.0 - 0.03 * torch.arange(H, dtype=torch.float32)
    x = (rows[:, None] * ramp[None, :]).expand(2, 3, H, W).contiguous().to(DEV)
    got = infer_prep(x, (h, w), views=2)
    fl = bilinear_resize(torch.flip(x, [3]), size=(h, w))
    assert torch.equal(got[2:], fl)
    assert torch.equal(got[:2], bilinear_resize(x, size=(h, w)))
    print("resize(flip(x)) == flip(resize(x)) bit for bit:",
          bool(torch.equal(fl, torch.flip(got[:2], [3]))))
    assert not torch.equal(fl, got[:2])        # the ramp is asymmetric


def test_prep_writes_into_out_and_takes_one_frame():
    from monocular_depth_estimation_amd.functional import infer_prep
    name = "generic"
    n, _, _, h, w = PREP_CASES[name]
    want = _prep_reference(name)
    big = torch.full((2 * n + 2, 3, h, w), -1.0, device=DEV)
    r = infer_prep(_frames(name).to(DEV), (h, w), views=2, out=big[1:2 * n + 1])
    assert r.data_ptr() == big[1].data_ptr()
    assert torch.equal(big[1:2 * n + 1], want)
    assert bool((big[0] == -1).all()) and bool((big[-1] == -1).all())
    one = infer_prep(_frames(name)[0].to(DEV), (h, w), views=2)   # [H, W, 3]
    assert torch.equal(one[0], want[0]) and torch.equal(one[1], want[n])
    with pytest.raises(ValueError):
        infer_prep(_frames(name).to(DEV), (h, w), views=2, out=big[:2 * n, :, :, :w - 1])
    with pytest.raises(TypeError):
        infer_prep(_frames(name).to(DEV).to(torch.int32), (h, w))


# ---------------------------------------------------------- depth_from_inverse
@pytest.mark.parametrize("maxd", MAXDS)
@pytest.mark.parametrize("name", ["generic", "generic_2"])
def test_depth_generic_is_resize_of_inverse_depth_norm(name, maxd):
    from monocular_depth_estimation_amd.functional import bilinear_resize
    n, _, _, H, W, _ = DEPTH_CASES[name]
    inv = _inv(name, maxd).to(DEV)
    want = bilinear_resize(_inverse_depth_norm(inv, maxd), size=(H, W))
    got = _run_depth(name, maxd)
    assert got.shape == (n, 1, H, W)
    assert int(torch.isnan(want).sum()) >= n             # the planted NaN reaches the map
    assert _same_bits(got, want)


@pytest.mark.parametrize("maxd", MAXDS)
def test_depth_identity_is_inverse_depth_norm(maxd):
    inv = _inv("identity", maxd).to(DEV)
    want = _inverse_depth_norm(inv, maxd)
    got = _run_depth("identity", maxd)
    assert _same_bits(got, want)
    n = inv.shape[0]
    assert int(torch.isnan(got).sum()) == n              # the NaN stays where it is
    d = got.cpu().view(n, -1)
    m = d.shape[1]
    assert d[:, 1].tolist() == [maxd] * n                 # 0 -> max_depth
    lo = float(torch.tensor(maxd / 100, dtype=torch.float32))
    assert d[:, m // 3].tolist() == [lo] * n              # negative -> max_depth / 100
    assert d[:, m // 2].tolist() == [maxd] * n            # 1e-30
    assert d[:, (2 * m) // 3].tolist() == [lo] * n        # 1e30
    # a 3-D map comes back 3-D
    from monocular_depth_estimation_amd.functional import depth_from_inverse
    assert _same_bits(depth_from_inverse(inv[:, 0], (5, 7), maxd), want[:, 0])


@pytest.mark.parametrize("maxd", MAXDS)
@pytest.mark.parametrize("name", ["x2", "x2_2"])
def test_depth_x2_within_the_rounding_bound(name, maxd):
    _, _, _, H, W, _ = DEPTH_CASES[name]
    inv = _inv(name, maxd)
    d32 = _inverse_depth_norm(inv.to(DEV), maxd).cpu()    # the fp32 depths D
    want = TF.interpolate(d32.double(), size=(H, W), mode="bilinear", align_corners=False)
    got = _run_depth(name, maxd).cpu().double()
    err = float((got - want).abs().max())
    bound = 4 * 2.0 ** -24 * maxd
    print(f"{name} max_depth {maxd}: max error {err:.3e} = {err / (2.0 ** -24 * maxd):.2f} "
          f"x 2^-24 max_depth (bound 4)")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("name", ["x2", "x2_2"])
def test_depth_x2_is_the_prediction_evalpair_compares(name):
    """Sums 0-3 (count and the three threshold counts) of eval_pair_sums' view 0 against
    eval_sums of the written map: integers, and both kernels form max(g / p, p / g)
    the same way, so any difference is a difference in p."""
    from monocular_depth_estimation_amd.functional import eval_pair_sums, eval_sums
    maxd = 10.0
    n, _, _, H, W, _ = DEPTH_CASES[name]
    gen = torch.Generator().manual_seed(4000 + H)
    gt = (0.5 + 9.0 * torch.rand((n, 1, H, W), generator=gen)).to(DEV)
    inv = _inv(name, maxd).to(DEV)
    pair = eval_pair_sums(inv, None, gt, maxd, None)[:, 0, :4].sum(0).cpu()
    depth = _run_depth(name, maxd)
    mine = eval_sums(depth, gt)[:4].cpu()
    assert pair[0] == n * H * W
    assert 0 < pair[1] < pair[3] <= pair[0]               # the thresholds discriminate
    assert torch.equal(pair, mine), (pair, mine)


def test_depth_writes_into_out():
    name, maxd = "generic", 10.0
    n, _, _, H, W, _ = DEPTH_CASES[name]
    plain = _run_depth(name, maxd)
    big = torch.full((n + 2, 1, H, W), -1.0, device=DEV)
    r = _run_depth(name, maxd, out=big[1:n + 1])
    assert r.data_ptr() == big[1].data_ptr()
    assert _same_bits(big[1:n + 1], plain)
    assert bool((big[0] == -1).all()) and bool((big[-1] == -1).all())


# ------------------------------------------------------------------ under guard
def _guarded():
    from monocular_depth_estimation_amd import _abi
    from tests._abi_guard import guarded_abi
    return guarded_abi(signatures={**_abi.SIGNATURES, **_abi.EVAL_SIGNATURES,
                                   **_abi.INFER_SIGNATURES})


@pytest.mark.parametrize("name", list(PREP_CASES))
def test_prep_under_guard(name):
    """Guard bands and poisoned outputs (tests/_abi_guard.py) around the entry: nothing
    written outside a buffer, every output element written; results equal the plain run."""
    for layout in (0, 1):
        plain = _run_prep(name, layout, 2)
        with _guarded() as guard:
            got = _run_prep(name, layout, 2)
            got1 = _run_prep(name, layout, 1)
        assert guard.calls["mde_infer_prep"] == 2
        assert torch.equal(got, plain)
        assert torch.equal(got1, plain[:plain.shape[0] // 2])


@pytest.mark.parametrize("name", list(DEPTH_CASES))
def test_depth_under_guard(name):
    for maxd in MAXDS:
        plain = _run_depth(name, maxd)
        with _guarded() as guard:
            got = _run_depth(name, maxd)
        assert guard.calls["mde_infer_depth"] == 1
        assert _same_bits(got, plain)
