"""mde_eval_pair_sums (functional.eval_pair_sums) against a float64 oracle written here
from the reference's evaluation loop (src/GuideDepth/evaluate.py:93-142: flip,
inverse_depth_norm, upscale, crop; src/GuideDepth/metrics.py:41-62: the terms).

Counts (sums 0-3) must equal the oracle's exactly: the inputs are built so that
no selected pixel's max(g/p, p/g) lies within relative 1e-5 of a threshold
(asserted on the CPU first), two orders above the ~1e-6 fp32 interpolation
error.  For sums 4-13 the error against the oracle is measured for the fused
entry (e_new) and for the unfused composition of the existing ops on the same
inputs (e_old: maxd / x, clamp, bilinear_resize, crop, eval_sums per image and
view, torch.flip for gt), and e_new <= 2 e_old + 1e-9 sum|term| is required:
the factor 2 allows an equally valid but different rounding order, the last
term covers the double-reordering bound N 2^-53 sum|term| at N <= 2^20.  The
error of a sum is the largest over the case's (image, view) rows, for both
sides: where the two paths round differently (the exact x2 resize kernels, the
logarithms) their errors on one row of a few dozen pixels are independent draws,
either of which can fall near zero, and a factor between two such draws says
nothing; the largest of the rows is the error a user of the sums can meet.
Measured at the NYU geometry (2 x 480 x 640, MI355X), e_old -> e_new:
sum (g-p)^2 8.2e-4 -> 1.0e-3 of 1.7e6, sum |log10 p - log10 g| 2.2e-3 -> 1.9e-5
of 6.3e4, sum (ln p - ln g) 3.5e-3 -> 9.1e-5 of 1.4e5 (the fused kernel rounds
its logarithms correctly; logf / log10f of the device library carry a relative
bias of about 3e-8 that a sum of a quarter of a million terms keeps).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAXD = 10.0
NYU_CROP = (20, 460, 24, 616)

# name: (ph, pw, H, W, n, crop, with_flip)
CASES = {
    "odd_ratio_asym_crop": (5, 7, 13, 18, 3, (2, 11, 3, 16), True),
    "wide_x2_one_axis": (4, 150, 9, 300, 2, (0, 9, 1, 300), True),
    "identity_no_crop": (6, 10, 6, 10, 2, None, True),
    "no_flip": (8, 8, 16, 16, 1, None, False),
    "empty_crop": (5, 7, 13, 18, 1, (4, 4, 0, 18), True),
    "nyu_half": (240, 320, 480, 640, 2, NYU_CROP, True),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")


# ----------------------------------------------------------------- the oracle
def _depth64(inv):
    """inverse_depth_norm (evaluate.py:174-177) in float64."""
    return torch.clamp(MAXD / inv.double(), MAXD / 100, MAXD)


def _views64(inv, inv_flip, gt, crop):
    """[(p, g)] float64 per view, p / g [n, h', w'] after upscale and crop
    (evaluate.py:94,113-116,129-132)."""
    H, W = gt.shape[-2:]
    c = crop if crop is not None else (0, H, 0, W)
    out = []
    for v, g in ((inv, gt.double()), (inv_flip, torch.flip(gt, [2]).double())):
        if v is None:
            out.append(None)
            continue
        p = TF.interpolate(_depth64(v)[:, None], size=(H, W), mode="bilinear",
                           align_corners=False)[:, 0]
        out.append((p[:, c[0]:c[1], c[2]:c[3]], g[:, c[0]:c[1], c[2]:c[3]]))
    return out


def _theta(p, g):
    return torch.maximum(g / p, p / g)


def _terms64(p, g):
    """The 14 per-pixel terms of the sums (metrics.py:41-62; layout of metrics.hip)."""
    th = _theta(p, g)
    d = g - p
    ln = torch.log(p) - torch.log(g)
    l10 = torch.log10(p) - torch.log10(g)
    ip = 1.0 / p - 1.0 / g
    return [torch.ones_like(p), (th < 1.25).double(), (th < 1.25 ** 2).double(),
            (th < 1.25 ** 3).double(), d * d, ln * ln, d.abs() / g, d * d / g, ln, l10.abs(),
            d.abs(), l10 * l10, ip.abs(), ip * ip]


def _oracle(inv, inv_flip, gt, crop):
    """(sums [n, 2, 16], sum|term| [n, 2, 16]) in float64."""
    n = gt.shape[0]
    s = torch.zeros((n, 2, 16), dtype=torch.float64)
    a = torch.zeros((n, 2, 16), dtype=torch.float64)
    for v, pg in enumerate(_views64(inv, inv_flip, gt, crop)):
        if pg is None:
            continue
        for k, t in enumerate(_terms64(*pg)):
            s[:, v, k] = t.flatten(1).sum(1)
            a[:, v, k] = t.abs().flatten(1).sum(1)
    return s, a


def _margin(inv, inv_flip, gt, crop):
    """Smallest relative distance of a selected pixel's max(g/p, p/g) to a threshold,
    and the [n, H, W] mask (gt coordinates) of the pixels closer than 1e-5."""
    H, W = gt.shape[-2:]
    c = crop if crop is not None else (0, H, 0, W)
    bad = torch.zeros(gt.shape, dtype=torch.bool)
    best = math.inf
    for v, pg in enumerate(_views64(inv, inv_flip, gt, crop)):
        if pg is None or pg[0].numel() == 0:
            continue
        th = _theta(*pg)
        near = torch.zeros(th.shape, dtype=torch.bool)
        for k in (1, 2, 3):
            rel = (th / 1.25 ** k - 1.0).abs()
            rel = torch.where(torch.isnan(rel), torch.full_like(rel, math.inf), rel)
            best = min(best, float(rel.min()))
            near |= rel < 1e-5
        full = torch.zeros(gt.shape, dtype=torch.bool)
        full[:, c[0]:c[1], c[2]:c[3]] = near
        bad |= torch.flip(full, [2]) if v == 1 else full
    return best, bad


# ----------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Seeded (inv, inv_flip, gt) on the CPU: gt uniform in [0.3, 9.8]; the predictions
    are MAXD / (area-downsample of gt x lognormal noise, sigma 0.2), so the delta
    fractions are mid-range; a 0, a negative value and a value below 1 (depth
    clamped to MAXD) are planted in inv.  Ground-truth pixels whose theta lies
    within 1e-5 of a threshold are nudged by 0.3 % until none does."""
    ph, pw, H, W, n, crop, with_flip = CASES[name]
    gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    gt = 0.3 + 9.5 * torch.rand((n, H, W), generator=gen)

    def pred(src):
        small = TF.adaptive_avg_pool2d(src[:, None], (ph, pw))[:, 0]
        return MAXD / (small * torch.exp(0.2 * torch.randn((n, ph, pw), generator=gen)))

    inv = pred(gt)
    inv_flip = pred(torch.flip(gt, [2])) if with_flip else None
    flat = inv.view(-1)
    m = flat.numel()
    flat[m // 3] = 0.0
    flat[m // 2] = -0.7
    flat[(2 * m) // 3] = 0.25
    for _ in range(20):
        _, bad = _margin(inv, inv_flip, gt, crop)
        if not bool(bad.any()):
            break
        gt = torch.where(bad, gt * 1.003, gt)
    return inv.contiguous(), inv_flip, gt.contiguous()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Oracle sums, sum|term| and the margin of a case, computed once."""
    inv, inv_flip, gt = _inputs(name)
    crop = CASES[name][5]
    s, a = _oracle(inv, inv_flip, gt, crop)
    return s, a, _margin(inv, inv_flip, gt, crop)[0]


def _dev(t):
    return None if t is None else t.to(DEV)


def _fused(name, out=None):
    from monocular_depth_estimation_amd.functional import eval_pair_sums
    inv, inv_flip, gt = _inputs(name)
    return eval_pair_sums(_dev(inv)[:, None], None if inv_flip is None else _dev(inv_flip)[:, None],
                          _dev(gt)[:, None], MAXD, CASES[name][5], out=out)


def _unfused(name):
    """The parent's composition: maxd / x, clamp, bilinear_resize, crop, eval_sums per
    image and view, torch.flip for gt.  [n, 2, 16] float64 on the CPU."""
    from monocular_depth_estimation_amd.functional import bilinear_resize, eval_sums
    inv, inv_flip, gt = _inputs(name)
    H, W = gt.shape[-2:]
    crop = CASES[name][5]
    c = crop if crop is not None else (0, H, 0, W)
    g0 = _dev(gt)[:, None]
    out = torch.zeros((gt.shape[0], 2, 16), dtype=torch.float64)
    for v, (x, g) in enumerate(((inv, g0), (inv_flip, torch.flip(g0, [3])))):
        if x is None:
            continue
        p = torch.clamp(MAXD / _dev(x)[:, None], MAXD / 100, MAXD)
        p = bilinear_resize(p, size=(H, W))
        p, g = p[:, :, c[0]:c[1], c[2]:c[3]], g[:, :, c[0]:c[1], c[2]:c[3]]
        for i in range(gt.shape[0]):
            out[i, v] = eval_sums(p[i:i + 1], g[i:i + 1]).cpu()
    return out


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", list(CASES))
def test_against_float64_oracle(name):
    want, absum, margin = _reference(name)
    print(f"{name}: smallest relative distance of theta to a threshold {margin:.3e}")
    assert margin >= 1e-5, margin            # the input condition, before any GPU call
    got = _fused(name).cpu()
    assert got.shape == want.shape and got.dtype == torch.float64
    old = _unfused(name)
    assert torch.equal(got[..., 14:], torch.zeros_like(got[..., 14:]))
    if not CASES[name][6]:
        assert torch.equal(got[:, 1], torch.zeros_like(got[:, 1]))   # inv_pred_flip=None
    if name == "empty_crop":
        assert torch.equal(got, torch.zeros_like(got))
    assert torch.equal(got[..., :4], want[..., :4]), (got[..., :4], want[..., :4])
    # per sum, the largest error over the case's (image, view) rows
    e_new = (got - want).abs()[..., 4:14].amax((0, 1))
    e_old = (old - want).abs()[..., 4:14].amax((0, 1))
    scale = absum[..., 4:14].amax((0, 1))
    for k in range(10):
        print(f"{name}: sum {k + 4}: e_old {float(e_old[k]):.3e} e_new {float(e_new[k]):.3e} "
              f"sum|term| {float(scale[k]):.3e}")
    bound = 2 * e_old + 1e-9 * scale
    assert bool((e_new <= bound).all()), (e_new - bound).max()


def test_clamp_cases_reach_the_sums():
    """The planted 0 / negative / < 1 samples are in the inputs the oracle comparison
    runs on, so torch.clamp's edge semantics are part of what is compared."""
    inv, _, _ = _inputs("odd_ratio_asym_crop")
    d = _depth64(inv)
    assert int((inv == 0).sum()) == 1 and int((inv < 0).sum()) == 1
    assert float(d[inv == 0]) == MAXD and float(d[inv < 0]) == MAXD / 100
    assert int((d == MAXD).sum()) >= 2


def test_nan_propagates_like_torch_clamp():
    from monocular_depth_estimation_amd.functional import eval_pair_sums
    inv = torch.tensor([[[1.0, 2.0, float("nan"), 4.0, 5.0, 2.5]]])
    gt = torch.tensor([[[9.0, 5.5, 3.0, 2.0, 2.5, 4.5]]])
    assert bool(torch.isnan(torch.clamp(MAXD / inv, MAXD / 100, MAXD)).any())
    got = eval_pair_sums(inv.to(DEV), torch.flip(inv, [2]).to(DEV), gt.to(DEV), MAXD).cpu()
    # same size: the sample itself, so the oracle needs no interpolation
    want = torch.zeros((1, 2, 16), dtype=torch.float64)
    for v, (x, g) in enumerate(((inv, gt), (torch.flip(inv, [2]), torch.flip(gt, [2])))):
        for k, t in enumerate(_terms64(_depth64(x), g.double())):
            want[0, v, k] = t.sum()
    for v in (0, 1):
        assert got[0, v, 0] == 6
        assert torch.equal(got[0, v, 1:4], want[0, v, 1:4])   # NaN < t is False, as in torch
        assert bool(torch.isnan(got[0, v, 4:14]).all()) and bool(torch.isnan(want[0, v, 4:14]).all())


def test_image_sums_do_not_depend_on_the_batch():
    """Image i of the n = 3 call == the same image alone, bit for bit."""
    from monocular_depth_estimation_amd.functional import eval_pair_sums
    name = "odd_ratio_asym_crop"
    inv, inv_flip, gt = _inputs(name)
    full = _fused(name).cpu()
    for i in range(gt.shape[0]):
        one = eval_pair_sums(_dev(inv[i:i + 1]), _dev(inv_flip[i:i + 1]), _dev(gt[i:i + 1]), MAXD,
                             CASES[name][5]).cpu()
        assert torch.equal(one[0], full[i]), i


def test_deterministic_and_writes_into_out():
    name = "wide_x2_one_axis"
    a = _fused(name).cpu()
    big = torch.full((5, 2, 16), -1.0, dtype=torch.float64, device=DEV)
    r = _fused(name, out=big[2:4])
    assert r.data_ptr() == big[2:4].data_ptr()
    assert torch.equal(big[2:4].cpu(), a)
    assert bool((big[:2] == -1).all()) and bool((big[4:] == -1).all())


@pytest.mark.parametrize("name", list(CASES))
def test_under_guard(name):
    """Guard bands, poisoned outputs and scratch (tests/_abi_guard.py) around the new
    entry: nothing written outside a buffer, every output element written, no
    dependence on what scratch or the output held; results equal the unguarded run."""
    from monocular_depth_estimation_amd import _abi
    from tests._abi_guard import guarded_abi
    plain = _fused(name).cpu()
    with guarded_abi(signatures={**_abi.SIGNATURES, **_abi.EVAL_SIGNATURES}) as guard:
        got = _fused(name).cpu()
    assert guard.calls["mde_eval_pair_sums"] > 0
    assert torch.equal(got, plain)
