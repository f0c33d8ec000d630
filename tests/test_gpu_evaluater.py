"""GuideDepth.evaluate.Evaluater end to end on the GPU.

The yardstick is the reference's loop (src/GuideDepth/evaluate.py:84-142) written
here with ATen ops, one image at a time, with the reference's Result formulae
(src/GuideDepth/metrics.py:41-62) and its running average (:65-110).  Run in
float64 on the CPU it is the oracle; run in float32 on the GPU it is what the
reference computes (error e_old against the oracle).  Evaluater's averages
(error e_new) must satisfy e_new <= 2 e_old + 1e-9 |field| (half of the last
term for the square-rooted fields), the bound of tests/test_gpu_eval_pair.py,
and its delta averages must equal the oracle's exactly: the ground truth is
built so that no selected pixel's max(g/p, p/g) lies within relative 1e-5 of a
threshold, asserted before Evaluater runs.
"""
import math
import os
import types

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAXD = 10.0
LINEAR = ("mse", "mae", "absrel", "lg10", "imae")
ROOTED = ("rmse", "rmse_log", "irmse")
DELTAS = ("delta1", "delta2", "delta3")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")


class Recorder(torch.nn.Module):
    """Keeps what the wrapped network returned, so the loop can be fed exactly that."""

    def __init__(self, net):
        super().__init__()
        self.net, self.outs = net, []

    def forward(self, x):
        y = self.net(x)
        self.outs.append(y.detach().clone())
        return y


class Stub(torch.nn.Module):
    """Per-sample, batch-independent 'network': elementwise and per-sample ops only."""

    def forward(self, x):
        return x.mean(1, keepdim=True) * 20 + 0.5


def _args(tmp, mode="alhashim", resolution=(16, 24)):
    return types.SimpleNamespace(dataset="nyu", resolution=resolution, eval_mode=mode,
                                 save_results=str(tmp), model="GuideDepth", weights_path=None)


# --------------------------------------------------- the reference's loop, ATen
def _log10(x):
    return torch.log(x) / math.log(10)


def _result(output, target):
    """metrics.py:41-62 on one view; returns (fields, theta)."""
    abs_diff = (output - target).abs()
    r = {}
    r["mse"] = float(torch.pow(abs_diff, 2).mean())
    r["rmse"] = math.sqrt(r["mse"])
    r["mae"] = float(abs_diff.mean())
    r["lg10"] = float((_log10(output) - _log10(target)).abs().mean())
    r["rmse_log"] = math.sqrt(torch.pow(_log10(output) - _log10(target), 2).mean())
    r["absrel"] = float((abs_diff / target).mean())
    ratio = torch.max(output / target, target / output)
    # .float() in the reference; the loop's own dtype here, so that the float64 run
    # gives the exact fraction instead of its float32 rounding
    r["delta1"] = float((ratio < 1.25).to(output.dtype).mean())
    r["delta2"] = float((ratio < 1.25 ** 2).to(output.dtype).mean())
    r["delta3"] = float((ratio < 1.25 ** 3).to(output.dtype).mean())
    inv = (1 / output - 1 / target).abs()
    r["irmse"] = math.sqrt(torch.pow(inv, 2).mean())
    r["imae"] = float(inv.mean())
    return r, ratio


def _reference_loop(pairs, gts, crop, dtype, device):
    """evaluate.py:93-142 from the network's outputs on: pairs[i] = (inv, inv_flip)
    [1, 1, h, w] (inv_flip None: that view is left out), gts[i] [1, 1, H, W].
    Returns (averaged fields, per-image [theta view 0, theta view 1] in crop
    coordinates)."""
    sums, count, thetas = {}, 0, []
    for (inv, inv_flip), gt in zip(pairs, gts):
        gt = gt.to(device=device, dtype=dtype)
        gt_flip = torch.flip(gt, [3])
        per = []
        for x, g in ((inv, gt), (inv_flip, gt_flip)):
            if x is None:
                continue
            p = MAXD / x.to(device=device, dtype=dtype)
            p = torch.clamp(p, MAXD / 100, MAXD)
            if p.shape[-2:] != g.shape[-2:]:
                p = TF.interpolate(p, size=g.shape[-2:], mode="bilinear", align_corners=False)
            if crop is not None:
                g = g[:, :, crop[0]:crop[1], crop[2]:crop[3]]
                p = p[:, :, crop[0]:crop[1], crop[2]:crop[3]]
            r, th = _result(p, g)
            per.append(th)
            for k, v in r.items():
                sums[k] = sums.get(k, 0) + v
            count += 1
        thetas.append(per)
    return {k: v / count for k, v in sums.items()}, thetas


def _margin(pairs, gts, crop):
    """Smallest relative distance of a selected pixel's theta to a threshold in the float64
    loop, and per image the mask (gt coordinates) of the pixels closer than 1e-5."""
    H, W = gts[0].shape[-2:]
    c = crop if crop is not None else (0, H, 0, W)
    _, thetas = _reference_loop(pairs, gts, crop, torch.float64, "cpu")
    best, masks = math.inf, []
    for gt, per in zip(gts, thetas):
        bad = torch.zeros(gt.shape, dtype=torch.bool)
        for v, th in enumerate(per):
            near = torch.zeros(th.shape, dtype=torch.bool)
            for k in (1, 2, 3):
                rel = (th / 1.25 ** k - 1.0).abs()
                best = min(best, float(rel.min()))
                near |= rel < 1e-5
            full = torch.zeros(gt.shape, dtype=torch.bool)
            full[:, :, c[0]:c[1], c[2]:c[3]] = near
            bad |= torch.flip(full, [3]) if v == 1 else full
        masks.append(bad)
    return best, masks


def _settle_gt(pairs, gts, crop):
    """Nudge (by 0.3 %) the ground-truth pixels within 1e-5 of a threshold until none is;
    returns (gts, their margin)."""
    for _ in range(20):
        best, masks = _margin(pairs, gts, crop)
        if not any(bool(m.any()) for m in masks):
            break
        gts = [torch.where(m, gt * 1.003, gt) for gt, m in zip(gts, masks)]
    return gts, _margin(pairs, gts, crop)[0]


def _check_against_loop(avg, pairs, gts, crop):
    oracle, _ = _reference_loop(pairs, gts, crop, torch.float64, "cpu")
    old, _ = _reference_loop(pairs, gts, crop, torch.float32, DEV)
    for f in DELTAS:
        assert getattr(avg, f) == oracle[f], (f, getattr(avg, f), oracle[f])
    # AverageMeter.average() hands mae / rmse_log over in swapped positions (metrics.py:99-101)
    got = {f: getattr(avg, f) for f in LINEAR + ROOTED}
    got["mae"], got["rmse_log"] = avg.rmse_log, avg.mae
    for f in LINEAR + ROOTED:
        e_new, e_old = abs(got[f] - oracle[f]), abs(old[f] - oracle[f])
        slack = (0.5e-9 if f in ROOTED else 1e-9) * abs(oracle[f])
        print(f"{f}: oracle {oracle[f]:.9g} e_old {e_old:.3e} e_new {e_new:.3e}")
        assert math.isfinite(got[f])
        assert e_new <= 2 * e_old + slack, (f, e_new, e_old)


# ------------------------------------------------------------------ stub data
def _stub_data():
    gen = torch.Generator().manual_seed(77)
    images = [torch.rand((1, 3, 32, 48), generator=gen) for _ in range(5)]
    # ground truth correlated with what the stub will predict (delta fractions mid-range)
    gts = [torch.clamp(MAXD / Stub()(im) * torch.exp(0.25 * torch.randn((1, 1, 32, 48), generator=gen)),
                       0.3, 9.8) for im in images]
    return images, gts


def _clipped(crop, H, W):
    return (min(crop[0], H), min(crop[1], H), min(crop[2], W), min(crop[3], W))


def test_batching_is_exact(tmp_path):
    """batch_size 1 and 4 (a ragged last batch): bit-identical averages, byte-identical
    results.txt."""
    from monocular_depth_estimation_amd.GuideDepth.evaluate import Evaluater
    images, gts = _stub_data()
    out = []
    for bs in (1, 4):
        d = tmp_path / f"bs{bs}"
        ev = Evaluater(_args(d), model=Stub(), test_loader=list(zip(images, gts)), batch_size=bs)
        avg = ev.evaluate()
        out.append(([getattr(avg, f) for f in LINEAR + ROOTED + DELTAS],
                    open(os.path.join(str(d), "results.txt"), "rb").read()))
    assert out[0][0] == out[1][0]
    assert out[0][1] == out[1][1] and out[0][1].startswith(b"RMSE,MAE,REL, RMSE_log,Lg10,")


def test_against_the_reference_loop(tmp_path):
    """'alhashim' at a custom (16, 24) resolution, the NYU crop clipped to the 32 x 48 ground
    truth as the reference's slices clip it: rows [20, 32), columns [24, 48)."""
    from monocular_depth_estimation_amd.GuideDepth.evaluate import Evaluater, crops
    images, gts = _stub_data()
    crop = _clipped(crops["nyu"], 32, 48)
    assert crop == (20, 32, 24, 48)
    ev = Evaluater(_args(tmp_path), model=Stub(), batch_size=2)
    # the loop gets what the network returned on the GPU (fp32), as the reference's would
    with torch.no_grad():
        pairs = []
        for im in images:
            im = im.to(DEV)
            a, b = ev.predict(ev.downscale_image(im), ev.downscale_image(torch.flip(im, [3])))
            pairs.append((a.cpu(), b.cpu()))
    gts, margin = _settle_gt(pairs, gts, crop)
    print(f"smallest relative distance of theta to a threshold {margin:.3e}")
    assert margin >= 1e-5, margin
    ev.test_loader = list(zip(images, gts))
    avg = ev.evaluate()
    _check_against_loop(avg, pairs, gts, crop)


def test_other_modes_neither_resize_nor_crop(tmp_path):
    """eval_mode != 'alhashim': the prediction is at the ground-truth resolution and every
    pixel counts; the averages are those of Result.evaluate(prediction, gt) and its
    flipped twin."""
    from monocular_depth_estimation_amd.GuideDepth.evaluate import Evaluater
    from monocular_depth_estimation_amd.GuideDepth.metrics import AverageMeter, Result
    images, gts = _stub_data()
    images, gts = images[:3], gts[:3]
    ev = Evaluater(_args(tmp_path, mode="eigen", resolution="half"), model=Stub(),
                   test_loader=list(zip(images, gts)), batch_size=2)
    avg = ev.evaluate()
    meter = AverageMeter()
    for im, gt in zip(images, gts):
        im, gt = im.to(DEV), gt.to(DEV)
        for x, g in ((im, gt), (torch.flip(im, [3]), torch.flip(gt, [3]))):
            r = Result()
            r.evaluate(ev.inverse_depth_norm(Stub()(x)), g)
            meter.update(r, 0, 0, 1)
    want = meter.average()
    # The depth at every pixel is bit for bit the same, so every sum differs only in the order
    # of its double additions -- except the two log10 fields: the fused kernel rounds log10
    # correctly, eval_sums calls the device library's log10f (2 ulp).  Depths lie in
    # [0.1, 10], so a log10 value is below 2 in magnitude (ulp 2^-23) and a term, the
    # difference of two of them, moves by at most 2 x 2.5 ulp; the mean of |term| and the
    # root of the mean square move by no more than a term does.  (average() holds
    # rmse_log in .mae, metrics.py:99-101.)
    log_fields = {"lg10": 5 * 2.0 ** -23, "mae": 5 * 2.0 ** -23}
    for f in LINEAR + ROOTED:
        if f in log_fields:
            assert abs(getattr(avg, f) - getattr(want, f)) <= log_fields[f], f
        else:
            assert math.isclose(getattr(avg, f), getattr(want, f), rel_tol=1e-12), f
    for f in DELTAS:
        assert getattr(avg, f) == getattr(want, f), f


def test_real_model_once(tmp_path):
    """A seeded random-weight GuideDepth in eval mode at 64 x 96 (the smallest input of the
    GuideDepth GPU tests), 2 images, ground truth at 128 x 192."""
    from monocular_depth_estimation_amd import _abi
    from monocular_depth_estimation_amd.GuideDepth.evaluate import Evaluater, crops
    from monocular_depth_estimation_amd.GuideDepth.model.GuideDepth import GuideDepth
    from oracle.weights import fill_
    gen = torch.Generator().manual_seed(5)
    images = [torch.rand((1, 3, 128, 192), generator=gen) for _ in range(2)]
    gts = [0.3 + 9.5 * torch.rand((1, 1, 128, 192), generator=gen) for _ in range(2)]
    crop = _clipped(crops["nyu"], 128, 192)
    model = Recorder(fill_(GuideDepth(pretrained=False))).to(DEV).eval()
    ev = Evaluater(_args(tmp_path, resolution=(64, 96)), model=model, batch_size=1)
    with torch.no_grad():
        pairs = []
        for im in images:
            im = im.to(DEV)
            a, b = ev.predict(ev.downscale_image(im), ev.downscale_image(torch.flip(im, [3])))
            pairs.append((a.cpu(), b.cpu()))
    assert pairs[0][0].shape == (1, 1, 64, 96)
    gts, margin = _settle_gt(pairs, gts, crop)
    print(f"smallest relative distance of theta to a threshold {margin:.3e}")
    assert margin >= 1e-5, margin
    ev.test_loader = list(zip(images, gts))
    del model.outs[:]
    _abi.timing_enable(True)
    _abi.timing_reset()
    try:
        avg = ev.evaluate()
        torch.cuda.synchronize()
        counts = {k: v[1] for k, v in _abi.timing_collect().items()}
    finally:
        _abi.timing_enable(False)
        _abi.timing_reset()
    assert counts.get("eval_pair") == 2 and counts.get("eval_pair_final") == 2, counts
    assert "eval_sums" not in counts
    # The loop is fed predict()'s outputs of the evaluated run itself: library convolutions
    # may pick another algorithm from one call to the next, which moves the network's
    # output in the last bits and has nothing to do with what is compared here.
    assert len(model.outs) == 2 and model.outs[0].shape == (2, 1, 64, 96)
    seen = [(o[:1].cpu(), o[1:].cpu()) for o in model.outs]
    print("forward repeats bit for bit:",
          all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(pairs, seen)))
    margin = _margin(seen, gts, crop)[0]
    assert margin >= 1e-5, margin
    _check_against_loop(avg, seen, gts, crop)
    assert avg.gpu_time > 0
