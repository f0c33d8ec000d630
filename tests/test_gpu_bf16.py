"""BASELINE cfg3 precision (bf16 autocast) against the FLOAT64 oracle.

The training step runs under torch.autocast(bfloat16): MIOpen / hipBLASLt
convolutions and GEMMs compute in bf16 (8-bit mantissa, unit roundoff
2^-9 = 2.0e-3), the HIP BatchNorm kernels keep bf16 activations with fp32
statistics, the other HIP kernels compute in fp32.  Truth is the oracle
(oracle/guidedepth.py pinned to the reference by the goldens;
oracle/mobilenetv3.py restated, parity unpinned) run in float64 on the same
weights and inputs.

How close bf16 can get depends on the network's conditioning, not on the
kernels: on these deterministically filled nets, train-mode BatchNorm over the
few values of DDRNet's 1x1 / 2x2 bottom maps amplifies a 2^-9 rounding into
tens of percent (the fp32 path already sits ~5e-3 from float64 there).  So
the bf16 bar is the REFERENCE ALGORITHM's own bf16 error: the oracle run
under CPU bf16 autocast (oneDNN bf16 convolutions, same weights and inputs)
is measured against the same float64 truth in the test, and the HIP path
must stay within

  depth map (max |err| / max |truth|)     <= 2 x oracle-bf16 error + 1e-2
  loss (relative)                          <= 2 x oracle-bf16 error + 2e-3
  grad norms: median relative error        <= 2 x oracle-bf16 median + 1e-2
              90th percentile               <= 2 x oracle-bf16 p90 + 2e-2
"""
import numpy as np
import pytest
import torch

from oracle import guidedepth as og
from oracle import mobilenetv3 as om
from oracle import ops as oops
from oracle.weights import fill_, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ws(nbytes, like):
    """The product's workspace helper: exactly the queried size, 1-D uint8."""
    from monocular_depth_estimation_amd.functional import _ws as ws
    return ws(nbytes, like)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")


def _grad_rel(model, truth, skip=""):
    got, want = dict(model.named_parameters()), dict(truth.named_parameters())
    norms = {k: float(p.grad.norm()) for k, p in want.items() if p.grad is not None}
    top = max(norms.values())
    return np.array([abs(float(got[k].grad.double().norm()) - w) / w
                     for k, w in norms.items()
                     if w > 1e-6 * top and not (skip and k.startswith(skip))])


def _errors(pred, loss, model, tp, tl, truth, skip=""):
    pred, loss = pred.detach().double().cpu(), float(loss.detach())
    rel = _grad_rel(model, truth, skip)
    return {"map": float((pred - tp.detach()).abs().max()) / float(tp.detach().abs().max()),
            "loss": abs(loss - float(tl.detach())) / abs(float(tl.detach())),
            "med": float(np.median(rel)), "p90": float(np.percentile(rel, 90))}


def _compare(build_truth, build_ours, build_cpu, x, d, what, skip=""):
    truth = build_truth().double().train()
    tp = truth(x.double())
    tl = oops.train_loss(tp, d.double())
    tl.backward()
    # the reference algorithm's own bf16 error (CPU autocast, same weights / inputs)
    cpu = build_cpu().train()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        cp = cpu(x)
    cl = oops.train_loss(cp.float(), d)
    cl.backward()
    floor = _errors(cp.float(), cl, cpu, tp, tl, truth, skip)
    from monocular_depth_estimation_amd.loss import SSIML1
    ours = build_ours().to(DEV).train()
    with torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        pred = ours(x.to(DEV))
        loss = SSIML1(1.0, 0.1)(pred, d.to(DEV))
    loss.backward()
    got = _errors(pred, loss, ours, tp, tl, truth, skip)
    print(f"{what}: HIP bf16 {got}  oracle bf16 {floor}")
    assert got["map"] <= 2 * floor["map"] + 1e-2, (got, floor)
    assert got["loss"] <= 2 * floor["loss"] + 2e-3, (got, floor)
    assert got["med"] <= 2 * floor["med"] + 1e-2, (got, floor)
    assert got["p90"] <= 2 * floor["p90"] + 2e-2, (got, floor)


def test_guidedepth_bf16_golden_vs_float64_oracle(golden):
    """Golden 2x3x64x96 step: map, loss and the DECODER's gradient norms.

    The encoder's gradient norms are ill-conditioned at batch 2 (DAPPM's
    pooled branches reach train-mode BatchNorm with two values per channel at
    1x1): the fp32 HIP step with its input perturbed by about one bf16
    rounding (+-2^-9 relative) moves the encoder's median gradient-norm
    difference by 0.07-2.5 while the decoder's stays at 0.04-0.06
    (profiles/r03_bf16_grad_conditioning.txt, tools/grad_conditioning.py),
    so any bf16 rounding difference lands anywhere in that range.  The
    whole-model gradient check is the batch-8 case below, where the same
    perturbation moves the encoder by 0.01."""
    from monocular_depth_estimation_amd import GuideDepth
    g = golden("golden_guidedepth.npz")
    _compare(lambda: fill_(og.GuideDepth()), lambda: fill_(GuideDepth(pretrained=False)),
             lambda: fill_(og.GuideDepth()), torch.from_numpy(g["x"]), torch.from_numpy(g["depth"]),
             "GuideDepth bf16 golden 64x96", skip="feature_extractor")


def test_guidedepth_bf16_240x320_vs_float64_oracle():
    """Whole model (encoder included) at batch 8, 240x320: well-conditioned
    (input perturbation of one bf16 rounding moves gradient norms by a median
    0.01, p90 0.05-0.07; profiles/r03_bf16_grad_conditioning.txt)."""
    from monocular_depth_estimation_amd import GuideDepth
    x = torch.from_numpy(seeded((8, 3, 240, 320), 71, 0, 1))
    d = torch.from_numpy(seeded((8, 1, 240, 320), 72, 0.1, 10.0))
    _compare(lambda: fill_(og.GuideDepth()), lambda: fill_(GuideDepth(pretrained=False)),
             lambda: fill_(og.GuideDepth()), x, d, "GuideDepth bf16 8x240x320")


def test_ptmodel_bf16_vs_float64_oracle():
    """cfg4 model (MobileNetV3-L + NewCRF) under bf16 autocast, 128x160 bs 2."""
    from monocular_depth_estimation_amd.model_mobileV3_large_newCRFs import PTModel
    state = fill_(om.PTModel()).state_dict()

    def ours():
        m = PTModel()
        m.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in state.items()})
        return m

    x = torch.from_numpy(seeded((2, 3, 128, 160), 21, 0, 1))
    d = torch.from_numpy(seeded((2, 1, 128, 160), 22, 0.5, 10))
    _compare(lambda: fill_(om.PTModel()), ours, lambda: fill_(om.PTModel()), x, d, "PTModel bf16")


@pytest.mark.parametrize("cin,cout,n,h,w", [(16, 8, 4, 96, 128), (32, 16, 2, 60, 80), (64, 32, 2, 30, 64),
                                            (64, 64, 2, 30, 64)])
def test_bnrelu_pointwise_bf16_storage_matches_fp32_kernel(cin, cout, n, h, w):
    """The fused BN-ReLU-1x1 pair on bf16 activations (autocast) vs the fp32
    kernels on the same values.  The bf16 path rounds the 1x1's operands to
    bf16 (the BN-ReLU output and the weight, as autocast hands a conv) and
    multiplies on the bf16 MFMA with fp32 sums (pwbf.hip): y2 within a bf16
    rounding plus the operand roundings' sum error, the gradients within 1e-2
    of their max; the BN's running statistics (from y1 alone) bit-exact."""
    import copy

    from monocular_depth_estimation_amd.nn import BatchNorm2d, bn_relu_pointwise
    g = torch.Generator().manual_seed(cin + cout + h)
    y1 = (torch.rand((n, cin, h, w), generator=g) * 2 - 0.7).to(DEV).to(torch.bfloat16)
    gy2 = (torch.rand((n, cout, h, w), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    bn = BatchNorm2d(cin, act="relu").to(DEV).train()
    conv = torch.nn.Conv2d(cin, cout, 1).to(DEV)
    outs = []
    for dt in (torch.bfloat16, torch.float32):
        b, c = copy.deepcopy(bn), copy.deepcopy(conv)
        x = y1.detach().to(dt).clone().requires_grad_(True)
        y2, _ = bn_relu_pointwise(x, b, None, c, None, False)
        assert y2.dtype == dt
        y2.backward(gy2.to(dt))
        outs.append((y2.detach(), x.grad, c.weight.grad, b.weight.grad, b.running_var.clone()))
    (ya, ga, wa, gga, rva), (yb, gb, wb, ggb, rvb) = outs
    assert torch.equal(rva, rvb)

    def rel(a, b):
        return float((a.float() - b.float()).abs().max()) / float(b.float().abs().max())

    assert rel(ya, yb) <= 1e-2, rel(ya, yb)
    assert rel(wa, wb) <= 1e-2, rel(wa, wb)
    assert rel(ga, gb) <= 1e-2, rel(ga, gb)
    assert rel(gga, ggb) <= 1e-2, rel(gga, ggb)


PW_SHAPES = [(16, 8), (16, 16), (32, 16), (32, 32), (64, 32), (32, 64), (16, 32), (64, 64)]


@pytest.mark.parametrize("cin,cout", PW_SHAPES)
@pytest.mark.parametrize("bnr", [True, False])
def test_pointwise_bf16_products_vs_float64(cin, cout, bnr):
    """pwbf.hip against float64 on the operands autocast hands the 1x1 conv:
    s = bf16(relu(x * sc + sh)) (or x), W rounded to bf16.  y / gs within 2^-8
    of each element plus 1e-3 of the max (one bf16 rounding of an fp32 sum);
    gW within 1e-4 of its max (fp32 sums of exact bf16 products over 61k
    pixels); the BN-sum epilogue (cin <= 32) within 1e-4 of its scale."""
    from monocular_depth_estimation_amd import _abi
    n, h, w = 2, 48, 640  # hw % 64 == 0; 960 tiles: a few per wave
    g = torch.Generator().manual_seed(7 * cin + cout + bnr)
    x = (torch.rand((n, cin, h, w), generator=g) * 2 - 0.7).to(torch.bfloat16)
    gy = (torch.rand((n, cout, h, w), generator=g) - 0.5).to(torch.bfloat16)
    wt = (torch.rand((cout, cin), generator=g) - 0.5) * (3.0 / cin) ** 0.5
    sc = torch.rand(cin, generator=g) + 0.5
    sh = torch.rand(cin, generator=g) - 0.5
    mean = torch.rand(cin, generator=g) * 0.2
    xf = x.float()
    s = (xf * sc[:, None, None] + sh[:, None, None]).clamp(min=0) if bnr else xf
    s = s.to(torch.bfloat16).double()
    wb = wt.to(torch.bfloat16).double()
    y_ref = torch.einsum("oc,nchw->nohw", wb, s)
    gs_ref = torch.einsum("oc,nohw->nchw", wb, gy.double())
    gw_ref = torch.einsum("nohw,nchw->oc", gy.double(), s)
    d = dict(device=DEV)
    xg, gyg, wg = x.to(**d), gy.to(**d), wt.to(**d)
    scg, shg, mug = sc.to(**d), sh.to(**d), mean.to(**d)
    st = _abi.stream_of(xg)
    bf = _abi.MDE_BF16
    y = torch.empty((n, cout, h, w), dtype=torch.bfloat16, **d)
    _abi.call("mde_pointwise_fwd", _abi.ptr(xg), _abi.ptr(scg) if bnr else None,
              _abi.ptr(shg) if bnr else None, _abi.ptr(wg), _abi.ptr(y), n, cin, cout, h, w, bf, st)
    gs = torch.empty_like(xg)
    gw = torch.empty((cout, cin), dtype=torch.float32, **d)
    ws = _ws(_abi.query("mde_pointwise_workspace", n, cin, cout, h, w), xg)
    sums = None
    if bnr and cin <= 32:
        sums = torch.empty((cin, 2), dtype=torch.float32, **d)
        _abi.call("mde_pointwise_bwd_bn", _abi.ptr(gyg), _abi.ptr(xg), _abi.ptr(scg), _abi.ptr(shg),
                  _abi.ptr(mug), _abi.ptr(wg), _abi.ptr(gs), _abi.ptr(gw), _abi.ptr(sums), n, cin,
                  cout, h, w, _abi.ptr(ws), bf, st)
    else:
        _abi.call("mde_pointwise_bwd", _abi.ptr(gyg), _abi.ptr(xg), _abi.ptr(scg) if bnr else None,
                  _abi.ptr(shg) if bnr else None, _abi.ptr(wg), _abi.ptr(gs), _abi.ptr(gw), n, cin,
                  cout, h, w, _abi.ptr(ws), bf, st)
    torch.cuda.synchronize()

    def close(got, ref):
        got = got.double().cpu()
        bad = (got - ref).abs() > 2.0 ** -8 * ref.abs() + 1e-3 * ref.abs().max()
        return int(bad.sum())

    assert close(y, y_ref) == 0
    assert close(gs, gs_ref) == 0
    err = float((gw.double().cpu() - gw_ref).abs().max() / gw_ref.abs().max())
    assert err <= 1e-4, err
    if sums is not None:
        # gs_ref from the exact products; the kernel sums its fp32 gs (unrounded)
        m = ((xf * sc[:, None, None] + sh[:, None, None]) > 0).double()
        e = gs_ref * m
        s1 = e.sum((0, 2, 3))
        s2 = (e * (xf.double() - mean.double()[:, None, None])).sum((0, 2, 3))
        sc1 = float(e.abs().sum((0, 2, 3)).max())
        got = sums.double().cpu()
        assert float((got[:, 0] - s1).abs().max()) <= 1e-4 * sc1
        assert float((got[:, 1] - s2).abs().max()) <= 1e-4 * sc1 * 2


@pytest.mark.parametrize("cin,cout,n,h,w", [(64, 32, 2, 60, 80), (32, 16, 3, 48, 64)])
def test_skip_reduce_bf16_storage_matches_fp32_kernel(cin, cout, n, h, w):
    """reduce(residual + depth) on bf16 activations == the fp32 kernel on the
    same values: output and the shared input gradient bit-exact with the
    rounded fp32 results, weight / bias gradients bit-exact."""
    from monocular_depth_estimation_amd.functional import skip_reduce
    g = torch.Generator().manual_seed(cin + h)
    r = (torch.rand((n, cin, h, w), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    d = (torch.rand((n, cin, h, w), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    go = (torch.rand((n, cout, h, w), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    wt = ((torch.rand((cout, cin, 1, 1), generator=g) - 0.5) * 0.3).to(DEV)
    bias = (torch.rand((cout,), generator=g) - 0.5).to(DEV)
    outs = []
    for dt in (torch.bfloat16, torch.float32):
        rr = r.detach().to(dt).clone().requires_grad_(True)
        dd = d.detach().to(dt).clone().requires_grad_(True)
        ww = wt.clone().requires_grad_(True)
        bb = bias.clone().requires_grad_(True)
        y = skip_reduce(rr, dd, ww, bb)
        assert y.dtype == dt
        y.backward(go.to(dt))
        outs.append((y.detach(), rr.grad, ww.grad, bb.grad))
    (ya, ga, wa, ba), (yb, gb, wb, bb_) = outs
    assert torch.equal(ya, yb.to(torch.bfloat16))
    assert torch.equal(ga, gb.to(torch.bfloat16))
    assert torch.equal(wa, wb) and torch.equal(ba, bb_)


@pytest.mark.parametrize("cin,cout,n,h,w", [(64, 32, 2, 60, 80), (32, 16, 3, 48, 64), (16, 1, 2, 48, 64),
                                             (4, 1, 2, 30, 40)])
def test_skip_reduce_bn_bf16_storage_matches_fp32_kernel(cin, cout, n, h, w):
    """reduce(relu(bn(r + pb)) + d) (the comb_conv's last BN + ReLU and the skip
    fusion, modules.py:72-73,100) on bf16 activations vs the fp32 kernels on
    the same values.  1-output-channel shapes (fp32 products): output and d's
    gradient bit-exact with the rounded fp32 results; 1x1 weight / bias
    gradients to 1e-5 (the BN coefficients of a bf16
    and an fp32 input can differ in the last bit: the statistics pass sums in
    another order per storage width); r's gradient (the BN apply reads the
    stored, rounded skip gradient) to bf16 rounding."""
    import copy

    from monocular_depth_estimation_amd.nn import BatchNorm2d, skip_reduce_bn
    g = torch.Generator().manual_seed(cin + cout + h)
    r = (torch.rand((n, cin, h, w), generator=g) * 2 - 0.7).to(DEV).to(torch.bfloat16)
    d = (torch.rand((n, cin, h, w), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    go = (torch.rand((n, cout, h, w), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    wt = ((torch.rand((cout, cin, 1, 1), generator=g) - 0.5) * 0.3).to(DEV)
    bias = (torch.rand((cout,), generator=g) - 0.5).to(DEV)
    pb = (torch.rand((cin,), generator=g) - 0.5).to(DEV)
    bn = BatchNorm2d(cin, act="relu").to(DEV).train()
    outs = []
    for dt in (torch.bfloat16, torch.float32):
        b = copy.deepcopy(bn)
        rr = r.detach().to(dt).clone().requires_grad_(True)
        dd = d.detach().to(dt).clone().requires_grad_(True)
        ww, bb = wt.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        y = skip_reduce_bn(rr, b, pb, dd, ww, bb)
        assert y.dtype == dt
        y.backward(go.to(dt))
        outs.append((y.detach(), dd.grad, ww.grad, bb.grad, rr.grad, b.weight.grad,
                     b.running_var.clone()))
    (ya, gda, wa, ba, gra, gga, rva), (yb, gdb, wb, bb_, grb, ggb, rvb) = outs
    torch.testing.assert_close(rva, rvb, rtol=1e-6, atol=0)
    assert float((gra.float() - grb).abs().max()) <= 1e-2 * float(grb.abs().max())
    if (cin, cout) in ((64, 32), (32, 16)):
        # bf16 products (pwbf.hip): the 1x1 sees s = bf16(bf16(relu(bn(r))) + d) and the
        # weight rounded to bf16, as autocast's conv does -- within bf16 rounding of the
        # fp32-product kernels
        def rel(a, b):
            return float((a.float() - b.float()).abs().max()) / float(b.float().abs().max())
        assert rel(ya, yb) <= 1e-2 and rel(gda, gdb) <= 1e-2
        assert rel(wa, wb) <= 1e-2 and rel(ba, bb_) <= 1e-3
        return
    assert torch.equal(ya, yb.to(torch.bfloat16))
    assert torch.equal(gda, gdb.to(torch.bfloat16))
    torch.testing.assert_close(wa, wb, rtol=1e-5, atol=1e-5 * float(wb.abs().max()))
    torch.testing.assert_close(ba, bb_, rtol=1e-5, atol=1e-5 * float(bb_.abs().max()))
    assert float((gga - ggb).abs().max()) <= 1e-2 * float(ggb.abs().max())


@pytest.mark.parametrize("ca,cb,n,h,w", [(16, 16, 2, 60, 80), (8, 8, 3, 48, 64), (32, 32, 2, 30, 40)])
def test_se_bn_cat_bf16_storage_matches_fp32_kernel(ca, cb, n, h, w):
    """SELayer(cat([relu(bn_a(ya)), relu(bn_b(yb))])) (modules.py:21-25,49,59,90) on
    bf16 activations == the fp32 kernels on the same values: SE output and both
    input gradients bit-exact with the rounded fp32 results; BN parameter and
    SE weight gradients and the running statistics bit-exact."""
    import copy

    from monocular_depth_estimation_amd.nn import BatchNorm2d, se_bn_cat
    g = torch.Generator().manual_seed(ca + cb + h)
    ya = (torch.rand((n, ca, h, w), generator=g) * 2 - 0.7).to(DEV).to(torch.bfloat16)
    yb = (torch.rand((n, cb, h, w), generator=g) * 2 - 0.6).to(DEV).to(torch.bfloat16)
    go = (torch.rand((n, ca + cb, h, w), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    c = ca + cb
    w1 = ((torch.rand((c, c), generator=g) - 0.5) * 0.3).to(DEV)
    w2 = ((torch.rand((c, c), generator=g) - 0.5) * 0.3).to(DEV)
    pa = (torch.rand((ca,), generator=g) - 0.5).to(DEV)
    pbb = (torch.rand((cb,), generator=g) - 0.5).to(DEV)
    bna, bnb = BatchNorm2d(ca, act="relu").to(DEV).train(), BatchNorm2d(cb, act="relu").to(DEV).train()
    outs = []
    for dt in (torch.bfloat16, torch.float32):
        a, b = copy.deepcopy(bna), copy.deepcopy(bnb)
        xa = ya.detach().to(dt).clone().requires_grad_(True)
        xb = yb.detach().to(dt).clone().requires_grad_(True)
        v1, v2 = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
        out = se_bn_cat(xa, xb, a, b, pa, pbb, v1, v2)
        assert out.dtype == dt
        out.backward(go.to(dt))
        outs.append((out.detach(), xa.grad, xb.grad, a.weight.grad, b.bias.grad, v1.grad, v2.grad,
                     a.running_mean.clone(), b.running_var.clone()))
    fa, fb = outs
    assert torch.equal(fa[0], fb[0].to(torch.bfloat16))
    assert torch.equal(fa[1], fb[1].to(torch.bfloat16))
    assert torch.equal(fa[2], fb[2].to(torch.bfloat16))
    for u, v in zip(fa[3:], fb[3:]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("c,h,w", [(64, 60, 80), (16, 30, 40), (8, 15, 21)])
def test_bilinear_x2_bf16_storage_matches_fp32_kernel(c, h, w):
    """The exact x2 upsample (GuideDepth.py:49,52,55) on bf16 storage == the fp32
    kernel on the same values, rounded: forward, backward, and the two-gradient
    backward (the GradSlot sum) bit-exact; wi odd takes the one-column kernels."""
    from monocular_depth_estimation_amd import _abi
    from monocular_depth_estimation_amd.functional import bilinear_resize
    g = torch.Generator().manual_seed(c + h + w)
    n = 2
    x = (torch.rand((n, c, h, w), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    gy = (torch.rand((n, c, 2 * h, 2 * w), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    gy2 = (torch.rand((n, c, 2 * h, 2 * w), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    res = []
    for dt in (torch.bfloat16, torch.float32):
        xx = x.detach().to(dt).clone().requires_grad_(True)
        y = bilinear_resize(xx, scale_factor=2)
        assert y.dtype == dt
        y.backward(gy.to(dt))
        two = None
        if w % 2 == 0:
            two = torch.empty_like(xx)
            g1, g2 = gy.to(dt).contiguous(), gy2.to(dt).contiguous()  # alive across the launch
            _abi.call("mde_bilinear_bwd2", _abi.ptr(g1), _abi.ptr(g2), _abi.ptr(two), n, c, h, w,
                      2 * h, 2 * w, 0.5, 0.5, 0, _abi.dtype_code(xx), _abi.stream_of(xx))
            torch.cuda.synchronize()
        res.append((y.detach(), xx.grad, two))
    (ya, ga, ta), (yb, gb, tb) = res
    assert torch.equal(ya, yb.to(torch.bfloat16))
    assert torch.equal(ga, gb.to(torch.bfloat16))
    if ta is not None:
        assert torch.equal(ta, tb.to(torch.bfloat16))


# (c, hi, wi, ho, wo, align): DDRNet's resizes (DDRNet_23_slim.py:182-191, 332-351 --
# 15x20 -> 60x80 on the x4 kernel, 8x10 -> 60x80 and 4x5 -> 8x10 on the plane
# backward), a band-backward plane (40x50 -> 140x180), the generic backward
# (4x5 -> 128x128), an odd output width (generic forward, one column per
# thread), a downsample and align_corners=True
GENERIC = [(64, 15, 20, 60, 80, False), (128, 8, 10, 60, 80, False), (32, 4, 5, 8, 10, False),
           (8, 40, 50, 140, 180, False), (4, 4, 5, 128, 128, False), (16, 9, 11, 20, 27, False),
           (16, 33, 47, 17, 23, False), (8, 12, 16, 30, 41, True)]


@pytest.mark.parametrize("c,hi,wi,ho,wo,align", GENERIC)
def test_bilinear_generic_bf16_storage_matches_fp32_kernel(c, hi, wi, ho, wo, align):
    """Every non-x2 bilinear kernel on bf16 storage (autocast; F.interpolate
    keeps its input dtype) == the fp32 kernel on the same values, rounded once:
    forward and backward bit-exact, output / gradient dtype bf16."""
    from monocular_depth_estimation_amd.functional import bilinear_resize
    g = torch.Generator().manual_seed(c + hi + wo)
    n = 2
    x = (torch.rand((n, c, hi, wi), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    gy = (torch.rand((n, c, ho, wo), generator=g) - 0.5).to(DEV).to(torch.bfloat16)
    res = []
    for dt in (torch.bfloat16, torch.float32):
        xx = x.detach().to(dt).clone().requires_grad_(True)
        y = bilinear_resize(xx, size=(ho, wo), align_corners=align)
        assert y.dtype == dt
        y.backward(gy.to(dt))
        assert xx.grad.dtype == dt
        res.append((y.detach(), xx.grad))
    (ya, ga), (yb, gb) = res
    assert torch.equal(ya, yb.to(torch.bfloat16))
    assert torch.equal(ga, gb.to(torch.bfloat16))


@pytest.mark.parametrize("cout,h,w", [(16, 64, 96), (32, 37, 70), (64, 30, 40), (16, 21, 36),
                                      (32, 9, 100)])
def test_guide_conv_bf16_matches_rounded_fp32_kernel(cout, h, w):
    """The autocast guide conv (mde_conv3x3_guide_bf16_fwd, modules.py:52-54):
    image and weight rounded to bf16, fp32 accumulation, bf16 output == the
    fp32 HIP kernel on the rounded image and weight, output rounded (the same
    accumulation order): bit-exact, and its statistics epilogue == the fp32
    kernel's statistics of those rounded outputs within fp32 summation."""
    from monocular_depth_estimation_amd import _abi
    n = 2
    g = torch.Generator().manual_seed(cout + h)
    x = (torch.rand((n, 3, h, w), generator=g)).to(DEV)
    wt = ((torch.rand((cout, 3, 3, 3), generator=g) - 0.5) * 0.5).to(DEV)
    y = torch.empty((n, cout, h, w), dtype=torch.bfloat16, device=DEV)
    nb = _abi.query("mde_conv3x3_guide_bf16_stats_blocks", n, cout, h, w)
    stats = torch.empty((cout, nb, 4), device=DEV)
    st = _abi.stream_of(x)
    _abi.call("mde_conv3x3_guide_bf16_fwd", _abi.ptr(x), _abi.ptr(wt), _abi.ptr(y), _abi.ptr(stats),
              n, cout, h, w, st)
    xr = x.to(torch.bfloat16).float()
    wr = wt.to(torch.bfloat16).float()
    ref = torch.empty((n, cout, h, w), device=DEV)
    _abi.call("mde_conv3x3_fwd", _abi.ptr(xr), _abi.ptr(wr), _abi.ptr(ref), n, 3, cout, h, w, 0, st)
    assert torch.equal(y, ref.to(torch.bfloat16))
    yf = y.float()
    cnt = stats[:, :, 1].sum(1)
    mean = ((stats[:, :, 2] + stats[:, :, 0] * stats[:, :, 1]).sum(1) / cnt).double()
    assert torch.allclose(cnt, torch.full_like(cnt, n * h * w))
    assert torch.allclose(mean, yf.double().mean((0, 2, 3)), rtol=1e-5, atol=1e-6)
