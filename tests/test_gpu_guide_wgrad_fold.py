"""The guide convs' weight gradient with the BatchNorm backward apply on its
operand load (include/mde_wgrad_fold_abi.h) against the pair it replaces,
mde_batchnorm_bwd_apply -> mde_conv3x3_wgrad: bit for bit (torch.equal), at
the entries, in a Guided_Upsampling_Block and in a GuideDepth step.

No tolerance anywhere: the deferred kernel evaluates the apply kernel's fp32
operations one for one (csrc/pw_defer.h) and everything after its LDS store is
the text of the kernel fed the applied gradient, so the sums and their order
are the same.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
COUTS = [16, 32, 64]
# (n, h, w): the FULL path (w % 64 == 0) at h w = 1024 exactly, the smallest
# routed plane; the generic float4 path with a ragged last row tile (17 rows)
# and an 8-column last tile; w % 4 != 0, the element-load path
SIZES = [(2, 16, 64), (2, 17, 72), (1, 18, 58)]
NEW = ("mde_conv3x3_wgrad_bn_deferred", "mde_batchnorm_bwd_reduce_coef")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    import monocular_depth_estimation_amd  # noqa: F401


def _ws(nbytes, like):
    from monocular_depth_estimation_amd.functional import _ws as ws
    return ws(nbytes, like)


def _inputs(cout, n, h, w):
    """x (the image), y (the conv's output) ~ U(-1, 1), g (upstream of the
    BatchNorm + ReLU), and BatchNorm constants whose scale lies in [0.5, 1.5]
    and shift in [-0.2, 0.2]."""
    gen = torch.Generator().manual_seed(100 * cout + h * w + n)
    x = torch.rand((n, 3, h, w), generator=gen).to(DEV)
    y = (torch.rand((n, cout, h, w), generator=gen) * 2 - 1).to(DEV)
    g = (torch.rand((n, cout, h, w), generator=gen) - 0.5).to(DEV)
    scale = (torch.rand(cout, generator=gen) + 0.5).to(DEV)
    shift = (torch.rand(cout, generator=gen) * 0.4 - 0.2).to(DEV)
    mean = y.mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(y.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    gamma = scale / invstd
    beta = shift + mean * scale
    sc = gamma * invstd
    sh = beta - mean * sc
    assert float(sc.min()) > 0.49 and float(sc.max()) < 1.51
    assert float(sh.min()) > -0.21 and float(sh.max()) < 0.21
    pos = y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) > 0
    share = float(pos.float().mean())
    assert 0.2 < share < 0.8, share  # the ReLU mask is mixed
    # the BatchNorm backward's sums [c][2] = sum dy', sum dy' (y - mean), by a reduce
    e = g * pos
    sums = torch.stack([e.sum(dim=(0, 2, 3)),
                        (e * (y - mean.view(1, -1, 1, 1))).sum(dim=(0, 2, 3))], 1).contiguous()
    return dict(x=x, y=y, g=g, gamma=gamma.contiguous(), beta=beta.contiguous(),
                mean=mean.contiguous(), invstd=invstd.contiguous(), sums=sums)


def _wgrad(gy, x, n, cout, h, w):
    from monocular_depth_estimation_amd import _abi
    gw = torch.empty((cout, 3, 3, 3), device=DEV)
    ws = _ws(_abi.query("mde_conv3x3_wgrad_workspace", n, 3, cout, h, w, 0), x)
    _abi.call("mde_conv3x3_wgrad", _abi.ptr(gy), _abi.ptr(x), _abi.ptr(gw), n, 3, cout, h, w,
              _abi.ptr(ws), 0, _abi.stream_of(x))
    return gw


def _wgrad_deferred(g, y, tab, x, n, cout, h, w):
    from monocular_depth_estimation_amd import _abi
    gw = torch.empty((cout, 3, 3, 3), device=DEV)
    ws = _ws(_abi.query("mde_conv3x3_wgrad_workspace", n, 3, cout, h, w, 0), x)
    _abi.call("mde_conv3x3_wgrad_bn_deferred", _abi.ptr(g), _abi.ptr(y), _abi.ptr(tab), _abi.ptr(x),
              _abi.ptr(gw), n, 3, cout, h, w, _abi.ptr(ws), 0, _abi.stream_of(x))
    return gw


def _params(c):
    return {k: torch.empty(c, device=DEV) for k in ("gg", "gb", "gpb")}


def _entry_case(cout, n, h, w):
    """(today's pair, the deferred entry): gweight and the BatchNorm's parameter gradients."""
    from monocular_depth_estimation_amd import _abi
    assert _abi.query("mde_conv3x3_wgrad_bn_deferred_supported", n, 3, cout, h, w) == 1
    t = _inputs(cout, n, h, w)
    st = _abi.stream_of(t["x"])

    def bn():  # fresh per call: the guard harness tracks pointers call by call
        return [_abi.ptr(t[k]) for k in ("gamma", "beta", "mean", "invstd")]

    old, new = _params(cout), _params(cout)
    gy = torch.empty_like(t["y"])
    _abi.call("mde_batchnorm_bwd_apply", _abi.ptr(t["g"]), _abi.ptr(t["y"]), None, *bn(), 1,
              _abi.ptr(t["sums"]), _abi.ptr(gy), None, _abi.ptr(old["gg"]), _abi.ptr(old["gb"]),
              _abi.ptr(old["gpb"]), n, cout, h, w, 1, 0, st)
    old["gw"] = _wgrad(gy, t["x"], n, cout, h, w)
    tab = torch.empty((5, cout), device=DEV)
    _abi.call("mde_batchnorm_bwd_coef", *bn(), 1, _abi.ptr(t["sums"]), _abi.ptr(tab),
              _abi.ptr(new["gg"]), _abi.ptr(new["gb"]), _abi.ptr(new["gpb"]), n, cout, h, w, st)
    new["gw"] = _wgrad_deferred(t["g"], t["y"], tab, t["x"], n, cout, h, w)
    torch.cuda.synchronize()
    return old, new


def _reduce_case():
    """c = 64 (up_1: the 1x1 backward delivers no sums): mde_batchnorm_bwd's
    reduce + apply -> mde_conv3x3_wgrad vs mde_batchnorm_bwd_reduce_coef -> the
    deferred entry."""
    from monocular_depth_estimation_amd import _abi
    cout, n, h, w = 64, 2, 16, 64
    t = _inputs(cout, n, h, w)
    st = _abi.stream_of(t["x"])

    def bn():  # fresh per call: the guard harness tracks pointers call by call
        return [_abi.ptr(t[k]) for k in ("gamma", "beta", "mean", "invstd")]

    old, new = _params(cout), _params(cout)
    gy = torch.empty_like(t["y"])
    ws = _ws(_abi.query("mde_batchnorm_workspace", n, cout, h, w), t["y"])
    _abi.call("mde_batchnorm_bwd", _abi.ptr(t["g"]), _abi.ptr(t["y"]), None, *bn(), 1, _abi.ptr(gy),
              None, _abi.ptr(old["gg"]), _abi.ptr(old["gb"]), _abi.ptr(old["gpb"]), n, cout, h, w, 1,
              _abi.ptr(ws), 0, st)
    old["gw"] = _wgrad(gy, t["x"], n, cout, h, w)
    tab = torch.empty((5, cout), device=DEV)
    ws2 = _ws(_abi.query("mde_batchnorm_workspace", n, cout, h, w), t["y"])
    _abi.call("mde_batchnorm_bwd_reduce_coef", _abi.ptr(t["g"]), _abi.ptr(t["y"]), *bn(), 1,
              _abi.ptr(tab), _abi.ptr(new["gg"]), _abi.ptr(new["gb"]), _abi.ptr(new["gpb"]), n, cout,
              h, w, 1, _abi.ptr(ws2), 0, st)
    new["gw"] = _wgrad_deferred(t["g"], t["y"], tab, t["x"], n, cout, h, w)
    torch.cuda.synchronize()
    return old, new


def _same(old, new, what):
    diff = [k for k in old if not torch.equal(old[k], new[k])]
    assert not diff, f"{what}: not bit-identical to today's pair: {diff}"
    assert bool(torch.isfinite(old["gw"]).all()) and bool(old["gw"].abs().max() > 0), what


@pytest.mark.parametrize("n,h,w", SIZES)
@pytest.mark.parametrize("cout", COUTS)
def test_entry_vs_apply_then_wgrad(cout, n, h, w):
    _same(*_entry_case(cout, n, h, w), f"3->{cout} n{n} {h}x{w}")


def test_reduce_coef_vs_batchnorm_bwd():
    _same(*_reduce_case(), "reduce_coef c64")


def test_under_guard():
    """Guard bands, poisoned outputs and scratch (tests/_abi_guard.py) around
    every case above; the results equal today's pair there too."""
    from monocular_depth_estimation_amd import _abi
    from tests._abi_guard import guarded_abi
    with guarded_abi(signatures={**_abi.SIGNATURES, **_abi.WGRAD_FOLD_SIGNATURES}) as guard:
        cases = [(f"3->{c} n{n} {h}x{w}", _entry_case(c, n, h, w)) for c in COUTS
                 for n, h, w in SIZES]
        cases.append(("reduce_coef c64", _reduce_case()))
    for name in NEW:
        assert guard.calls[name] > 0, name
    assert guard.calls["mde_conv3x3_wgrad_bn_deferred"] == len(cases)
    for what, (old, new) in cases:
        _same(old, new, what)


# ---------------------------------------------------------------- block, model
def _spy(monkeypatch):
    from monocular_depth_estimation_amd import _abi
    calls = []
    real = _abi.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)

    monkeypatch.setattr(_abi, "call", spy)
    return calls


def _block_run(n, h, w, guide_grad=False):
    """One Guided_Upsampling_Block(16, 16, 1) train step: gradients and the launch
    registry's (launches, algorithmic bytes) per id."""
    from monocular_depth_estimation_amd import _abi
    from monocular_depth_estimation_amd.GuideDepth.model.modules import Guided_Upsampling_Block
    from oracle.weights import fill_
    gen = torch.Generator().manual_seed(9)
    blk = fill_(Guided_Upsampling_Block(16, 16, 1)).to(DEV).train()
    guide = torch.rand((n, 3, h, w), generator=gen).to(DEV).requires_grad_(guide_grad)
    depth = (torch.rand((n, 16, h, w), generator=gen) - 0.3).to(DEV).requires_grad_(True)
    gy = (torch.rand((n, 1, h, w), generator=gen) - 0.5).to(DEV)
    _abi.timing_enable(True)
    _abi.timing_reset()
    try:
        blk(guide, depth).backward(gy)
        torch.cuda.synchronize()
        reg = {k: (v[1], v[2]) for k, v in _abi.timing_collect().items()}
    finally:
        _abi.timing_enable(False)
        _abi.timing_reset()
    grads = {k: p.grad.clone() for k, p in blk.named_parameters()}
    grads["depth"] = depth.grad.clone()
    return grads, reg


def test_unsupported_size_keeps_the_apply_pass(monkeypatch):
    from monocular_depth_estimation_amd import _abi
    for cout in COUTS:
        assert _abi.query("mde_conv3x3_wgrad_bn_deferred_supported", 2, 3, cout, 8, 16) == 0
    calls = _spy(monkeypatch)
    _block_run(2, 8, 16)
    assert "mde_batchnorm_bwd_apply" in calls and "mde_conv3x3_wgrad" in calls
    assert not set(calls) & set(_abi.WGRAD_FOLD_SIGNATURES)


def test_block_switch_on_off(monkeypatch):
    from monocular_depth_estimation_amd import _abi
    calls = _spy(monkeypatch)
    monkeypatch.setenv("MDE_GUIDE_WGRAD_FOLD", "0")
    g0, r0 = _block_run(2, 32, 32)
    assert not set(calls) & set(_abi.WGRAD_FOLD_SIGNATURES)
    del calls[:]
    monkeypatch.setenv("MDE_GUIDE_WGRAD_FOLD", "1")
    g1, r1 = _block_run(2, 32, 32)
    assert calls.count("mde_conv3x3_wgrad_bn_deferred") == 1
    assert set(g0) == set(g1)
    diff = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not diff, diff
    print("off:", r0, "\non:", r1)
    assert r0["bn_bwd_apply"][0] - r1["bn_bwd_apply"][0] == 1
    assert r1.get("bn_bwd_final", (0, 0))[0] - r0.get("bn_bwd_final", (0, 0))[0] == 1
    assert r1["bn_bwd_apply"][1] < r0["bn_bwd_apply"][1]
    assert r1["conv3x3_wgrad_guide"][0] == r0["conv3x3_wgrad_guide"][0]
    # a guide that needs a gradient: d/dy1 has a second reader, nothing is routed
    del calls[:]
    _block_run(2, 32, 32, guide_grad=True)
    assert not set(calls) & set(_abi.WGRAD_FOLD_SIGNATURES)
    assert "mde_batchnorm_bwd_apply" in calls and "mde_conv3x3_wgrad" in calls


def _model_step():
    """One GuideDepth train step at 128x128, bs 1: up_1's guide plane is 32 x 32
    = 1024, so all three guide sites route."""
    import monocular_depth_estimation_amd as mde
    from oracle.weights import fill_, seeded
    x = torch.from_numpy(seeded((1, 3, 128, 128), 7, 0, 1)).to(DEV)
    d = torch.from_numpy(seeded((1, 1, 128, 128), 8, 0.1, 10.0)).to(DEV)
    model = fill_(mde.GuideDepth(pretrained=False)).to(DEV).train()
    loss = mde.SSIML1(1.0, 0.1)(model(x), d)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


def test_model_step_switch_on_off(monkeypatch):
    from monocular_depth_estimation_amd import _abi
    # MIOpen's default solvers for the encoder's convolutions are not
    # run-to-run deterministic (bench.py --dump-outputs selects these too)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    calls = _spy(monkeypatch)
    monkeypatch.setenv("MDE_GUIDE_WGRAD_FOLD", "0")
    _model_step()  # MIOpen picks (and builds) its solvers on a shape's first call
    del calls[:]
    l0, g0 = _model_step()
    assert not set(calls) & set(_abi.WGRAD_FOLD_SIGNATURES)
    del calls[:]
    monkeypatch.setenv("MDE_GUIDE_WGRAD_FOLD", "1")
    l1, g1 = _model_step()
    assert calls.count("mde_conv3x3_wgrad_bn_deferred") == 3
    assert calls.count("mde_batchnorm_bwd_reduce_coef") == 1
    assert torch.equal(l0, l1)
    diff = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not diff, diff
