"""The 1x1 conv backward with a DEFERRED incoming gradient
(mde_pointwise_bwd_bn_deferred) against the pair it replaces: the BatchNorm /
SE-over-BatchNorm backward's apply pass followed by mde_pointwise_bwd_bn.

Tolerance (none hard-coded): every compared quantity is also computed in
float64 with plain torch ops from the same inputs (the upstream gradient, the
conv's own output, the kernels' fp32 tables cast to double); the separate
pair's max error against that, relative to the float64 result's max magnitude
(`rel_err` of tests/test_gpu_wino.py), is the yardstick, and the fused entry
must stay within 2 x it -- an equally valid fp32 evaluation order may land
either side of the old one.

gprebias (d/d of a conv bias folded in front of a training-mode BatchNorm) is
identically zero analytically; the kernels form it in double as a sum of
cancelling terms of magnitude |A sum dy'|, so its float64 "result" is rounding
noise and no scale.  For it alone the errors are taken relative to that term
magnitude, with a floor of one fp32 ulp (2^-24: the stored format's precision)
under the 2 x rule.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ws(nbytes, like):
    """The product's workspace helper: exactly the queried size, 1-D uint8."""
    from monocular_depth_estimation_amd.functional import _ws as ws
    return ws(nbytes, like)


SHAPES = [(16, 16), (16, 8), (32, 32), (32, 16)]  # the routed (cin, cout); cin 64 keeps the apply pass
# (n, h, w): one tile per image (fewer tiles than a block's waves: the clamped
# tail load); 9 tiles (odd count through the two-set unrolled loop); the size
# of the SE channel-slice case
SIZES = [(2, 8, 8), (3, 8, 24), (2, 8, 16)]
ULP32 = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    import monocular_depth_estimation_amd  # noqa: F401


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _bn_coefs(x, gamma, beta):
    mean = x.mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(x.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    scale = gamma * invstd
    return mean, invstd, scale, beta - mean * scale


def _bc(v):
    return v.double().view(1, -1, 1, 1)


class _Conv:
    """The 1x1 conv under test with its input BatchNorm (BN1): y1, weights,
    coefficients, workspace; `tail` runs BN1's apply pass from the sums."""

    def __init__(self, gen, n, cin, cout, h, w):
        from monocular_depth_estimation_amd import _abi
        self.dims = (n, cin, cout, h, w)
        f = dict(device=DEV, dtype=torch.float32)
        self.y1 = (torch.rand((n, cin, h, w), generator=gen) * 2 - 0.7).to(DEV)
        self.w2 = (torch.rand((cout, cin), generator=gen) - 0.5).to(DEV)
        self.gamma = (torch.rand(cin, generator=gen) + 0.5).to(DEV)
        self.beta = (torch.rand(cin, generator=gen) - 0.5).to(DEV)
        self.mean, self.invstd, self.scale, self.shift = _bn_coefs(self.y1, self.gamma, self.beta)
        self.ws = _ws(_abi.query("mde_pointwise_workspace", n, cin, cout, h, w), self.y1)

    def outputs(self):
        n, cin, cout, h, w = self.dims
        f = dict(device=DEV, dtype=torch.float32)
        return dict(gs=torch.empty_like(self.y1), gw=torch.empty_like(self.w2),
                    sums=torch.empty((cin, 2), **f), gy1=torch.empty_like(self.y1),
                    gg1=torch.empty(cin, **f), gb1=torch.empty(cin, **f), gpb1=torch.empty(cin, **f))

    def separate(self, gy):
        from monocular_depth_estimation_amd import _abi
        n, cin, cout, h, w = self.dims
        o = self.outputs()
        _abi.call("mde_pointwise_bwd_bn", _abi.ptr(gy), _abi.ptr(self.y1), _abi.ptr(self.scale),
                  _abi.ptr(self.shift), _abi.ptr(self.mean), _abi.ptr(self.w2), _abi.ptr(o["gs"]),
                  _abi.ptr(o["gw"]), _abi.ptr(o["sums"]), n, cin, cout, h, w, _abi.ptr(self.ws), 0,
                  _abi.stream_of(gy))
        return self.tail(o)

    def deferred(self, g_raw, choff, y_out, tab, s=None, dm=None):
        from monocular_depth_estimation_amd import _abi
        n, cin, cout, h, w = self.dims
        o = self.outputs()
        _abi.call("mde_pointwise_bwd_bn_deferred", _abi.ptr(g_raw), g_raw.shape[1], choff,
                  _abi.ptr(y_out), _abi.ptr(tab), _abi.ptr(s), _abi.ptr(dm), _abi.ptr(self.y1),
                  _abi.ptr(self.scale), _abi.ptr(self.shift), _abi.ptr(self.mean),
                  _abi.ptr(self.w2), _abi.ptr(o["gs"]), _abi.ptr(o["gw"]), _abi.ptr(o["sums"]), n,
                  cin, cout, h, w, _abi.ptr(self.ws), 0, _abi.stream_of(g_raw))
        return self.tail(o)

    def tail(self, o):
        from monocular_depth_estimation_amd import _abi
        n, cin, cout, h, w = self.dims
        _abi.call("mde_batchnorm_bwd_apply", _abi.ptr(o["gs"]), _abi.ptr(self.y1), None,
                  _abi.ptr(self.gamma), _abi.ptr(self.beta), _abi.ptr(self.mean),
                  _abi.ptr(self.invstd), 1, _abi.ptr(o["sums"]), _abi.ptr(o["gy1"]), None,
                  _abi.ptr(o["gg1"]), _abi.ptr(o["gb1"]), _abi.ptr(o["gpb1"]), n, cin, h, w, 1, 0,
                  _abi.stream_of(self.y1))
        return o

    def reference(self, G):
        """float64: gs = W^T G, gW = G relu(bn1(y1))^T, BN1's sums and parameter
        gradients; `gpb1_scale` is the magnitude of gprebias's cancelling terms."""
        n = self.dims[0] * self.dims[3] * self.dims[4]
        W, y1 = self.w2.double(), self.y1.double()
        z = y1 * _bc(self.scale) + _bc(self.shift)
        gs = torch.einsum("oc,nohw->nchw", W, G)
        gw = torch.einsum("nohw,nchw->oc", G, z.clamp_min(0.0))
        e = gs * (z > 0)
        s1 = e.sum(dim=(0, 2, 3))
        s2 = (e * (y1 - _bc(self.mean))).sum(dim=(0, 2, 3))
        is_, mu, sc = self.invstd.double(), self.mean.double(), self.scale.double()
        B = -sc * is_ * is_ * s2 / n
        D = -sc * s1 / n - B * mu
        return dict(gs=gs, gw=gw, sums=torch.stack([s1, s2], 1), gg1=s2 * is_, gb1=s1,
                    gy1=_bc(sc) * e + _bc(B) * y1 + _bc(D), gpb1=torch.zeros_like(s1),
                    gpb1_scale=float((sc * s1).abs().max()))


def _check(old, new, ref, what, exact=False):
    """fused error <= 2 x the separate pair's error, each against float64;
    exact: also every output bit for bit the separate pair's."""
    if exact:
        diff = [k for k in old if not torch.equal(old[k], new[k])]
        assert not diff, f"{what}: not bit-identical to the separate pair: {diff}"
    report = {}
    for k in old:
        if k.startswith("gpb"):  # analytically zero: see the module docstring
            scale = max(ref[k + "_scale"], 1e-30)
            eo = float((old[k].double() - ref[k]).abs().max()) / scale
            en = float((new[k].double() - ref[k]).abs().max()) / scale
        else:
            eo, en = rel_err(old[k], ref[k]), rel_err(new[k], ref[k])
        report[k] = (eo, en)
        print(f"{what} {k}: separate {eo:.3e} fused {en:.3e}")
    bad = {k: v for k, v in report.items()
           if v[1] > (max(2.0 * v[0], ULP32) if k.startswith("gpb") else 2.0 * v[0])}
    assert not bad, f"{what}: fused error above 2 x the separate pair's: {bad}"


# h w >= 1024: the BatchNorm apply pass runs its plane kernel, the one the
# full-size decoder blocks use.  The deferred entry repeats that kernel's (and
# the SE apply kernel's) fp32 operations one for one, so there every output is
# bit-identical -- which a training run needs to stay on the same trajectory
# (Adam grows a 1e-7 difference to 1e-4 of the loss within a few steps).
EXACT_SIZE = (2, 16, 64)


@pytest.mark.parametrize("n,h,w", SIZES)
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_bn_form_fused_vs_separate(cin, cout, n, h, w):
    """The comb branch: gs -> [mde_batchnorm_bwd_apply -> gr -> mde_pointwise_bwd_bn]
    vs mde_batchnorm_bwd_coef + mde_pointwise_bwd_bn_deferred(gs, r, tab)."""
    _bn_case(cin, cout, n, h, w)


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_bn_form_bit_identical_at_plane_size(cin, cout):
    _bn_case(cin, cout, *EXACT_SIZE, exact=True)


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_se_form_bit_identical_at_plane_size(cin, cout):
    _se_case(cin, cout, *EXACT_SIZE, exact=True)


def _bn_case(cin, cout, n, h, w, exact=False):
    from monocular_depth_estimation_amd import _abi
    assert _abi.query("mde_pointwise_deferred_supported", cin, cout, h, w) == 1
    gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + h * w)
    f = dict(device=DEV, dtype=torch.float32)
    conv = _Conv(gen, n, cin, cout, h, w)
    r = (torch.rand((n, cout, h, w), generator=gen) * 2 - 0.8).to(DEV)   # the conv's output
    gs2 = (torch.rand((n, cout, h, w), generator=gen) - 0.5).to(DEV)     # upstream of BN2's apply
    gamma2 = (torch.rand(cout, generator=gen) + 0.5).to(DEV)
    beta2 = (torch.rand(cout, generator=gen) - 0.5).to(DEV)
    mean2, invstd2, scale2, shift2 = _bn_coefs(r, gamma2, beta2)
    e2 = gs2 * ((r * scale2.view(1, -1, 1, 1) + shift2.view(1, -1, 1, 1)) > 0)
    sums2 = torch.stack([e2.sum(dim=(0, 2, 3)),
                         (e2 * (r - mean2.view(1, -1, 1, 1))).sum(dim=(0, 2, 3))], 1).contiguous()
    st = _abi.stream_of(r)
    # separate: BN2's apply pass writes gr, the conv backward reads it
    gr = torch.empty_like(r)
    bn2_old = {k: torch.empty(cout, **f) for k in ("gg2", "gb2", "gpb2")}
    _abi.call("mde_batchnorm_bwd_apply", _abi.ptr(gs2), _abi.ptr(r), None, _abi.ptr(gamma2),
              _abi.ptr(beta2), _abi.ptr(mean2), _abi.ptr(invstd2), 1, _abi.ptr(sums2), _abi.ptr(gr),
              None, _abi.ptr(bn2_old["gg2"]), _abi.ptr(bn2_old["gb2"]), _abi.ptr(bn2_old["gpb2"]), n,
              cout, h, w, 1, 0, st)
    old = conv.separate(gr)
    old.update(bn2_old)
    # fused: coefficients only, the conv backward forms gr in registers
    tab = torch.empty((5, cout), **f)
    bn2_new = {k: torch.empty(cout, **f) for k in ("gg2", "gb2", "gpb2")}
    _abi.call("mde_batchnorm_bwd_coef", _abi.ptr(gamma2), _abi.ptr(beta2), _abi.ptr(mean2),
              _abi.ptr(invstd2), 1, _abi.ptr(sums2), _abi.ptr(tab), _abi.ptr(bn2_new["gg2"]),
              _abi.ptr(bn2_new["gb2"]), _abi.ptr(bn2_new["gpb2"]), n, cout, h, w, st)
    new = conv.deferred(gs2, 0, r, tab)
    new.update(bn2_new)
    torch.cuda.synchronize()
    # float64 from the same inputs (sums2 and the fp32 table are inputs)
    t = tab.double()
    z2 = r.double() * _bc(tab[0]) + _bc(tab[1])
    G = _bc(tab[2]) * (gs2.double() * (z2 > 0)) + _bc(tab[3]) * r.double() + _bc(tab[4])
    ref = conv.reference(G)
    s1, s2 = sums2[:, 0].double(), sums2[:, 1].double()
    ref.update(gg2=s2 * invstd2.double(), gb2=s1, gpb2=torch.zeros_like(s1),
               gpb2_scale=float((t[2] * s1).abs().max()))
    _check(old, new, ref, f"bn {cin}->{cout} n{n} {h}x{w}", exact)


@pytest.mark.parametrize("n,h,w", SIZES)
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_se_form_fused_vs_separate(cin, cout, n, h, w):
    """The feature / guide branches: mde_se_bn_bwd (writes gya | gyb) + two
    mde_pointwise_bwd_bn vs mde_se_bn_bwd_coef + two deferred conv backwards
    reading channels [0, ca) and [ca, c) of the SE gradient in place (the
    second one the non-zero channel offset into a wider g_raw)."""
    _se_case(cin, cout, n, h, w)


def _se_case(cin, cout, n, h, w, exact=False):
    from monocular_depth_estimation_amd import _abi
    gen = torch.Generator().manual_seed(77 * cin + 3 * cout + h * w)
    f = dict(device=DEV, dtype=torch.float32)
    ca = cb = cout
    c = cr = ca + cb
    convs = [_Conv(gen, n, cin, cout, h, w) for _ in range(2)]
    ys = [(torch.rand((n, cout, h, w), generator=gen) * 2 - 0.8).to(DEV) for _ in range(2)]
    gout = (torch.rand((n, c, h, w), generator=gen) - 0.5).to(DEV)
    gamma = (torch.rand(c, generator=gen) + 0.5).to(DEV)
    beta = (torch.rand(c, generator=gen) - 0.5).to(DEV)
    w1 = ((torch.rand((cr, c), generator=gen) - 0.5) * 0.5).to(DEV)
    w2 = ((torch.rand((c, cr), generator=gen) - 0.5) * 0.5).to(DEV)
    mean, invstd, scale, shift = _bn_coefs(torch.cat(ys, 1), gamma, beta)
    st = _abi.stream_of(gout)
    ws = _ws(_abi.query("mde_se_bn_workspace", n, c, cr, h, w), gout)
    out = torch.empty((n, c, h, w), **f)
    s, hidden, semean = torch.empty((n, c), **f), torch.empty((n, cr), **f), torch.empty((n, c), **f)
    _abi.call("mde_se_bn_fwd", _abi.ptr(ys[0]), ca, _abi.ptr(ys[1]), cb, _abi.ptr(scale),
              _abi.ptr(shift), _abi.ptr(w1), _abi.ptr(w2), cr, _abi.ptr(out), _abi.ptr(s),
              _abi.ptr(hidden), _abi.ptr(semean), n, h, w, _abi.ptr(ws), 0, st)

    def se_outputs():
        return dict(gg2=torch.empty(c, **f), gb2=torch.empty(c, **f), gw1=torch.empty_like(w1),
                    gw2=torch.empty_like(w2))

    # separate
    gys = [torch.empty_like(y) for y in ys]
    se_old = se_outputs()
    _abi.call("mde_se_bn_bwd", _abi.ptr(gout), _abi.ptr(ys[0]), ca, _abi.ptr(ys[1]), cb,
              _abi.ptr(scale), _abi.ptr(shift), _abi.ptr(mean), _abi.ptr(invstd), 1, _abi.ptr(w1),
              _abi.ptr(w2), cr, _abi.ptr(s), _abi.ptr(hidden), _abi.ptr(semean), _abi.ptr(gys[0]),
              _abi.ptr(gys[1]), _abi.ptr(se_old["gg2"]), _abi.ptr(se_old["gb2"]),
              _abi.ptr(se_old["gw1"]), _abi.ptr(se_old["gw2"]), n, h, w, _abi.ptr(ws), 0, st)
    olds = [convs[i].separate(gys[i]) for i in range(2)]
    # fused
    dm, tab = torch.empty((n, c), **f), torch.empty((5, c), **f)
    se_new = se_outputs()
    _abi.call("mde_se_bn_bwd_coef", _abi.ptr(gout), _abi.ptr(ys[0]), ca, _abi.ptr(ys[1]), cb,
              _abi.ptr(scale), _abi.ptr(shift), _abi.ptr(mean), _abi.ptr(invstd), 1, _abi.ptr(w1),
              _abi.ptr(w2), cr, _abi.ptr(s), _abi.ptr(hidden), _abi.ptr(semean), _abi.ptr(dm),
              _abi.ptr(tab), _abi.ptr(se_new["gg2"]), _abi.ptr(se_new["gb2"]),
              _abi.ptr(se_new["gw1"]), _abi.ptr(se_new["gw2"]), n, h, w, _abi.ptr(ws), 0, st)
    news = [convs[i].deferred(gout, i * ca, ys[i], tab, s, dm) for i in range(2)]
    torch.cuda.synchronize()
    # the SE part itself is the same launches either way
    for k in se_old:
        assert torch.equal(se_old[k], se_new[k]), k
    # float64 from the same inputs (s, dm and the fp32 table are inputs)
    t, sd, dmd = tab.double(), s.double(), dm.double()
    y = torch.cat(ys, 1).double()
    z = y * _bc(t[0]) + _bc(t[1])
    P = (_bc(t[0]) * sd.view(n, c, 1, 1))
    Q = (_bc(t[0]) * dmd.view(n, c, 1, 1)) / (h * w)
    G = (z > 0) * (P * gout.double() + Q) + _bc(t[3]) * (y - _bc(t[2])) + _bc(t[4])
    for i in range(2):
        ref = convs[i].reference(G[:, i * ca:(i + 1) * ca])
        _check(olds[i], news[i], ref, f"se[{i}] {cin}->{cout} n{n} {h}x{w}", exact)


def _block_inputs(out_features, n, h, w):
    gen = torch.Generator().manual_seed(9)
    guide = torch.rand((n, 3, h, w), generator=gen)
    depth = torch.rand((n, 16, h, w), generator=gen) - 0.3
    gy = torch.rand((n, out_features, h, w), generator=gen) - 0.5
    return guide, depth, gy


def _block_reference(out_features, n, h, w):
    """The same block and inputs in float64 with plain torch ops (the CPU oracle)."""
    from oracle import guidedepth as og
    from oracle.weights import fill_
    blk = fill_(og.GuidedUpsamplingBlock(16, 16, out_features)).double().train()
    guide, depth, gy = (t.double() for t in _block_inputs(out_features, n, h, w))
    guide.requires_grad_(True)
    depth.requires_grad_(True)
    blk(guide, depth).backward(gy)
    grads = {k: p.grad for k, p in blk.named_parameters()}
    grads["guide"], grads["depth"] = guide.grad, depth.grad
    return grads


def _block_case(out_features, n, h, w):
    """One Guided_Upsampling_Block(16, 16, out) train step's gradients and the
    launch registry's counts."""
    from monocular_depth_estimation_amd import _abi
    from monocular_depth_estimation_amd.GuideDepth.model.modules import Guided_Upsampling_Block
    from oracle.weights import fill_
    blk = fill_(Guided_Upsampling_Block(16, 16, out_features)).to(DEV).train()
    guide, depth, gy = (t.to(DEV) for t in _block_inputs(out_features, n, h, w))
    guide.requires_grad_(True)
    depth.requires_grad_(True)
    _abi.timing_enable(True)
    _abi.timing_reset()
    try:
        blk(guide, depth).backward(gy)
        torch.cuda.synchronize()
        counts = {k: v[1] for k, v in _abi.timing_collect().items()}
    finally:
        _abi.timing_enable(False)
        _abi.timing_reset()
    grads = {k: p.grad.clone() for k, p in blk.named_parameters()}
    grads["guide"], grads["depth"] = guide.grad.clone(), depth.grad.clone()
    return grads, counts


def _block_compare(g0, g1, ref):
    """g1 (deferred) within 2 x the error of g0 (apply pass) against the float64 ref."""
    assert set(g0) == set(g1) == set(ref)
    bad = {}
    for k in sorted(ref):
        if "_conv." in k and k.endswith(".bias") and ".1." not in k and ".4." not in k:
            # a conv bias in front of a train-mode BatchNorm: identically zero
            # gradient, the float64 value is rounding noise -> errors relative
            # to that conv's weight gradient, floor one fp32 ulp
            scale = float(ref[k[:-4] + "weight"].abs().max())
            eo = float((g0[k].double().cpu() - ref[k]).abs().max()) / scale
            en = float((g1[k].double().cpu() - ref[k]).abs().max()) / scale
            bound = max(2.0 * eo, ULP32)
        else:
            eo, en = rel_err(g0[k], ref[k]), rel_err(g1[k], ref[k])
            bound = 2.0 * eo
        print(f"{k}: apply-pass {eo:.3e} deferred {en:.3e}")
        if en > bound:
            bad[k] = (eo, en)
    assert not bad, f"deferred error above 2 x the apply-pass path's: {bad}"


@pytest.mark.parametrize("out_features", [8, 1])
def test_block_deferred_vs_apply_pass(out_features, monkeypatch):
    """Guided_Upsampling_Block (in = expand = 16) backward with MDE_PW_DEFER=1 vs
    0: all parameter gradients and both input gradients within 2 x the
    MDE_PW_DEFER=0 path's own error against the float64 oracle, and the launch
    registry shows the fused run issued no se_bwd_apply launch, and one
    bn_bwd_apply launch fewer where the comb branch is on the fused skip path
    (out = 1, up_3's block; mde_skip_reduce_bn has no 16 -> 8 kernel, so at
    out = 8 the comb BatchNorm keeps its own pass and only the SE fold runs)."""
    from monocular_depth_estimation_amd import _abi
    n, h, w = 2, 8, 16  # h w % 64 == 0: the smallest the pointwise kernels take
    assert _abi.query("mde_pointwise_supported", 16, 8, h, w) == 1
    assert _abi.query("mde_pointwise_supported", 16, 16, h, w) == 1
    assert _abi.query("mde_pointwise_deferred_supported", 16, 8, h, w) == 1
    assert _abi.query("mde_pointwise_deferred_supported", 16, 16, h, w) == 1
    comb = _abi.query("mde_skip_reduce_bn_supported", 16, out_features, h, w, 1)
    assert comb == (1 if out_features == 1 else 0)
    monkeypatch.setenv("MDE_PW_DEFER", "0")
    g0, c0 = _block_case(out_features, n, h, w)
    monkeypatch.setenv("MDE_PW_DEFER", "1")
    g1, c1 = _block_case(out_features, n, h, w)

    def applies(c):
        return c.get("bn_bwd_apply", 0) + c.get("bn_bwd_apply_small", 0)

    print("launches off:", c0, "\nlaunches on:", c1)
    assert c0.get("se_bwd_apply", 0) == 1 and c1.get("se_bwd_apply", 0) == 0
    assert applies(c0) - applies(c1) == comb
    assert c1.get("bn_bwd_final", 0) - c0.get("bn_bwd_final", 0) == comb
    _block_compare(g0, g1, _block_reference(out_features, n, h, w))
