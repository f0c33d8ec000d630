"""The paths of csrc/attn.hip that the decoder goldens (window 7, shifts 0 and 3,
at most 60 windows) never take, against the float64 reference of
tests/_attn_cases.py: the generic-window kernel instances (window != 7), window 7
at its untested shifts / single window row / idle waves, and the backward's loop
over several windows per block -- chosen by the kernel itself at two large
shapes, and forced with MDE_ATTN_BWD_WPB in a fresh process at small ones.

Tolerances are the kernel's existing ones (test_window_attention_vs_oracle):
output 1e-5, every gradient 1e-4, scale-relative."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _attn_cases as ac

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    import monocular_depth_estimation_amd  # noqa: F401  (loads libmde_hip.so, raises if absent)


def _check(case, v_bias=False):
    b, h, w, heads, ws, shift = case
    got = ac.run_kernel(*case, v_bias=v_bias)
    ref = ac.reference(*case, v_bias)
    ac.close_scaled(got["out"], ref["out"], 1e-5, "out")
    x = ac.make_inputs(*case, v_bias)
    for name in ac.GRADS:
        if ref[name] is None:
            assert got[name] is None, name
        elif ws == 1 and name in ("gqk", "gqk_bias", "gtable"):
            # One key per query: P = 1 and every dS = P (dP - sum P dP) is 0, so these
            # three are 0 and a relative bound says nothing.  |dP| <= 32 |gout| |v|, so
            # a rounding residue in dS is far below 1e-6 |gout|max |v|max: the bound of
            # the table (a sum of dS); gqk = dS k / sqrt(32) scales with |qk|max.
            bound = 1e-6 * float(x["gout"].abs().max()) * float(x["v"].abs().max())
            if name != "gtable":
                bound *= max(1.0, float(x["qk"].abs().max()))
            err = float(got[name].abs().max())
            print(f"{name}: |max| {err:.3g} bound {bound:.3g}")
            assert float(ref[name].abs().max()) == 0.0 and err <= bound, (name, err, bound)
        else:
            ac.close_scaled(got[name], ref[name], 1e-4, name)


@pytest.mark.parametrize("b,h,w,heads,ws,shift", ac.GENERIC_CASES)
def test_generic_window(b, h, w, heads, ws, shift):
    """wattn_fwd_kernel<0> / wattn_bwd_kernel<0>: the full 64 x 67 tile, the window
    size at run time; ws 8 fills all 64 token slots and 225 of 256 table slots."""
    _check((b, h, w, heads, ws, shift))


@pytest.mark.parametrize("b,h,w,heads,ws,shift", ac.VBIAS_CASES)
def test_generic_window_v_bias(b, h, w, heads, ws, shift):
    """The SAM form on the generic instances: a padded token's v is v_bias."""
    _check((b, h, w, heads, ws, shift), v_bias=True)


@pytest.mark.parametrize("b,h,w,heads,ws,shift", ac.WS7_EDGE_CASES)
def test_window7_edges(b, h, w, heads, ws, shift):
    _check((b, h, w, heads, ws, shift))


@pytest.mark.parametrize("b,h,w,heads,ws,shift", ac.NATURAL_WPB_CASES)
def test_backward_several_windows_per_block(b, h, w, heads, ws, shift):
    """Shapes with more than 8 rounds of resident blocks (LDS holds 3 blocks of the
    7 x 7 backward and 2 of the generic one on a CU), where windows_per_block gives
    each block several windows: the path of the bs16 C128 120 x 160 training stage.
    On a 256-CU MI355X: 6272 windows in 697 blocks and 4608 in 512, 9 per block."""
    nwin, nblk = ac.backward_blocks(b, h, w, heads, ws)
    print(f"nwin {nwin} nblk {nblk} wpb {-(-nwin // nblk)}")
    assert nblk < nwin, f"one window per block ({nwin} windows, {nblk} blocks): path not reached"
    _check((b, h, w, heads, ws, shift))


@pytest.mark.parametrize("b,h,w,heads,ws,shift", ac.BATCH_SPLIT_CASES)
def test_backward_window_loop_bitwise_vs_one_image(b, h, w, heads, ws, shift):
    """All four waves of a block at work, every CU full: the batch runs several
    windows per block, one image of it alone runs one (both asserted).  A window's
    output and data gradients depend on neither, so they are bitwise equal.  This
    is the case in which a wave can be a whole phase ahead of its block when the
    next window's token list is written (without the barrier at the top of the
    window loop the window-7 shape differs in gqk; the one-head shapes above and
    the small forced ones do not notice); no float64 reference at this size."""
    from monocular_depth_estimation_amd.newcrf_layers import window_attention
    nwin, nblk = ac.backward_blocks(b, h, w, heads, ws)
    assert nblk < nwin, f"batch: one window per block ({nwin} windows, {nblk} blocks)"
    nwin1, nblk1 = ac.backward_blocks(1, h, w, heads, ws)
    assert nblk1 == nwin1, f"one image: {nwin1} windows in {nblk1} blocks"
    c = heads * ac.HEAD_DIM
    gen = torch.Generator(device="cuda").manual_seed(h * w + ws)
    rnd = lambda shape, lo, hi: lo + (hi - lo) * torch.rand(shape, generator=gen, device="cuda")
    qk, v, gout = rnd((b, h * w, 2 * c), -2, 2), rnd((b, h, w, c), -1, 1), rnd((b, h * w, c), -1, 1)
    qk_bias, table = rnd((2 * c,), -1, 1), rnd(((2 * ws - 1) ** 2, heads), -1, 1)

    def run(lo, hi):
        q, u = qk[lo:hi].clone().requires_grad_(True), v[lo:hi].clone().requires_grad_(True)
        o = window_attention(q, qk_bias, u, table, h, w, heads, ws, shift)
        o.backward(gout[lo:hi])
        return o.detach(), q.grad, u.grad

    whole = run(0, b)
    for i in range(b):
        for name, a, one in zip(("out", "gqk", "gv"), whole, run(i, i + 1)):
            assert torch.equal(a[i:i + 1], one), f"image {i}: {name} differs from the image run alone"


def _child(case, out):
    """tests/_attn_wpb_child.py in a fresh process (MDE_ATTN_BWD_WPB is read once per
    process); any failure of it fails the test before anything else is launched."""
    b, h, w, heads, ws, shift, v_bias, wpb = case
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    env = dict(os.environ, MDE_ATTN_BWD_WPB=str(wpb))
    argv = [str(a) for a in (b, h, w, heads, ws, shift, int(v_bias), wpb)]
    try:
        p = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_attn_wpb_child.py"), *argv, out],
                           env=env, cwd=os.path.dirname(HERE), capture_output=True, text=True,
                           timeout=180)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"child timed out: {e.stdout} {e.stderr}")
    assert p.returncode == 0, f"child exit {p.returncode}:\n{(p.stdout + p.stderr)[-4000:]}"
    with np.load(out, allow_pickle=False) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.mark.parametrize("b,h,w,heads,ws,shift,v_bias,wpb", ac.FORCED_WPB_CASES)
def test_backward_forced_windows_per_block(b, h, w, heads, ws, shift, v_bias, wpb, tmp_path):
    """The window loop at small shapes, under guard (poisoned slab, guard bands
    around the smaller workspace).  Each window's data gradients do not depend on
    how windows are grouped into blocks: bitwise equal to one window per block.
    The table and bias gradients are a fixed-order sum: within tolerance of
    float64, and bitwise equal between two runs."""
    case = (b, h, w, heads, ws, shift)
    nwin, nblk = ac.backward_blocks(b, h, w, heads, ws)
    assert nblk == nwin, f"this process must run one window per block ({nwin}, {nblk})"
    own = ac.run_kernel(*case, v_bias=v_bias)
    first = _child(case + (v_bias, wpb), str(tmp_path / "a.npz"))
    second = _child(case + (v_bias, wpb), str(tmp_path / "b.npz"))
    ref = ac.reference(*case, v_bias)
    assert torch.equal(first["gqk"], own["gqk"]), "gqk depends on the grouping"
    assert torch.equal(first["gv"], own["gv"]), "gv depends on the grouping"
    names = ("gtable", "gqk_bias") + (("gv_bias",) if v_bias else ())
    for name in names:
        ac.close_scaled(first[name], ref[name], 1e-4, name)
        assert torch.equal(first[name], second[name]), f"{name}: two runs differ"
    assert torch.equal(first["gqk"], second["gqk"]) and torch.equal(first["gv"], second["gv"])
