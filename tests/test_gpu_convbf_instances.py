"""Every compiled instance of csrc/convbf.hip, and every patch-geometry edge of
its launchers, against float64: the cases of tests/_convbf_instance_cases.py
(tests/test_convbf_instances.py proves without a GPU that they reach every
instance id and edge).  The ABI entries are called directly, so no dispatch
threshold keeps a small plane away from its kernel, and each case first
asserts -- on this device, whose CU count moves `per` -- that the library's
query names the id and shows the properties it is listed for.

Oracle, bounds, guards: tests/_convbf_instance_check.py (those of
tests/test_gpu_convbf.py for the same kernels).  Every forward case also runs
the statistics epilogue (the STATS = true twin of its instance); every weight
gradient with more than one split runs twice, bitwise equal.

The three process-wide switches (MDE_CONVBF_RES=0, MDE_CONVBF_RESMODE=t21,
MDE_CONVBF_NW8=1) are read once per process: each runs the forward and
data-gradient lists, and the cases of the ids only it has, in one fresh child
(tests/_convbf_switch_child.py), one child at a time.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import _convbf_instance_cases as cc
from tests import _convbf_instance_check as ck

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("MDE_CONVBF_RES", "MDE_CONVBF_RESMODE", "MDE_CONVBF_NW8", "MDE_CONVBF_WBLOCKS")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    import monocular_depth_estimation_amd  # noqa: F401
    for name in SWITCHES:
        assert name not in os.environ, f"{name} is set: the case lists are for the defaults"


def _params(cases):
    return [pytest.param(shape, row, props, id=f"id{row}-" + "x".join(map(str, shape)))
            for shape, row, props in cases]


@pytest.mark.parametrize("shape,row,props", _params(cc.FWD_CASES))
def test_convbf_forward_instance_vs_float64(shape, row, props):
    ck.assert_listed(shape, 0, row, props)
    ck.run_forward(shape)


@pytest.mark.parametrize("shape,row,props", _params(cc.DGRAD_CASES))
def test_convbf_dgrad_instance_vs_float64(shape, row, props):
    ck.assert_listed(shape, 1, row, props)
    ck.run_dgrad(shape)


@pytest.mark.parametrize("shape,row,props", _params(cc.WGRAD_CASES))
def test_convbf_wgrad_instance_vs_float64(shape, row, props):
    info = ck.assert_listed(shape, 2, row, props)
    ck.run_wgrad(shape, info["blocks"])


@pytest.mark.parametrize("switch", sorted(cc.SWITCH_CASES))
def test_convbf_switch_in_a_fresh_process(switch, tmp_path):
    """One child under the switch: every forward / data-gradient case within
    the bounds, every id that exists only under the switch reached."""
    env, fwd, dgrad = cc.SWITCH_CASES[switch]
    out = str(tmp_path / "report.json")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    try:
        p = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_convbf_switch_child.py"), switch, out],
                           env=dict(os.environ, **env), cwd=os.path.dirname(HERE), capture_output=True,
                           text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"child timed out: {e.stdout} {e.stderr}")
    print(p.stdout[-6000:])
    assert p.returncode == 0, f"child exit {p.returncode}:\n{(p.stdout + p.stderr)[-4000:]}"
    with open(out) as f:
        report = json.load(f)
    assert len(report) == len(cc.FWD_CASES) + len(cc.DGRAD_CASES) + len(fwd) + len(dgrad)
    assert all(r["ok"] for r in report), [r for r in report if not r["ok"]]
    reached = {r["id"] for r in report}
    only = {row for _, row, _ in fwd + dgrad}
    assert only <= reached, f"{switch}: ids {sorted(only - reached)} not reached"
    for r in report:       # a switch-only case names the id it is listed for
        if r["want"] is not None:
            assert r["id"] == r["want"], r
    if switch == "res0":
        assert all(r["kernel"] == 1 for r in report), "MDE_CONVBF_RES=0 left a resident-filter launch"
    if switch == "t21":
        assert all(r["tw"] == 1 for r in report if r["kernel"] == 0), "t21 left a 256-pixel resident launch"
