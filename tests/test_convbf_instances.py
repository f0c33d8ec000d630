"""The case lists of tests/_convbf_instance_cases.py reach every compiled
instance of csrc/convbf.hip and every patch-geometry edge they are listed for
(no GPU: mde_convbf_instance is host arithmetic, the record the launchers
themselves switch on; with no device the CU count is the MI355X's 256).

A case removed, or a selection constant changed (a capacity, the tile widths,
the split targets) so that a listed case moves, fails here until the lists are
right again; tests/test_gpu_convbf_instances.py runs exactly these cases
against float64.
"""
import ctypes
import os
import re

import pytest

from tests import _convbf_instance_cases as cc
from tests._convbf_instance_check import assert_listed, family, properties, query
from tests.conftest import REPO

ALL = [(0, cc.FWD_CASES), (1, cc.DGRAD_CASES), (2, cc.WGRAD_CASES)]
SWITCHES = ("MDE_CONVBF_RES", "MDE_CONVBF_RESMODE", "MDE_CONVBF_NW8", "MDE_CONVBF_WBLOCKS")


def _lib():
    from monocular_depth_estimation_amd import _abi
    return _abi.load()


@pytest.fixture(autouse=True)
def _switches_unset():
    # read once per process by the library: the lists are for the default selection
    for name in SWITCHES:
        assert name not in os.environ, f"{name} is set: the case lists are for the defaults"


def _params():
    return [pytest.param(p, shape, row, props, id=f"pass{p}-id{row}-" + "x".join(map(str, shape)))
            for p, cases in ALL for shape, row, props in cases]


def test_info_fields_match_the_header():
    from monocular_depth_estimation_amd import _abi
    text = open(os.path.join(REPO, "include", "mde_abi.h")).read()
    assert int(re.search(r"#define MDE_CONVBF_INFO_LEN (\d+)", text).group(1)) == _abi.CONVBF_INFO_LEN
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define MDE_CBF_I_(\w+) (\d+)", text)}
    assert idx == {name: i for i, name in enumerate(_abi.CONVBF_INFO)}
    assert len(idx) <= _abi.CONVBF_INFO_LEN
    res, args = _abi.SIGNATURES["mde_convbf_instance"]
    assert res is ctypes.c_int and ctypes.c_void_p not in args       # a host query: no device pointer
    assert _lib().mde_convbf_instance(2, 64, 64, 60, 80, 3, 1, 0, None) == 11   # info is optional


@pytest.mark.parametrize("pass_,shape,row,props", _params())
def test_case_is_what_it_is_listed_for(pass_, shape, row, props):
    info = assert_listed(shape, pass_, row, props)
    n, cin, cout, h, w, ks, stride = shape
    lib = _lib()
    assert lib.mde_convbf_supported_n(n, cin, cout, h, w, ks, stride, pass_) == 1
    assert info["img_px"] <= info["cap"] and info["np"] == n * info["ppi"]
    assert info["ks"] == ks and info["blocks"] == -(-info["np"] // info["per"])
    # the bound's sum length, and a few patches an image wherever the kernel allows
    assert (cout if pass_ == 1 else cin) * ks * ks <= 5760


def test_cases_cover_every_instance_in_every_role():
    lib = _lib()
    count = lib.mde_convbf_instance_count(0)
    assert count == 46 and lib.mde_convbf_instance_count(1) == 4
    assert [lib.mde_convbf_instance_count(k) for k in (-1, 2)] == [0, 0]
    fwd = {row for _, row, _ in cc.FWD_CASES}
    dgrad = {row for _, row, _ in cc.DGRAD_CASES}
    assert not (fwd | dgrad) & set(cc.UNREACHED)
    assert fwd | dgrad | set(cc.UNREACHED) == set(range(count)), \
        sorted(set(range(count)) - fwd - dgrad - set(cc.UNREACHED))
    # an id's roles, from the record of a case listed for it: MODE S1 runs the
    # forward and the data gradient of stride-1 convs, S2 forwards, U2 data gradients
    mode = {}
    for p, cases in ALL[:2]:
        for shape, row, _ in cases:
            mode[row] = query(shape, p)[1]["mode"]
    for row, m in mode.items():
        if m in (0, 1):
            assert row in fwd, f"id {row} has no forward case"
        if m in (0, 2):
            assert row in dgrad, f"id {row} has no data-gradient case"
    wg = {row for _, row, _ in cc.WGRAD_CASES}
    assert wg | set(cc.UNREACHED_WGRAD) == set(range(lib.mde_convbf_instance_count(1)))
    # the switch-only ids have their cases in the list of their switch
    only = {row for row, why in cc.UNREACHED.items() if why.startswith("only under")}
    listed = {row for _, f, d in cc.SWITCH_CASES.values() for _, row, _ in f + d}
    assert listed == only, (sorted(listed), sorted(only))


def test_cases_cover_every_geometry_edge():
    have = {}     # family -> properties its cases are listed for
    for p, cases in ALL:
        for shape, _, props in cases:
            info = query(shape, p)[1]
            have.setdefault(family(info), set()).update(props)
            # "exact" is listed for a flat and for a tile geometry: tell them apart
            if "exact" in props:
                have[family(info)].add("exact-tile" if info["tile"] else "exact-flat")
    edges = {"flat", "tile", "pcol", "pband", "pboth", "clip"}
    for fam in ("res2", "res1", "chunk", "wgrad"):
        assert edges <= have[fam], f"{fam}: no case listed for {sorted(edges - have[fam])}"
    every = set().union(*have.values())
    assert {f"pc{v}" for v in (64, 40, 32, 20, 16, 8, 4)} <= every
    assert {"exact-flat", "exact-tile"} <= every
    # persistent blocks: a short last block and a block across two images, in the
    # resident kernel and in the weight gradient's splits; a half-empty M block on tiles
    assert {"per", "short", "span"} <= have["res1"] | have["res2"]
    assert {"per", "short", "span", "c32tile"} <= have["wgrad"]
    # every capacity constant reachable with the switches unset has its edge case
    caps = {query(shape, p)[1]["cap"] for p, cases in ALL for shape, _, props in cases if "cap" in props}
    assert caps == set(cc.CAP_EDGE), (caps, cc.CAP_EDGE)


# the sweep: channels, planes and batches around every selection threshold
SWEEP_CH = (32, 64, 96, 128, 160, 256, 288, 1184)
SWEEP_W = tuple(range(2, 81, 2)) + (98, 106, 136, 200, 212, 264)
SWEEP_N = (2, 5, 33)


def test_sweep_reaches_no_unlisted_instance_and_queries_agree():
    """Over a bounded grid: no id of UNREACHED comes back (one that becomes
    reachable needs a case), no staged image exceeds the largest the lists
    name for its capacity, and the sibling queries agree with the record."""
    lib = _lib()
    info = (ctypes.c_int32 * 24)()
    inst, sup = lib.mde_convbf_instance, lib.mde_convbf_supported_n
    I_KS, I_IMG, I_CAP, I_BLOCKS, I_RECORDS, I_GROUPS = 1, 13, 14, 17, 18, 21
    seen, capmax = ({}, {}, {}), {}
    for n in SWEEP_N:
        # the larger batches move `per` and the 2^22 limit, not the channel rules
        chans = SWEEP_CH if n == 2 else (32, 96, 1184)
        for cin in chans:
            for cout in chans:
                for ks in (1, 3):
                    for stride in (1, 2):
                        for h in range(1, 41):
                            for w in SWEEP_W:
                                for p in (0, 1, 2):
                                    row = inst(n, cin, cout, h, w, ks, stride, p, info)
                                    if row < 0:
                                        assert sup(n, cin, cout, h, w, ks, stride, p) == 0
                                        continue
                                    seen[p].setdefault(row, (n, cin, cout, h, w, ks, stride))
                                    if info[I_IMG] > capmax.get(info[I_CAP], 0):
                                        capmax[info[I_CAP]] = info[I_IMG]
                                    if h % 8 == 1:       # a sixth of the grid: three more calls each
                                        args = (n, cin, cout, h, w, ks, stride)
                                        assert sup(*args, p) == 1, (args, p)
                                        if p == 0:
                                            assert lib.mde_convbf_stats_blocks(*args) == info[I_RECORDS] \
                                                == info[I_BLOCKS], args
                                        if p == 2:
                                            want = 4 * info[I_GROUPS] * info[I_BLOCKS] * 64 * ks * ks * 32
                                            assert lib.mde_convbf_wgrad_workspace(*args) == want, args
    bad = {row: seen[p][row] for p in (0, 1) for row in seen[p] if row in cc.UNREACHED}
    assert not bad, f"ids listed as unreached came back: {bad}"
    assert not set(seen[2]) & set(cc.UNREACHED_WGRAD)
    assert capmax == cc.CAP_EDGE, (capmax, cc.CAP_EDGE)
    # the lists stay minimal against the sweep too: everything it reaches is listed
    assert set(seen[0]) <= {r for _, r, _ in cc.FWD_CASES} and set(seen[1]) <= {r for _, r, _ in cc.DGRAD_CASES}


def test_the_query_refuses_what_the_launch_refuses():
    lib = _lib()

    def q(*a):
        return lib.mde_convbf_instance(*a, None)

    ok = (2, 64, 64, 8, 12, 3, 1)
    for p in (0, 1, 2):
        assert q(*ok, p) >= 0 and lib.mde_convbf_supported_n(*ok, p) == 1
        for bad in ((2, 64, 64, 8, 13, 3, 1),       # odd width
                    (2, 48, 64, 8, 12, 3, 1), (2, 64, 80, 8, 12, 3, 1),   # channels off the 32 grid
                    (0, 64, 64, 8, 12, 3, 1),       # an empty batch
                    (2, 64, 64, 8, 12, 5, 1), (2, 64, 64, 8, 12, 2, 1),   # kernel sizes
                    (2, 64, 64, 8, 12, 3, 3)):      # stride
            assert q(*bad, p) == -1 and lib.mde_convbf_supported_n(*bad, p) == 0, (bad, p)
    for p in (-1, 3):
        assert q(*ok, p) == -1
    # an output plane whose pixels break the 4-pixel store groups: 11 x 18 (wo % 4 and ho * wo % 4)
    assert q(2, 96, 64, 22, 36, 3, 2, 0) == -1 and q(2, 96, 64, 22, 36, 3, 2, 2) == -1
    assert q(2, 96, 64, 22, 40, 3, 2, 0) >= 0       # 11 x 20
    assert q(2, 96, 64, 24, 36, 3, 2, 0) >= 0       # 12 x 18: ho * wo % 4 == 0, flat
    # np = n * ppi < 2^22 (the kernels' exact-division range), by the batch alone: one patch an image
    small = (32, 32, 2, 4, 1, 1)
    for p in (0, 1, 2):
        row, info = query(((1 << 22) - 1,) + small, p)
        assert row >= 0 and info["ppi"] == 1 and info["np"] == (1 << 22) - 1, (p, row, info)
        assert q(1 << 22, *small, p) == -1 and lib.mde_convbf_supported_n(1 << 22, *small, p) == 0
    # two patches an image: half the batch
    two = (32, 32, 5, 52, 1, 1)
    assert query((2,) + two, 0)[1]["ppi"] == 2
    assert q((1 << 21) - 1, *two, 0) >= 0 and q(1 << 21, *two, 0) == -1
