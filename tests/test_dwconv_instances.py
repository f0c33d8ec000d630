"""The case lists of tests/_dwconv_instance_cases.py reach every compiled
instance of csrc/dwconv.hip and every layout edge they are listed for (no GPU:
mde_dwconv_instance is host arithmetic, the record mde_dwconv_fwd,
mde_dwconv_bwd and mde_dwconv_workspace themselves switch on).

A case removed, or a selection constant changed (the lane utilisation bound,
the segment width, the block targets) so that a listed case moves, fails here
until the lists are right again; tests/test_gpu_dwconv.py runs exactly these
cases against float64.
"""
import ctypes
import os
import re

import pytest

from tests import _dwconv_instance_cases as dc
from tests.conftest import REPO

INVALID = -1      # MDE_ERR_INVALID_ARG


def _abi():
    from monocular_depth_estimation_amd import _abi
    return _abi


def _lib():
    return _abi().load()


def named(info):
    """The record with path and reducer by name."""
    a = _abi()
    return dict(info, path=a.DW_PATHS[info["path"]], reducer=a.DW_REDUCERS[info["reducer"]])


def assert_listed(shape, row_f, row_b, fwd, bwd):
    """The queried records of a case equal what it is listed for; returns them."""
    a = _abi()
    got_f, info_f = a.dwconv_instance(*shape, 0)
    got_b, info_b = a.dwconv_instance(*shape, 1, True, True)
    assert (got_f, got_b) == (row_f, row_b), (shape, got_f, got_b)
    info_f, info_b = named(info_f), named(info_b)
    for want, info in ((fwd, info_f), (bwd, info_b)):
        have = {k: info[k] for k in want}
        assert have == want, (shape, have, want)
    return info_f, info_b


def test_info_fields_match_the_header():
    a = _abi()
    text = open(os.path.join(REPO, "include", "mde_abi.h")).read()
    assert int(re.search(r"#define MDE_DWCONV_INFO_LEN (\d+)", text).group(1)) == a.DWCONV_INFO_LEN
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define MDE_DW_I_(\w+) (\d+)", text)}
    assert idx == {name: i for i, name in enumerate(a.DWCONV_INFO)}
    assert len(idx) <= a.DWCONV_INFO_LEN
    for prefix, names in (("PATH", a.DW_PATHS), ("RED", a.DW_REDUCERS)):
        got = {m.group(1).lower(): int(m.group(2))
               for m in re.finditer(rf"#define MDE_DW_{prefix}_(\w+) (\d+)", text)}
        assert got == {name: i for i, name in enumerate(names)}
    res, args = a.SIGNATURES["mde_dwconv_instance"]
    assert res is ctypes.c_int and ctypes.c_void_p not in args       # a host query: no device pointer
    assert _lib().mde_dwconv_instance(2, 3, 9, 160, 3, 1, 1, 0, 0, 0, None) == 2   # info is optional


@pytest.mark.parametrize("shape,row_f,row_b,fwd,bwd",
                         [pytest.param(*c, id=dc.case_id(c[0])) for c in dc.ALL_CASES])
def test_case_is_what_it_is_listed_for(shape, row_f, row_b, fwd, bwd):
    a, lib = _abi(), _lib()
    info_f, info_b = assert_listed(shape, row_f, row_b, fwd, bwd)
    n, c, h, w, k, s, p = shape
    for info in (info_f, info_b):
        assert (info["k"], info["s"], info["pad"]) == (k, s, p)
        assert (info["ho"], info["wo"]) == ((h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1)
    assert info_f["ws"] == 0 and info_f["reducer"] == "none"
    assert info_b["ws"] == lib.mde_dwconv_workspace(*shape)
    # the gradients requested decide the reducer and the workspace, never the instance
    g = info_b["g"]
    for gx, gw in ((True, False), (False, True), (False, False)):
        row, one = a.dwconv_instance(*shape, 1, gx, gw)
        one = named(one)
        assert row == row_b
        skip = {"ws", "reducer", "blocks"}
        assert {k_: v for k_, v in one.items() if k_ not in skip} == \
            {k_: v for k_, v in info_b.items() if k_ not in skip}
        if not gw:
            assert (one["ws"], one["reducer"]) == (0, "none")
        else:
            assert one["ws"] == info_b["ws"]
            want = {"stream": "wsum" if g > 1 else "none", "strip": "wreduce" if g > 1 else "none",
                    "split": "wreduce"}[info_b["path"]]
            assert one["reducer"] == want
    # at most the suite's size limit for a quick case
    assert n * c * h * w <= 16 << 20


def test_cases_cover_every_instance_and_layout():
    lib = _lib()
    counts = [lib.mde_dwconv_instance_count(p) for p in (0, 1)]
    assert counts == [16, 20]
    assert [lib.mde_dwconv_instance_count(p) for p in (-1, 2)] == [0, 0]
    for p, col in ((0, 1), (1, 2)):
        ids = {c[col] for c in dc.ALL_CASES}
        unreached = {row for (pp, row), why in dc.UNREACHED.items() if pp == p and why}
        assert not ids & unreached
        assert ids | unreached == set(range(counts[p])), sorted(set(range(counts[p])) - ids - unreached)
    recs = [assert_listed(*c)[1] for c in dc.ALL_CASES]
    stream = [r for r in recs if r["path"] == "stream"]
    strip = [(c[0], assert_listed(*c)) for c in dc.STRIP_CASES]
    assert {r["wpb"] for r in stream} == dc.WPB_VALUES
    # one lane a segment with and without edge loads; prime column-group counts
    assert {(r["edge"], r["l"]) for r in stream} >= {(0, 1), (1, 1), (1, 2), (1, 20)}
    # stride 2 with an odd height, at every stride-2 instance
    odd = {c[1] for c in dc.ALL_CASES if c[3]["path"] == "stream" and c[0][5] == 2 and c[0][2] % 2}
    assert odd == {3, 4, 5, 9, 10, 11}
    assert any(c[0][2] < c[0][4] for c in dc.STREAM_CASES)               # h < k
    assert any(r["g"] > 64 for r in stream)
    # a channel split over blocks: with and without edge loads, at both strides
    assert {(r["s"], r["edge"]) for r in stream if r["g"] > 1} == {(1, 0), (1, 1), (2, 0), (2, 1)}
    tail = [r for r in stream if r["it"] > 1]
    assert tail and all(((r["g"] * r["it"] - 1) * r["wpb"]) * r["spw"] >= r["upc"] for r in tail)
    # strip: several tiles both ways at stride 2, short last stacks, split channels
    assert any(f["s"] == 2 and f["tx"] > 1 and f["ty"] > 1 for _, (f, b) in strip)
    assert any(f["pb"] > 1 and (sh[0] * sh[1]) % f["pb"] for sh, (f, b) in strip)
    assert any(b["pb"] > 1 and sh[0] % b["pb"] for sh, (f, b) in strip)
    assert {(b["k"], b["s"]) for _, (f, b) in strip if b["g"] > 1} == {(3, 1), (3, 2), (5, 1), (5, 2)}
    split = [r for r in recs if r["path"] == "split"]
    assert any(r["s"] == 2 and r["tx"] * r["ty"] > 1 and r["tx2"] * r["ty2"] > 1 for r in split)
    assert any(r["pad"] == 0 and r["ho"] == 1 and r["wo"] == 1 for r in split)


def dw_ok(n, c, h, w, k, s, p):
    """The shape contract of the depthwise entries (include/mde_abi.h, csrc/dwconv.hip: dw_ok)."""
    return (n > 0 and c > 0 and h > 0 and w > 0 and k in (3, 5) and s in (1, 2) and 0 <= p < k
            and n * c <= 65535 and n * c * h * w < 1 << 31 and h * w < 1 << 24
            and h + 2 * p - k >= 0 and w + 2 * p - k >= 0)


def test_the_query_refuses_what_the_launch_refuses():
    lib = _lib()
    ok = (2, 3, 9, 16, 3, 1, 1)
    edges = [ok, (0,) + ok[1:], (2, 0) + ok[2:], (2, 3, 0, 16, 3, 1, 1), (2, 3, 9, 0, 3, 1, 1),
             (2, 3, 9, 16, 4, 1, 1), (2, 3, 9, 16, 7, 1, 3), (2, 3, 9, 16, 3, 3, 1), (2, 3, 9, 16, 3, 0, 1),
             (2, 3, 9, 16, 3, 1, -1), (2, 3, 9, 16, 3, 1, 3), (2, 3, 9, 16, 3, 1, 2), (2, 3, 9, 16, 5, 2, 4),
             (65535, 1, 1, 4, 3, 1, 1), (65536, 1, 1, 4, 3, 1, 1), (255, 257, 1, 4, 3, 1, 1),
             (256, 256, 1, 4, 3, 1, 1), (2, 1, 1 << 15, (1 << 15) - 1, 3, 1, 1),
             (1, 127, 4096, 4095, 5, 2, 2), (1, 128, 4096, 4095, 5, 2, 2), (1, 128, 4096, 4096, 5, 2, 2),
             (1, 1, 4096, 4096, 3, 1, 1), (1, 1, 2, 2, 3, 1, 0), (1, 1, 2, 3, 3, 1, 1), (1, 1, 1, 1, 5, 1, 2),
             (1, 1, 1, 1, 5, 1, 1), (1, 1, 3, 2, 3, 2, 0)]
    for shape in edges:
        for p in (0, 1):
            row = lib.mde_dwconv_instance(*shape, p, 1, 1, None)
            assert (row >= 0) == dw_ok(*shape), (shape, p, row)
            if row < 0:
                assert row == INVALID and lib.mde_dwconv_workspace(*shape) == 0
        for p in (-1, 2):
            assert lib.mde_dwconv_instance(*shape, p, 1, 1, None) == INVALID
    # a refused query leaves info alone
    info = (ctypes.c_int32 * 32)(*([7] * 32))
    assert lib.mde_dwconv_instance(2, 3, 9, 16, 4, 1, 1, 0, 1, 1, info) == INVALID
    assert list(info) == [7] * 32


# the sweep: every plane up to 70 x 70 and the widths of the encoder's stages,
# every (k, stride, pad), a few (n, c) on both sides of the block-count targets
SWEEP_W = tuple(range(1, 71)) + (80, 92, 160, 184, 320)
SWEEP_NC = ((1, 1), (2, 3), (5, 700), (33, 40))


def test_sweep_layouts_cover_their_planes():
    """Over a bounded grid: the query refuses exactly what dw_ok refuses, the id
    is the table row of the record's own (path, K, S, V, EDGE), every layout
    covers its plane and its units, and mde_dwconv_workspace agrees."""
    a, lib = _abi(), _lib()
    inst, wsq = lib.mde_dwconv_instance, lib.mde_dwconv_workspace
    info = (ctypes.c_int32 * a.DWCONV_INFO_LEN)()
    I = {name: i for i, name in enumerate(a.DWCONV_INFO)}
    seen = ({}, {})
    for n, c in SWEEP_NC:
        for k in (3, 5):
            for s in (1, 2):
                for pad in range(k + 1):
                    for h in range(1, 71):
                        for w in SWEEP_W:
                            shape = (n, c, h, w, k, s, pad)
                            ok = dw_ok(*shape)
                            for p in (0, 1):
                                row = inst(*shape, p, 1, 1, info)
                                assert (row >= 0) == ok, (shape, p, row)
                                if not ok:
                                    continue
                                seen[p].setdefault(row, shape)
                                r = {name: info[i] for name, i in I.items()}
                                ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
                                assert (r["ho"], r["wo"], r["pass"]) == (ho, wo, p), shape
                                ks = 2 * (k == 5) + s - 1
                                if r["path"] == 0:
                                    v0 = 4 if s == 1 else 2
                                    assert pad == k // 2 and w == s * wo
                                    assert r["v"] in (v0, 2 * v0) and not (r["edge"] and r["v"] != v0)
                                    assert r["rb"] * r["v"] == (8 if s == 1 else 4) * v0, shape
                                    assert row == 3 * ks + (2 if r["v"] != v0 else 1 - r["edge"])
                                    assert r["l"] * r["nseg"] * r["v"] == wo, shape
                                    assert r["spw"] == 64 // r["l"] >= 1
                                    assert r["edge"] or r["nseg"] == 1
                                    assert (r["nb"] - 1) * r["rb"] < ho <= r["nb"] * r["rb"], shape
                                    if p:
                                        assert r["upc"] == n * r["nb"] * r["nseg"]
                                        assert r["g"] * r["it"] * r["wpb"] * r["spw"] >= r["upc"], shape
                                        # no block of a channel without a unit, at most 8 waves a block
                                        assert (r["g"] - 1) * r["it"] * r["wpb"] * r["spw"] < r["upc"], shape
                                        assert 1 <= r["wpb"] <= 8 and r["blocks"] == c * r["g"]
                                        want = 4 * c * r["g"] * k * k if r["g"] > 1 else 0
                                        assert r["ws"] == want == wsq(*shape), shape
                                        assert r["reducer"] == (1 if r["g"] > 1 else 0)
                                    else:
                                        units = n * c * r["nb"] * r["nseg"]
                                        assert r["blocks"] == -(-(-(-units // r["spw"])) // 4)
                                elif r["path"] == 1:
                                    assert row == 12 + ks and (p == 0 or pad == k // 2)
                                    assert r["tx"] * r["tw"] >= wo > (r["tx"] - 1) * r["tw"], shape
                                    assert r["ty"] * r["th"] >= ho > (r["ty"] - 1) * r["th"], shape
                                    assert r["th"] == 4 * r["rg"] and r["tw"] <= 64
                                    assert 1 <= r["pb"] and r["pb"] * r["tw"] * r["rg"] <= 256, shape
                                    if p:
                                        assert r["pb"] <= n
                                        items = -(-n // r["pb"]) * r["tx"] * r["ty"]
                                        assert 1 <= r["g"] <= items and r["blocks"] == c * r["g"]
                                        want = 4 * c * r["g"] * k * k if r["g"] > 1 else 0
                                        assert r["ws"] == want == wsq(*shape), shape
                                        assert r["reducer"] == (3 if r["g"] > 1 else 0)
                                    else:
                                        assert r["pb"] <= n * c and r["pb"] * k * k <= 256
                                        assert r["blocks"] == r["tx"] * r["ty"] * -(-n * c // r["pb"])
                                else:
                                    assert p == 1 and row == 16 + ks and pad != k // 2
                                    assert r["tx"] * r["tw"] >= w > (r["tx"] - 1) * r["tw"], shape
                                    assert r["ty"] * r["th"] >= h > (r["ty"] - 1) * r["th"], shape
                                    assert r["tx2"] * r["tw2"] >= wo > (r["tx2"] - 1) * r["tw2"], shape
                                    assert r["ty2"] * r["th2"] >= ho > (r["ty2"] - 1) * r["th2"], shape
                                    assert r["p"] == n * r["tx2"] * r["ty2"]
                                    assert r["ws"] == 4 * c * r["p"] * k * k == wsq(*shape), shape
                                    assert r["reducer"] == 3
                                    assert r["blocks"] == n * c * r["tx"] * r["ty"]
    counts = [lib.mde_dwconv_instance_count(p) for p in (0, 1)]
    for p in (0, 1):
        assert set(seen[p]) <= set(range(counts[p]))
        bad = {row: seen[p][row] for row in seen[p] if (p, row) in dc.UNREACHED}
        assert not bad, f"ids listed as unreached came back: {bad}"
        # the lists stay complete against the sweep: everything it reaches is listed
        assert set(seen[p]) <= {c[1 + p] for c in dc.ALL_CASES}
