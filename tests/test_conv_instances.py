"""The case lists of tests/_conv_instance_cases.py reach every row of the three
first-match instance tables of csrc/conv3x3s2.hip (no GPU: the queries are host
arithmetic, the launchers' own selection functions).

A row added to a table, or an R / NJ changed so that a listed shape moves to
another row, fails here until the lists name a case for every row again; the
GPU tests then run exactly those cases against float64.
"""
import pytest

from tests._conv_instance_cases import S1_WIDE_CASES, S2_DGRAD_CASES, S2_FWD_CASES


def _lib():
    from monocular_depth_estimation_amd import _abi
    return _abi.load()


def wide_rows(lib, case):
    """Rows of the two wide passes of a case: the forward of cin -> cout and the
    data gradient of the mirrored conv cout -> cin (both produce cout channels)."""
    n, cin, cout, h, w = case
    return (lib.mde_conv3x3_wide_instance(n, cin, cout, h, w, 0),
            lib.mde_conv3x3_wide_instance(n, cout, cin, h, w, 1))


@pytest.mark.parametrize("which,entry,cases", [
    (0, "mde_conv3x3s2_fwd_instance", S2_FWD_CASES),
    (1, "mde_conv3x3s2_dgrad_instance", S2_DGRAD_CASES)])
def test_stride2_cases_cover_every_table_row(which, entry, cases):
    lib = _lib()
    count = lib.mde_conv3x3s2_instance_count(which)
    assert count > 0
    rows = [getattr(lib, entry)(*c) for c in cases]
    assert set(rows) == set(range(count)), \
        f"{entry}: rows without a case {sorted(set(range(count)) - set(rows))}, rows of the cases {rows}"
    assert rows == list(range(count)), rows   # case i is listed for row i


def test_wide_cases_cover_every_table_row_in_both_passes():
    lib = _lib()
    count = lib.mde_conv3x3s2_instance_count(2)
    assert count > 0
    rows = [wide_rows(lib, c) for c in S1_WIDE_CASES]
    for p in (0, 1):
        got = [r[p] for r in rows]
        assert set(got) == set(range(count)), \
            f"pass {p}: rows without a case {sorted(set(range(count)) - set(got))}, rows of the cases {got}"
        assert got == list(range(count)), (p, got)


def test_instance_queries_follow_the_launch_rules():
    lib = _lib()
    assert [lib.mde_conv3x3s2_instance_count(k) for k in (-1, 3)] == [0, 0]
    # no dispatch threshold: planes the *_supported queries leave to MIOpen have a row
    assert lib.mde_conv3x3s2_fwd_supported(64, 64, 7, 10, 0) == 0
    assert lib.mde_conv3x3s2_fwd_instance(2, 64, 64, 7, 10) >= 0
    assert lib.mde_conv3x3s2_dgrad_supported(128, 256, 30, 40, 0) == 0
    assert lib.mde_conv3x3s2_dgrad_instance(2, 128, 256, 30, 40) >= 0
    # what the launchers refuse has none: odd width, channels off the 32 grid,
    # an empty batch, a band deeper than any instance, an unknown pass
    for bad in ((2, 32, 32, 8, 31), (2, 48, 32, 8, 32), (2, 32, 40, 8, 32), (0, 32, 32, 8, 32)):
        assert lib.mde_conv3x3s2_fwd_instance(*bad) == -1, bad
        assert lib.mde_conv3x3s2_dgrad_instance(*bad) == -1, bad
    assert lib.mde_conv3x3s2_fwd_instance(2, 32, 64, 40, 10) == -1      # 13 output rows under a tile
    assert lib.mde_conv3x3s2_dgrad_instance(2, 32, 32, 30, 40) == -1    # 32 channels: wide planes only
    assert lib.mde_conv3x3s2_dgrad_instance(2, 3, 32, 66, 256) == -1    # the image needs no gradient
    assert lib.mde_conv3x3_wide_instance(2, 32, 64, 9, 21, 2) == -1
    assert lib.mde_conv3x3_wide_instance(0, 32, 64, 9, 21, 0) == -1
    assert lib.mde_conv3x3_wide_instance(2, 16, 64, 9, 21, 0) == -1
    # the wide row depends on the batch: the 2 x 2 wave tiles from 512 blocks on
    n, cin, cout, h, w = S1_WIDE_CASES[9]
    assert n * -(-h * w // 128) >= 512 > (n - 1) * -(-h * w // 128)
    assert lib.mde_conv3x3_wide_instance(n, cin, cout, h, w, 0) == 9
    assert lib.mde_conv3x3_wide_instance(n - 1, cin, cout, h, w, 0) in range(6)
    # every query agrees with the batch-free *_supported one on whether a kernel exists
    for c in S1_WIDE_CASES:
        assert lib.mde_conv3x3_wide_supported(c[1], c[2], c[3], c[4], 0, 0) == 1, c
        assert lib.mde_conv3x3_wide_supported(c[2], c[1], c[3], c[4], 1, 0) == 1, c
