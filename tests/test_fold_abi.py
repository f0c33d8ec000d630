"""The full-resolution fold ABI (include/mde_fold_abi.h, _abi.FOLD_SIGNATURES) on the CPU.

No compute runs here: every call below returns from the argument checks, so the
non-null pointers (not device memory) are never dereferenced and nothing is
launched.
"""
import os
import re

from tests.conftest import REPO

HEADER = os.path.join(REPO, "include", "mde_fold_abi.h")
ENTRIES = {"mde_skip_reduce_bn_bwd_nogs", "mde_pointwise_bwd_bn_rank1", "mde_bilinear_bwd2_rank1"}
P = 0x1000  # non-null


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int64_t|int|size_t|double|const char\*)\s+(mde_\w+)\s*\(([^)]*)\)\s*;",
                         text):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return decls


def test_header_and_table_agree_and_are_exported():
    from monocular_depth_estimation_amd import _abi
    lib = _abi.load()
    d = declared_functions()
    assert set(d) == ENTRIES
    assert set(_abi.FOLD_SIGNATURES) == set(d)
    for name, nargs in d.items():
        assert hasattr(lib, name), f"{name} not exported by {_abi.LIB_PATH}"
        res, args = _abi.FOLD_SIGNATURES[name]
        assert len(args) == nargs, f"{name}: ctypes arity != header arity"
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)  # load() applied the table


def test_tables_are_disjoint():
    from monocular_depth_estimation_amd import _abi
    tables = [set(_abi.SIGNATURES), set(_abi.EVAL_SIGNATURES), set(_abi.INFER_SIGNATURES),
              set(_abi.AA_SIGNATURES), set(_abi.FOLD_SIGNATURES)]
    assert len(set().union(*tables)) == sum(len(t) for t in tables)


def _null_each(f, ptr_idx, args, optional=()):
    """Every pointer argument NULL in turn -> MDE_ERR_INVALID_ARG (-1)."""
    for k in ptr_idx:
        if k in optional:
            continue
        a = list(args)
        a[k] = None
        assert f(*a) == -1, k


def test_skip_bwd_nogs_refuses_before_launch():
    from monocular_depth_estimation_amd import _abi
    f = _abi.load().mde_skip_reduce_bn_bwd_nogs
    ok = [P] * 10 + [2, 16, 1, 8, 16, P, 0, None]
    _null_each(f, list(range(10)) + [15], ok)
    for k in (10, 13):  # n, h
        for bad in (0, -2):
            a = list(ok)
            a[k] = bad
            assert f(*a) == -1, (k, bad)
    # only 16 -> 1 with h w % 4 == 0, fp32
    for cin, cout, h, w in ((4, 1, 8, 16), (32, 16, 8, 16), (16, 2, 8, 16), (16, 1, 3, 5)):
        a = list(ok)
        a[11:15] = [cin, cout, h, w]
        assert f(*a) == -2, (cin, cout, h, w)
    for dtype in (1, 7):
        a = list(ok)
        a[16] = dtype
        assert f(*a) == -2


def test_pointwise_rank1_refuses_before_launch():
    from monocular_depth_estimation_amd import _abi
    f = _abi.load().mde_pointwise_bwd_bn_rank1
    ok = [P] * 12 + [2, 16, 16, 8, 16, P, 0, None]
    _null_each(f, list(range(12)) + [17], ok)
    # only 16 -> 16 with h w % 64 == 0, n > 0, fp32
    for n, cin, cout, h, w in ((2, 16, 8, 8, 16), (2, 32, 32, 8, 16), (2, 32, 16, 8, 16),
                               (2, 16, 16, 8, 12), (0, 16, 16, 8, 16), (-1, 16, 16, 8, 16),
                               (2, 16, 16, 0, 16)):
        a = list(ok)
        a[12:17] = [n, cin, cout, h, w]
        assert f(*a) == -2, (n, cin, cout, h, w)
    for dtype in (1, 7):
        a = list(ok)
        a[18] = dtype
        assert f(*a) == -2


def test_bilinear_rank1_refuses_before_launch():
    from monocular_depth_estimation_amd import _abi
    lib = _abi.load()
    f = lib.mde_bilinear_bwd2_rank1
    ok = [P, P, P, P, 2, 16, 5, 8, 10, 16, 0.5, 0.5, 0, 0, None]
    _null_each(f, range(4), ok)
    for k in range(4, 10):
        a = list(ok)
        a[k] = 0
        assert f(*a) == -1, k
    # the shapes mde_bilinear_bwd2 takes, and no others: not x2, odd width, align_corners
    for hi, wi, ho, wo, sh, sw, al in ((5, 8, 15, 24, 1 / 3, 1 / 3, 0), (5, 7, 10, 14, 0.5, 0.5, 0),
                                       (5, 8, 10, 16, 4 / 9, 7 / 15, 1)):
        assert lib.mde_bilinear_bwd2_supported(2, 16, hi, wi, ho, wo, sh, sw, al) == 0
        a = list(ok)
        a[6:13] = [hi, wi, ho, wo, sh, sw, al]
        assert f(*a) == -2, (hi, wi, ho, wo)
    for dtype in (1, 7):  # fp32 only (mde_bilinear_bwd2 also takes bf16)
        a = list(ok)
        a[13] = dtype
        assert f(*a) == -2
