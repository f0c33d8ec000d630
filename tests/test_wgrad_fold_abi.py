"""The guide weight-gradient fold ABI (include/mde_wgrad_fold_abi.h,
_abi.WGRAD_FOLD_SIGNATURES) on the CPU.

No compute runs here: every call below returns from the argument checks, so the
non-null pointers (not device memory) are never dereferenced and nothing is
launched.
"""
import ctypes
import os
import re

from tests.conftest import REPO

HEADER = os.path.join(REPO, "include", "mde_wgrad_fold_abi.h")
ENTRIES = {"mde_conv3x3_wgrad_bn_deferred_supported", "mde_conv3x3_wgrad_bn_deferred",
           "mde_batchnorm_bwd_reduce_coef"}
P = 0x1000  # non-null
_CTYPE = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64}


def declared_functions():
    """name -> (result type, arity) of every declaration in the header."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(int64_t|int|size_t)\s+(mde_\w+)\s*\(([^)]*)\)\s*;", text):
        args = m.group(3).strip()
        decls[m.group(2)] = (m.group(1), 0 if args in ("", "void") else args.count(",") + 1)
    return decls


def test_header_and_table_agree_and_are_exported():
    from monocular_depth_estimation_amd import _abi
    lib = _abi.load()
    d = declared_functions()
    assert set(d) == ENTRIES
    assert set(_abi.WGRAD_FOLD_SIGNATURES) == set(d)
    for name, (rtype, nargs) in d.items():
        assert hasattr(lib, name), f"{name} not exported by {_abi.LIB_PATH}"
        res, args = _abi.WGRAD_FOLD_SIGNATURES[name]
        assert res is _CTYPE[rtype], f"{name}: ctypes result type != header's {rtype}"
        assert len(args) == nargs, f"{name}: ctypes arity != header arity"
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)  # load() applied the table


def test_table_is_disjoint_from_the_other_five():
    from monocular_depth_estimation_amd import _abi
    others = [_abi.SIGNATURES, _abi.EVAL_SIGNATURES, _abi.INFER_SIGNATURES, _abi.AA_SIGNATURES,
              _abi.FOLD_SIGNATURES]
    for t in others:
        assert not set(t) & set(_abi.WGRAD_FOLD_SIGNATURES)
    tables = [set(t) for t in others] + [set(_abi.WGRAD_FOLD_SIGNATURES)]
    assert len(set().union(*tables)) == sum(len(t) for t in tables)


def test_supported_query():
    from monocular_depth_estimation_amd import _abi
    q = _abi.load().mde_conv3x3_wgrad_bn_deferred_supported
    for cout in (16, 32, 64):
        for n, h, w in ((2, 16, 64), (2, 17, 72), (1, 18, 58), (32, 480, 640), (1, 32, 32)):
            assert q(n, 3, cout, h, w) == 1, (cout, n, h, w)
    # h w < 1024, h w % 4 != 0: the apply pass is not on its plane kernel there
    for n, h, w in ((2, 8, 16), (2, 31, 33), (1, 33, 33), (2, 16, 63)):
        assert q(n, 3, 16, h, w) == 0, (n, h, w)
    # only the guide convs; sizes; the kernel's 32-bit offsets (64 h w < 2^31)
    for n, cin, cout, h, w in ((2, 16, 16, 16, 64), (2, 32, 32, 16, 64), (2, 3, 8, 16, 64),
                               (2, 3, 48, 16, 64), (0, 3, 16, 16, 64), (-1, 3, 16, 16, 64),
                               (2, 3, 16, 0, 64), (1, 3, 16, 4096, 8192)):
        assert q(n, cin, cout, h, w) == 0, (n, cin, cout, h, w)


def _null_each(f, ptr_idx, args, optional=()):
    """Every pointer argument NULL in turn -> MDE_ERR_INVALID_ARG (-1)."""
    for k in ptr_idx:
        if k in optional:
            continue
        a = list(args)
        a[k] = None
        assert f(*a) == -1, k


def test_wgrad_deferred_refuses_before_launch():
    from monocular_depth_estimation_amd import _abi
    f = _abi.load().mde_conv3x3_wgrad_bn_deferred
    ok = [P] * 5 + [2, 3, 16, 16, 64, P, 0, None]
    _null_each(f, list(range(5)) + [10], ok)
    for k in (5, 8, 9):  # n, h, w
        for bad in (0, -2):
            a = list(ok)
            a[k] = bad
            assert f(*a) == -1, (k, bad)
    for cin, cout, h, w in ((16, 16, 16, 64), (3, 8, 16, 64), (3, 16, 8, 16), (3, 16, 31, 33)):
        a = list(ok)
        a[6:10] = [cin, cout, h, w]
        assert f(*a) == -2, (cin, cout, h, w)
    for dtype in (1, 7):
        a = list(ok)
        a[11] = dtype
        assert f(*a) == -2


def test_reduce_coef_refuses_before_launch():
    from monocular_depth_estimation_amd import _abi
    f = _abi.load().mde_batchnorm_bwd_reduce_coef
    ok = [P] * 6 + [1] + [P] * 4 + [2, 64, 16, 64, 1, P, 0, None]
    _null_each(f, list(range(6)) + [7, 8, 9, 10, 16], ok, optional=(8, 9, 10))
    for k in (11, 12, 13, 14):  # n, c, h, w
        for bad in (0, -2):
            a = list(ok)
            a[k] = bad
            assert f(*a) == -1, (k, bad)
    for act in (-1, 3):
        a = list(ok)
        a[15] = act
        assert f(*a) == -1
    for h, w in ((8, 16), (31, 33)):  # the apply pass is not on its plane kernel
        a = list(ok)
        a[13:15] = [h, w]
        assert f(*a) == -2, (h, w)
    for dtype in (1, 7):
        a = list(ok)
        a[17] = dtype
        assert f(*a) == -2
