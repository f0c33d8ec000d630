"""The guard harness (tests/_abi_guard.py) must be able to fail: fake "entries"
that misbehave on HOST memory, inside the harness's own relocated allocation,
are each reported with entry, argument and byte offset.  No GPU is needed and no
kernel runs; the package import still loads the built library for `_abi`."""
import ctypes

import pytest
import torch

from monocular_depth_estimation_amd import _abi
from tests._abi_guard import (CARRIED, EXCLUDED, INDIRECT, RMW, TAIL, GuardViolation,
                              UnguardedPointer, guarded_abi, launching_entries)

_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int

# fake entries: (x, y, n, workspace, stream) unless noted
SIG = {
    "fake_double": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_past_end": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_before_start": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_skip": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_stale_scratch": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_acc": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_shift": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_scratch_overrun": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_keep": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_use_kept": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_short": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "fake_two": (_int, [_vp, _vp, _vp, _i64, _vp]),   # (x, y1, y2, n, stream)
}
N = 10
SKIPPED = 7


def _f32(p, n, first=0):
    """n floats at address p + 4 * first (first may be negative)."""
    return (ctypes.c_float * n).from_address(p + 4 * first)


def fake(name, x, y, n, ws, stream):
    if name == "fake_two":      # two outputs; the second skips one element
        x, y, y2, n = x, y, n, ws
        seen.append((name, y, y2, None))
        for i in range(n):
            _f32(y, n)[i] = _f32(x, n)[i]
            if i != SKIPPED:
                _f32(y2, n)[i] = _f32(x, n)[i]
        return
    seen.append((name, x, y, ws))
    xs, ys = _f32(x, n), _f32(y, n)
    tmp = _f32(ws, n) if ws else None
    if name == "fake_double":       # scratch written, then read: well behaved
        for i in range(n):
            tmp[i] = xs[i]
        for i in range(n):
            ys[i] = 2.0 * tmp[i]
    elif name == "fake_past_end":
        for i in range(n + 1):
            _f32(y, 1, i)[0] = 1.0
    elif name == "fake_before_start":
        for i in range(-1, n):
            _f32(y, 1, i)[0] = 1.0
    elif name == "fake_skip":
        for i in range(n):
            if i != SKIPPED:
                ys[i] = xs[i] + 1.0
    elif name == "fake_stale_scratch":  # assumes scratch starts at zero
        for i in range(n):
            ys[i] = xs[i] + tmp[i]
    elif name == "fake_acc":
        for i in range(n):
            ys[i] = ys[i] + xs[i]
    elif name == "fake_shift":      # reads all of x, then writes y (they may overlap)
        vals = [xs[i] + 1.0 for i in range(n)]
        for i in range(n):
            ys[i] = vals[i]
    elif name == "fake_short":      # stops one element early
        for i in range(n - 1):
            ys[i] = xs[i] + 1.0
    elif name == "fake_keep":        # leaves 3 x in the workspace for fake_use_kept
        for i in range(n):
            tmp[i] = 3.0 * xs[i]
            ys[i] = xs[i]
    elif name == "fake_use_kept":
        for i in range(n):
            ys[i] = tmp[i] + xs[i]
    elif name == "fake_scratch_overrun":
        for i in range(n):
            ys[i] = xs[i]
        ctypes.c_uint8.from_address(ws + 4 * n).value = 0
    else:
        raise AssertionError(name)


seen = []


def launch(g, name, x, y, ws=None, n=N):
    _abi.call(name, _abi.ptr(x), _abi.ptr(y), n, _abi.ptr(ws), None)


def _ws(n=N):
    ws = torch.empty(4 * n, dtype=torch.uint8)
    ws._mde_workspace = True   # as functional._ws tags what it returns
    return ws


def ctx(**kw):
    return guarded_abi(invoke=fake, signatures=SIG, **kw)


def test_patches_are_undone_and_calls_counted():
    real = (_abi.ptr, _abi.call)
    x, y = torch.arange(N, dtype=torch.float32), torch.zeros(N)
    with ctx() as g:
        assert (_abi.ptr, _abi.call) != real
        launch(g, "fake_double", x, y, _ws())
        launch(g, "fake_double", x, y, _ws())
    assert (_abi.ptr, _abi.call) == real
    assert g.calls == {"fake_double": 2}


def test_well_behaved_entry_passes_and_results_come_back():
    x, y = torch.arange(N, dtype=torch.float32), torch.full((N,), -3.0)
    x0 = x.clone()
    seen.clear()
    with ctx() as g:
        launch(g, "fake_double", x, y, _ws())
    assert torch.equal(y, 2 * x0) and torch.equal(x, x0)
    assert len(seen) == 2                      # ran twice ...
    for _, px, py, pw in seen:                 # ... and never on the caller's memory
        assert px != x.data_ptr() and py != y.data_ptr() and pw


def test_store_past_the_end_is_reported():
    x, y = torch.ones(N), torch.zeros(N)
    with ctx(), pytest.raises(GuardViolation) as e:
        launch(None, "fake_past_end", x, y)
    v = e.value
    assert (v.entry, v.arg, v.offset, v.shape, v.dtype) == ("fake_past_end", 1, 4 * N, (N,), torch.float32)
    assert "back guard" in str(v) and "fake_past_end" in str(v) and "argument 1" in str(v)


def test_store_before_the_start_is_reported():
    x, y = torch.ones(N), torch.zeros(N)
    with ctx(), pytest.raises(GuardViolation) as e:
        launch(None, "fake_before_start", x, y)
    v = e.value
    assert (v.entry, v.arg, v.offset) == ("fake_before_start", 1, -4)
    assert "front guard" in str(v)


def test_scratch_overrun_is_reported():
    x, y = torch.ones(N), torch.zeros(N)
    with ctx(), pytest.raises(GuardViolation) as e:
        launch(None, "fake_scratch_overrun", x, y, _ws())
    assert (e.value.entry, e.value.arg, e.value.offset) == ("fake_scratch_overrun", 3, 4 * N)


def test_skipped_output_element_is_reported():
    x, y = torch.ones(N), torch.zeros(N)
    with ctx(), pytest.raises(GuardViolation) as e:
        launch(None, "fake_skip", x, y)
    v = e.value
    assert (v.entry, v.arg, v.offset) == ("fake_skip", 1, 4 * SKIPPED)
    assert "disagree" in str(v)


def test_reading_scratch_before_writing_it_is_reported():
    x, y = torch.ones(N), torch.zeros(N)
    with ctx(), pytest.raises(GuardViolation) as e:
        launch(None, "fake_stale_scratch", x, y, _ws().zero_())
    assert (e.value.entry, e.value.arg) == ("fake_stale_scratch", 1)
    assert 0 <= e.value.offset < 4


def test_reading_its_own_output_is_reported_unless_rmw():
    x, y = torch.ones(N), torch.full((N,), 5.0)
    with ctx(rmw={}), pytest.raises(GuardViolation) as e:
        launch(None, "fake_acc", x, y)
    assert (e.value.entry, e.value.arg) == ("fake_acc", 1)
    y = torch.full((N,), 5.0)
    with ctx(rmw={"fake_acc": {1: "accumulator by contract"}}):
        launch(None, "fake_acc", x, y)
    assert torch.equal(y, torch.full((N,), 6.0))   # accumulated once, not twice


def test_workspace_that_carries_state_between_entries():
    x, y, ws = torch.ones(N), torch.zeros(N), _ws()
    with ctx():   # plain scratch: what the first entry left is gone, and that is reported
        launch(None, "fake_keep", x, y, ws)
        with pytest.raises(GuardViolation) as e:
            launch(None, "fake_use_kept", x, y, ws)
    assert (e.value.entry, e.value.arg) == ("fake_use_kept", 1)
    x, y, ws = torch.ones(N), torch.zeros(N), _ws()
    carried = {"fake_keep": {3: ("out", "kept for fake_use_kept")},
               "fake_use_kept": {3: ("in", "left by fake_keep")},
               "fake_scratch_overrun": {3: ("out", "")}, "fake_stale_scratch": {3: ("out", "")}}
    with ctx(carried=carried):
        launch(None, "fake_keep", x, y, ws)
        launch(None, "fake_use_kept", x, y, ws)
    assert torch.equal(y, torch.full((N,), 4.0))
    with ctx(carried=carried), pytest.raises(GuardViolation) as e:   # still guarded ...
        launch(None, "fake_scratch_overrun", x, y, ws)
    assert e.value.arg == 3
    with ctx(carried=carried), pytest.raises(GuardViolation):   # ... and the producer still filled
        launch(None, "fake_stale_scratch", x, y, ws)


def test_only_a_tagged_tensor_is_scratch():
    """A 1-D uint8 tensor that did not come from the workspace helper is data:
    checked by (b) and copied back."""
    x = torch.arange(4 * N, dtype=torch.uint8).view(torch.float32)
    y = torch.zeros(4 * N, dtype=torch.uint8)
    with ctx():
        launch(None, "fake_shift", x, y)
    assert torch.equal(y.view(torch.float32), x + 1)


def test_oversized_output_prefix_written_tail_left():
    x, y = torch.ones(N), torch.full((N + 6,), 7.0)
    with ctx(), pytest.raises(GuardViolation):      # without a row the unwritten tail is reported
        launch(None, "fake_shift", x, y)
    tail = {"fake_shift": {1: ("sized for the larger of two uses", lambda a: 4 * a[2])},
            "fake_skip": {1: ("", lambda a: 4 * a[2])}, "fake_short": {1: ("", lambda a: 4 * a[2])}}
    y = torch.full((N + 6,), 7.0)
    with ctx(tail=tail):
        launch(None, "fake_shift", x, y)
    assert torch.equal(y[:N], torch.full((N,), 2.0)) and torch.equal(y[N:], torch.full((6,), 7.0))
    y = torch.full((N + 6,), 7.0)
    with ctx(tail=tail), pytest.raises(GuardViolation) as e:   # a hole inside the prefix still is
        launch(None, "fake_skip", x, y)
    assert (e.value.arg, e.value.offset) == (1, 4 * SKIPPED)
    y = torch.full((N + 6,), 7.0)
    with ctx(tail=tail), pytest.raises(GuardViolation) as e:   # so is a prefix that stops early
        launch(None, "fake_short", x, y)
    assert (e.value.arg, e.value.offset) == (1, 4 * (N - 1))


def test_adjacent_output_views_are_each_poisoned():
    buf = torch.zeros(2 * N)
    x, y = torch.ones(N), buf[N:]
    seen.clear()
    with ctx(), pytest.raises(GuardViolation) as e:   # x2 = buf[:N] is written too (fake_two)
        _abi.call("fake_two", _abi.ptr(x), _abi.ptr(buf[:N]), _abi.ptr(y), N, None)
    assert (e.value.entry, e.value.arg, e.value.offset) == ("fake_two", 2, 4 * SKIPPED)
    assert seen[0][2] - seen[0][1] == 4 * N          # one region: the views stay adjacent


def test_in_place_and_overlapping_views_relocate_consistently():
    x = torch.arange(N, dtype=torch.float32)
    seen.clear()
    with ctx() as g:
        launch(g, "fake_shift", x, x)
    assert torch.equal(x, torch.arange(N, dtype=torch.float32) + 1)   # once, not twice
    assert all(px == py for _, px, py, _ in seen)

    buf = torch.arange(12, dtype=torch.float32)
    a, b = buf[0:8], buf[4:12]
    seen.clear()
    with ctx() as g:
        launch(g, "fake_shift", a, b, n=8)
    assert all(py - px == 16 for _, px, py, _ in seen)
    assert torch.equal(buf, torch.tensor([0, 1, 2, 3, 1, 2, 3, 4, 5, 6, 7, 8], dtype=torch.float32))


def test_view_keeps_its_address_mod_256():
    buf = torch.zeros(N + 1)
    x, y = buf[1:], torch.zeros(N)
    assert x.data_ptr() == buf.data_ptr() + 4
    seen.clear()
    with ctx() as g:
        launch(g, "fake_double", x, y, _ws())
    for _, px, py, pw in seen:
        assert px % 256 == x.data_ptr() % 256 and py % 256 == y.data_ptr() % 256
    # the view is held to its own extent: buf[0] is not part of the relocated span
    with ctx(), pytest.raises(GuardViolation) as e:
        launch(None, "fake_before_start", y, x)
    assert (e.value.arg, e.value.offset, e.value.shape) == (1, -4, (N,))
    assert buf[0] == 0


def test_unrecorded_pointer_is_reported():
    x, y = torch.ones(N), torch.zeros(N)
    with ctx(), pytest.raises(UnguardedPointer, match="unguarded pointer: argument 1"):
        _abi.call("fake_double", _abi.ptr(x), y.data_ptr(), N, None, None)
    with ctx(), pytest.raises(UnguardedPointer, match="argument 0"):  # recorded before the previous call
        p = _abi.ptr(x)
        launch(None, "fake_double", x, y, _ws())
        _abi.call("fake_double", p, _abi.ptr(y), N, None, None)


def test_tables_name_real_entries_and_arguments():
    for name, rows in RMW.items():
        args = _abi.SIGNATURES[name][1]
        for i, reason in rows.items():
            assert args[i] is _vp and "mde_abi.h:" in reason, (name, i)
    for name, rows in list(CARRIED.items()) + list(TAIL.items()):
        args = _abi.SIGNATURES[name][1]
        for i, row in rows.items():
            assert args[i] is _vp and "mde_abi.h:" in (row[1] if name in CARRIED else row[0])
    for name, reason in list(INDIRECT.items()) + list(EXCLUDED.items()):
        assert name in _abi.SIGNATURES and reason
    assert "mde_abi.h:" in "".join(INDIRECT.values())


def test_every_pointer_taking_entry_has_a_guarded_case_or_an_excuse():
    from tests.test_gpu_abi_guard import declared_entries
    declared = declared_entries()
    assert not declared & set(EXCLUDED), declared & set(EXCLUDED)
    # every entry of the ABI is accounted for: a guarded case, or an excuse
    missing = set(_abi.SIGNATURES) - declared - set(EXCLUDED)
    assert not missing, f"ABI entries without a guarded case in test_gpu_abi_guard.py: {sorted(missing)}"
    # ... the guarded ones are exactly the pointer-taking entries without an excuse
    assert declared == launching_entries() - set(EXCLUDED), \
        sorted(declared ^ (launching_entries() - set(EXCLUDED)))
    # ... and only the graph entries are excused although they take a pointer
    assert {n for n in EXCLUDED if n in launching_entries()} == {
        n for n in _abi.SIGNATURES if n.startswith("mde_graph_")}


def _rows(check):
    from tests.test_gpu_abi_guard import FAMILIES
    return [kw for fam in FAMILIES if fam[1] == check for kw in fam[2]]


def test_conv1x1_rows_reach_every_kernel_instance():
    """The guarded conv1x1 rows select, by the dispatch rules mirrored in
    c1_variants, exactly the set of kernel instances the dispatchers hold."""
    from tests.test_gpu_abi_guard import C1_INSTANCES, c1_variants
    hit = set()
    for kw in _rows("test_conv1x1_vs_float64_oracle"):          # all three passes
        hit |= c1_variants(**kw)
    for kw in _rows("test_conv1x1_mix_small_writes_every_output"):   # forward and data gradient
        hit |= {v for v in c1_variants(kw["cin"], kw["cout"], 1, kw["h"], kw["w"])
                if v[0] == "mix_small"}
    assert hit == C1_INSTANCES, (sorted(C1_INSTANCES - hit, key=str), sorted(hit - C1_INSTANCES, key=str))


def test_wide_wgrad_rows_reach_every_strip_variant():
    """The workspace query only says the wide path takes a shape; which strip
    kernel it takes follows from the width rule mirrored in c3_wide_variant."""
    from tests.test_gpu_abi_guard import c3_wide_variant

    def census(check, stride):
        return {c3_wide_variant(k["cin"], k["cout"], stride, k["w"]) for k in _rows(check) if k["cin"] != 3}

    assert census("test_conv3x3_wide_wgrad_vs_float64_oracle", 1) == {
        (0, False), (80, False), (40, False), (20, False)}
    assert census("test_conv3x3_wide_wgrad_padded_channels_vs_float64", 1) == {
        (80, True), (40, True), (20, True)}          # padded channels: the strip kernels only
    assert census("test_conv3x3s2_wide_wgrad_vs_float64", 2) == {(40, False), (20, False)}
    assert census("test_conv3x3s2_wgrad_vs_float64", 2) == {("c32", 0), ("c32", 40)}
