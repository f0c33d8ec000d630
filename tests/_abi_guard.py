"""Guard-band and stale-buffer harness for the raw-pointer C ABI.

`guarded_abi()` replaces `_abi.ptr` and `_abi.call` (the one choke point every
device pointer and every launch goes through) for the length of a `with` block.
Each launch is then run on relocated copies of its buffers, laid out as
[guard | span | guard] with the guards filled with 0xFF, and run twice from
identical inputs: once with scratch filled with 0xFF, once with scratch filled
with 0x5A and every region the first run wrote pre-filled with 0xA5.  It asserts

  (a) every guard byte is still 0xFF after both runs (no write outside a
      buffer, front or back, inputs, outputs and scratch alike);
  (b) both runs leave every non-scratch region byte-for-byte equal (no output
      element left unwritten, no result that depends on what an output or the
      scratch held before the call, no run-to-run non-determinism).

The first run's results are copied back, so the caller sees one ordinary call
and its own float64 / golden assertions prove that relocation changed nothing.

Scratch is what the product's workspace helper (`functional._ws`) returns: the
helper tags its tensors, and only a tagged tensor is treated as scratch.  A
test that allocates a workspace itself uses the helper.

What the harness cannot see: a read whose value is never used, a write that
lands beyond the guard, and memory reached through a device pointer table
(`INDIRECT`).  This is a plain helper module: no conftest, no pytest setting.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes

import torch

from monocular_depth_estimation_amd import _abi

GUARD = 0xFF      # NaN in fp32 and in bf16
POISON_OUT = 0xA5
SCRATCH_1 = 0xFF
SCRATCH_2 = 0x5A

_BN_RUNNING = "running statistics and *num_batches_tracked are updated in place"
_WINO_U = ("mde_wino_weight_bytes serves both transforms; one transform writes only its own padded "
           "extent and leaves the rest of u as it was (mde_abi.h:847-852)")
_DL_WS = ("the forward leaves the SSIM coefficients in the workspace and the backward reads them: "
          "the SAME workspace, unmodified (mde_abi.h:259-262)")

# entry -> {argument index: reason}; arguments that are read-modify-write by
# contract.  A row needs a sentence in include/mde_abi.h (cited).
RMW = {
    "mde_batchnorm_fwd_train": {
        4: _BN_RUNNING + " (mde_abi.h:286-288)", 5: _BN_RUNNING + " (mde_abi.h:286-288)",
        6: _BN_RUNNING + " (mde_abi.h:286-288)"},
    "mde_batchnorm_fwd_coef": {
        4: _BN_RUNNING + " (mde_abi.h:309-310)", 5: _BN_RUNNING + " (mde_abi.h:309-310)",
        6: _BN_RUNNING + " (mde_abi.h:309-310)"},
    "mde_batchnorm_fwd_train_stats": {
        4: _BN_RUNNING + " (mde_abi.h:335)", 5: _BN_RUNNING + " (mde_abi.h:335)",
        6: _BN_RUNNING + " (mde_abi.h:335)"},
    "mde_batchnorm_fwd_coef_stats": {
        4: _BN_RUNNING + " (mde_abi.h:335)", 5: _BN_RUNNING + " (mde_abi.h:335)",
        6: _BN_RUNNING + " (mde_abi.h:335)"},
}


def _wino_u_bytes(co, ci):
    """Bytes of one Winograd transform for the conv being RUN (ci -> co): 16 fp32
    per channel pair, co padded to 32 (16 stays 16), ci to 16 (mde_abi.h:847-852)."""
    co_p = 16 if co == 16 else -(-co // 32) * 32
    return 4 * 16 * co_p * (-(-ci // 16) * 16)


# entry -> {argument: (reason, bytes written as a function of the call's
# arguments)}: outputs whose buffer may be larger than what the entry writes.
# The written bytes are that prefix; the rest is left as it was.  Such an
# output is poisoned like any other: over the whole prefix both runs must agree
# (an element the entry skips, or a transform that stops early, is reported),
# and past it the first run must have left the caller's bytes alone.
TAIL = {
    # (weight, u, cin, cout, flip, stream): flip = the data gradient's conv cout -> cin
    "mde_wino_weight": {1: (_WINO_U, lambda a: _wino_u_bytes(a[2], a[3]) if a[4]
                            else _wino_u_bytes(a[3], a[2]))},
    # (weight, u, u_flip, cin, cout, stream)
    "mde_wino_weight2": {1: (_WINO_U, lambda a: _wino_u_bytes(a[4], a[3])),
                         2: (_WINO_U, lambda a: _wino_u_bytes(a[3], a[4]))},
}

# entry -> {workspace argument: ("out" | "in", reason)}: a workspace that carries
# state from one entry to the next by contract.  "out": filled like scratch
# before each run (the entry must not rely on what it held) and copied back to
# the caller; "in": an input -- never filled, restored between the runs.
CARRIED = {"mde_depth_loss_fwd": {10: ("out", _DL_WS)}, "mde_depth_loss_bwd": {12: ("in", _DL_WS)}}

# entries that reach memory through a device pointer table.  The table tensor is
# relocated and guarded like any argument; what its rows point to is not (the
# harness cannot substitute pointers stored in device memory), so those buffers
# are written in place, twice, without guards.
INDIRECT = {
    "mde_convbf_pack_table": "rows hold weight / pack pointers (mde_abi.h:949); the packs they "
                             "point to are written unguarded",
    "mde_wino_weight_table": "rows hold weight / u / u_flip pointers (mde_abi.h:880-886); the "
                             "transforms they point to are written unguarded",
}

# entries that launch nothing on tensors: passed through once, unguarded.
EXCLUDED = {
    "mde_graph_count_memsets": "graph introspection: takes a hipGraph_t, no tensor",
    "mde_graph_replace_memsets": "graph repair: takes a hipGraph_t, no tensor",
    "mde_graph_node_counts": "graph introspection: takes a hipGraph_t, no tensor",
    "mde_graph_node_types": "graph introspection: takes a hipGraph_t, no tensor",
    "mde_graph_dot": "graph introspection: takes a hipGraph_t and a path",
    "mde_timing_enable": "timing: host state only",
    "mde_timing_reset": "timing: host state only",
    "mde_timing_collect": "timing: resolves events, no tensor",
    "mde_timing_query": "timing: host out-parameters only",
    "mde_timing_query_flops": "timing: host out-parameter only",
    "mde_kernel_count": "timing: host query",
    "mde_kernel_name": "timing: host query",
    "mde_abi_version": "host query",
    "mde_status_string": "host query",
}
_QUERY_SUFFIXES = ("_supported", "_supported_n", "_workspace", "_blocks", "_bytes", "_elems",
                   "_mode", "_flops", "_route", "_instance", "_instance_count")
for _n, (_r, _a) in _abi.SIGNATURES.items():
    # shape / size / mode queries: host arithmetic, no pointer argument at all
    if _n.endswith(_QUERY_SUFFIXES) and not any(_t is ctypes.c_void_p for _t in _a):
        EXCLUDED.setdefault(_n, "host query: no pointer argument, launches nothing")


def launching_entries(signatures=None):
    """Entries of SIGNATURES with at least one c_void_p argument."""
    sig = _abi.SIGNATURES if signatures is None else signatures
    return {n for n, (_, args) in sig.items() if any(a is ctypes.c_void_p for a in args)}


class GuardViolation(AssertionError):
    """A launch wrote outside a buffer, or its two runs disagree."""

    def __init__(self, kind, entry, arg, shape, dtype, offset, detail=""):
        self.kind, self.entry, self.arg = kind, entry, arg
        self.shape, self.dtype, self.offset = tuple(shape), dtype, offset
        super().__init__(f"{entry}: {kind}: argument {arg} (shape {tuple(shape)}, {dtype}), "
                         f"first offending byte offset {offset}" + (f" -- {detail}" if detail else ""))


class UnguardedPointer(AssertionError):
    """A c_void_p argument that did not come from _abi.ptr since the last call."""


def _span_bytes(t) -> int:
    """Bytes from data_ptr up to and including the last addressed element."""
    if t.numel() == 0:
        return 0
    last = sum((s - 1) * abs(st) for s, st in zip(t.shape, t.stride()))
    return (last + 1) * t.element_size()


def _bytes_of(t, nbytes):
    """A flat uint8 alias of the first `nbytes` bytes at t.data_ptr()."""
    st = t.untyped_storage()
    off = t.data_ptr() - st.data_ptr()
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(st, off, (nbytes,), (1,))


def _is_scratch(t) -> bool:
    return getattr(t, "_mde_workspace", False)


class _Member:
    __slots__ = ("arg", "t", "start", "nbytes", "scratch", "off", "carried")

    def __init__(self, arg, t, start, nbytes, carried=None):
        self.arg, self.t, self.start, self.nbytes = arg, t, start, nbytes
        self.carried = carried            # None, "out" or "in"
        self.scratch = carried == "out" or (_is_scratch(t) and carried is None)
        self.off = 0


class _Region:
    def __init__(self, members, guard_bytes):
        self.members = members
        self.start = min(m.start for m in members)
        self.size = max(m.start + m.nbytes for m in members) - self.start
        for m in members:
            m.off = m.start - self.start
        self.scratch = all(m.scratch for m in members)
        self.args = sorted({m.arg for m in members})
        g = guard_bytes if guard_bytes is not None else min(max(64 << 10, self.size), 1 << 20)
        self.guard = g
        dev = members[0].t.device
        self.buf = torch.full((g + self.size + g + 256,), GUARD, dtype=torch.uint8, device=dev)
        base = self.buf.data_ptr() + g
        self.lo = g + (self.start - base) % 256          # interior keeps its address mod 256
        self.addr = self.buf.data_ptr() + self.lo
        self.interior = self.buf[self.lo:self.lo + self.size]
        self.front = self.buf[:self.lo]
        self.back = self.buf[self.lo + self.size:]
        for m in members:
            self.interior[m.off:m.off + m.nbytes].copy_(_bytes_of(m.t, m.nbytes))
        self.pre = self.interior.clone()

    def member_at(self, o):
        for m in self.members:
            if m.off <= o < m.off + m.nbytes:
                return m
        return self.members[0]

    def check_guards(self, entry, run):
        for side, g in (("front", self.front), ("back", self.back)):
            bad = g != GUARD
            if bool(bad.any()):
                k = int(bad.nonzero()[0])
                if side == "back":
                    m = max(self.members, key=lambda m: m.off + m.nbytes)
                    off = self.size + k - m.off
                    what = f"{off - m.nbytes} byte(s) past the end"
                else:
                    m = min(self.members, key=lambda m: m.off)
                    off = k - self.lo
                    what = f"{-off} byte(s) before the start"
                raise GuardViolation(f"write outside the buffer ({side} guard, run {run})", entry,
                                     m.arg, m.t.shape, m.t.dtype, off, what)


class Guard:
    """State of one guarded_abi() context: `calls` counts the entries called."""

    def __init__(self, invoke, guard_bytes, rmw, signatures, carried=None, tail=None):
        self.invoke, self.guard_bytes = invoke, guard_bytes
        self.rmw = RMW if rmw is None else rmw
        self.carried = CARRIED if carried is None else carried
        self.tail = TAIL if tail is None else tail
        self.signatures = _abi.SIGNATURES if signatures is None else signatures
        self.calls = collections.Counter()
        self.max_numel = 0        # largest non-scratch tensor seen
        self._recorded = {}

    @contextlib.contextmanager
    def paused(self):
        """The real `_abi.ptr` / `_abi.call` for the length of a block (an
        unguarded run to compare a guarded one with)."""
        mine = _abi.ptr, _abi.call
        _abi.ptr, _abi.call = self._real
        try:
            yield
        finally:
            _abi.ptr, _abi.call = mine

    # -- the two replacements ------------------------------------------------
    def ptr(self, t):
        if t is None:
            return None
        p = t.data_ptr()
        if not _is_scratch(t):   # a workspace is sized in bytes, not elements
            self.max_numel = max(self.max_numel, t.numel())
        self._recorded.setdefault(p, []).append(t)
        return p

    def call(self, name, *args):
        try:
            self._call(name, args)
        finally:
            self._recorded = {}

    # -- internals -------------------------------------------------------------
    def _stream(self):
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("guarded_abi cannot run during stream capture")
            return torch.cuda.current_stream().cuda_stream
        return None

    def _call(self, name, args):
        self.calls[name] += 1
        argtypes = self.signatures[name][1]
        if name in EXCLUDED or not any(a is ctypes.c_void_p for a in argtypes):
            return self.invoke(name, *args)
        stream = self._stream()
        members = []
        for i, (a, ty) in enumerate(zip(args, argtypes)):
            if ty is not ctypes.c_void_p or a is None or a == 0:
                continue
            if a in self._recorded:
                t = max(self._recorded[a], key=_span_bytes)
                n = _span_bytes(t)
                if n:
                    members.append(_Member(i, t, a, n, self.carried.get(name, {}).get(i, (None,))[0]))
            elif a == stream:
                continue
            elif name not in INDIRECT:
                raise UnguardedPointer(
                    f"{name}: unguarded pointer: argument {i} = {a:#x} is neither NULL, the "
                    "current stream, nor a pointer taken with _abi.ptr since the previous call")
        regions = self._regions(members)
        where = {}
        for r in regions:
            for m in r.members:
                where[m.arg] = (m.start, r.addr + m.off)
        new_args = [where[i][1] if i in where else a for i, a in enumerate(args)]
        rmw = self.rmw.get(name, {})
        tail = self.tail.get(name, {})
        on_gpu = any(m.t.is_cuda for m in members)

        def run(fill):
            for r in regions:
                if r.scratch:
                    r.interior.fill_(fill)
            if on_gpu:       # the fills above and the launch may be on different streams
                torch.cuda.synchronize()
            self.invoke(name, *new_args)
            if on_gpu:
                torch.cuda.synchronize()
            for r in regions:
                r.check_guards(name, 1 if fill == SCRATCH_1 else 2)
            return [r.interior.clone() for r in regions]

        def disagree(r, a, b, lo, hi, kind="the two runs disagree"):
            o = lo + int((a[lo:hi] != b[lo:hi]).nonzero()[0])
            m = r.member_at(o)
            raise GuardViolation(
                kind, name, m.arg, m.t.shape, m.t.dtype, o - m.off,
                f"run 1 byte {int(a[o]):#04x}, run 2 byte {int(b[o]):#04x} (0xa5: never "
                "written, or the entry reads its own output or its scratch before writing it)")

        r1 = run(SCRATCH_1)
        for r, a in zip(regions, r1):
            r.interior.copy_(r.pre)
            if r.scratch:
                continue
            # Poison what the first run wrote: every member whose bytes changed,
            # unless it is read-modify-write by contract or overlaps another
            # argument (in place: input and output at once -- restored only).
            for m in r.members:
                lo, hi = m.off, m.off + m.nbytes
                alone = not any(o is not m and o.off < hi and lo < o.off + o.nbytes for o in r.members)
                if (alone and m.arg not in rmw and m.carried is None
                        and not torch.equal(a[lo:hi], r.pre[lo:hi])):
                    r.interior[lo:hi].fill_(POISON_OUT)
        r2 = run(SCRATCH_2)
        for r, a, b in zip(regions, r1, r2):
            if r.scratch and not any(m.carried for m in r.members):
                continue
            if not r.scratch:
                m = r.members[0]
                if len(r.members) == 1 and m.arg in tail:
                    # the contract's prefix written in full, the rest untouched in run 1
                    end = int(tail[m.arg][1](args))
                    if end > r.size:
                        raise GuardViolation("buffer smaller than what the entry writes", name,
                                             m.arg, m.t.shape, m.t.dtype, r.size, f"{end} bytes")
                    if not torch.equal(a[:end], b[:end]):
                        disagree(r, a, b, 0, end)
                    if not torch.equal(a[end:], r.pre[end:]):
                        disagree(r, a, r.pre, end, r.size, "write past the written prefix")
                elif not torch.equal(a, b):
                    disagree(r, a, b, 0, r.size)
            for m in r.members:
                _bytes_of(m.t, m.nbytes).copy_(a[m.off:m.off + m.nbytes])

    def _regions(self, members):
        # Overlapping spans merge (in place, aliased arguments); adjacent ones merge
        # when they are views of one storage.  Separate allocations that merely
        # touch stay apart, so each keeps its own guards and its own poison.
        members = sorted(members, key=lambda m: m.start)
        groups, end = [], None
        for m in members:
            same = groups and any(m.t.untyped_storage().data_ptr() == o.t.untyped_storage().data_ptr()
                                  for o in groups[-1])
            if groups and (m.start < end or (m.start == end and same)):
                groups[-1].append(m)
                end = max(end, m.start + m.nbytes)
            else:
                groups.append([m])
                end = m.start + m.nbytes
        return [_Region(g, self.guard_bytes) for g in groups]


@contextlib.contextmanager
def guarded_abi(invoke=None, guard_bytes=None, rmw=None, signatures=None, carried=None, tail=None):
    """Run every `_abi.call` inside the block under guard (module docstring).

    invoke(name, *args): what performs a launch (default: the real `_abi.call`);
    guard_bytes: guard size on each side (default min(max(64 KiB, span), 1 MiB));
    rmw / carried / tail / signatures: replacements for RMW / CARRIED / TAIL / `_abi.SIGNATURES`
    (the host tests' fake entries).  Yields the Guard, whose `calls` counts the entries called."""
    real_ptr, real_call = _abi.ptr, _abi.call
    g = Guard(invoke or real_call, guard_bytes, rmw, signatures, carried, tail)
    g._real = (real_ptr, real_call)
    _abi.ptr, _abi.call = g.ptr, g.call
    try:
        yield g
    finally:
        _abi.ptr, _abi.call = real_ptr, real_call
