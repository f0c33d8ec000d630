"""Small cases for every compiled instance and layout edge of csrc/dwconv.hip
(data only): checked against the launchers' own choice record,
mde_dwconv_instance, without a GPU (tests/test_dwconv_instances.py) and run
against float64 (tests/test_gpu_dwconv.py).

A case is ((n, c, h, w, k, stride, pad), forward id, backward id, forward
fields, backward fields): the rows of the two instance tables
(include/mde_abi.h) and the fields of the info record (MDE_DW_I_*, by their
names in _abi.DWCONV_INFO) the case is listed for.  Backward fields are those
of a call that requests gx and gw; "path" and "reducer" are given by name.

Instance tables (rows 0-11 in both passes, (K, S, V, EDGE)):
   0 (3,1,4,E)   1 (3,1,4,-)   2 (3,1,8,-)    3 (3,2,2,E)   4 (3,2,2,-)   5 (3,2,4,-)
   6 (5,1,4,E)   7 (5,1,4,-)   8 (5,1,8,-)    9 (5,2,2,E)  10 (5,2,2,-)  11 (5,2,4,-)
  12-15 strip k3s1, k3s2, k5s1, k5s2 (forward: every shape that does not
  stream, any padding; backward: padding k/2); 16-19, backward only: the split
  data- / weight-gradient kernels of the other paddings.
"""


def _s(v, rb, edge, l, nseg, nb, **kw):
    return dict(path="stream", v=v, rb=rb, edge=edge, l=l, spw=64 // l, nseg=nseg, nb=nb, **kw)


def _stream(shape, row, v, rb, edge, l, nseg, nb, wpb, it=1, g=1, **bwd):
    """A streaming case: the same instance and segment layout in both passes."""
    red = "fold" if g > 1 else "none"
    return (shape, row, row, _s(v, rb, edge, l, nseg, nb),
            _s(v, rb, edge, l, nseg, nb, wpb=wpb, it=it, g=g, reducer=red, **bwd))


# every streaming instance at n = 2, c = 3; stride 2 with odd heights (the
# last band's store and row guards), EDGE segments of 1, 2 and 20 lanes
STREAM_CASES = [
    _stream((2, 3, 9, 160, 3, 1, 1), 2, 8, 4, 0, 20, 1, 3, wpb=2),
    _stream((2, 3, 9, 160, 5, 1, 2), 8, 8, 4, 0, 20, 1, 3, wpb=2),
    _stream((2, 3, 5, 32, 3, 1, 1), 1, 4, 8, 0, 8, 1, 1, wpb=1),
    _stream((2, 3, 9, 16, 3, 1, 1), 1, 4, 8, 0, 4, 1, 2, wpb=1),
    _stream((2, 3, 5, 92, 5, 1, 2), 6, 4, 8, 1, 1, 23, 1, wpb=1),      # cg = 23: one-lane segments
    _stream((2, 3, 9, 184, 3, 1, 1), 0, 4, 8, 1, 2, 23, 2, wpb=3),
    _stream((2, 3, 9, 168, 3, 2, 1), 5, 4, 2, 0, 21, 1, 3, wpb=2, ho=5),
    _stream((2, 3, 15, 160, 5, 2, 2), 11, 4, 2, 0, 20, 1, 4, wpb=3, ho=8),
    _stream((2, 3, 9, 320, 3, 2, 1), 3, 2, 4, 1, 20, 4, 2, wpb=6, ho=5),
    _stream((2, 3, 9, 320, 5, 2, 2), 9, 2, 4, 1, 20, 4, 2, wpb=6, ho=5),
    _stream((2, 3, 15, 40, 3, 2, 1), 4, 2, 4, 0, 10, 1, 2, wpb=1, ho=8),
    _stream((2, 3, 7, 32, 3, 2, 1), 4, 2, 4, 0, 8, 1, 1, wpb=1, ho=4),
    _stream((2, 3, 7, 80, 5, 2, 2), 10, 2, 4, 0, 20, 1, 1, wpb=1, ho=4),
    _stream((2, 3, 11, 40, 5, 2, 2), 10, 2, 4, 0, 10, 1, 2, wpb=1, ho=6),
    # degenerate planes: h < k, a single lane a row (L = 1 without EDGE)
    _stream((2, 3, 1, 4, 3, 1, 1), 1, 4, 8, 0, 1, 1, 1, wpb=1, ho=1),
    _stream((2, 3, 2, 8, 5, 1, 2), 7, 4, 8, 0, 2, 1, 1, wpb=1, ho=2),
    _stream((2, 3, 1, 4, 5, 2, 2), 10, 2, 4, 0, 1, 1, 1, wpb=1, ho=1, wo=2),
    _stream((3, 5, 3, 8, 3, 2, 1), 4, 2, 4, 0, 2, 1, 1, wpb=1, ho=2),
    _stream((2, 3, 9, 4, 3, 2, 1), 4, 2, 4, 0, 1, 1, 2, wpb=1, ho=5),
]

# the backward layout: a whole channel in one 8-wave block; a channel split
# over G blocks (G > 1: the partials are folded by the gx launch, or summed by
# dw_wsum_kernel when only gw is requested), G > 64 (the second trip of the
# wave's partial loop), and IT > 1 with a short tail group (IT G WPB SPW > UPC
# by more than one block's units)
LAYOUT_CASES = [
    _stream((2, 3, 20, 260, 3, 1, 1), 0, 4, 8, 1, 13, 5, 3, wpb=8, upc=30),
    _stream((3, 2, 40, 320, 3, 1, 1), 0, 4, 8, 1, 20, 4, 5, wpb=4, g=5, upc=60, ws=4 * 2 * 5 * 9),
    _stream((3, 2, 40, 336, 5, 1, 2), 6, 4, 8, 1, 14, 6, 5, wpb=4, g=6, upc=90, ws=4 * 2 * 6 * 25),
    _stream((3, 2, 80, 320, 3, 2, 1), 3, 2, 4, 1, 20, 4, 10, wpb=4, g=10, upc=120),
    _stream((10, 2, 32, 80, 3, 2, 1), 4, 2, 4, 0, 20, 1, 4, wpb=4, g=4, upc=40),
    _stream((4, 2, 392, 320, 3, 1, 1), 0, 4, 8, 1, 20, 4, 49, wpb=4, g=66, upc=784),
    _stream((25, 2048, 2, 80, 5, 1, 2), 7, 4, 8, 0, 20, 1, 1, wpb=4, it=2, g=2, upc=25),
]


def _strip(shape, row, fwd, bwd):
    return (shape, row, row, dict(path="strip", **fwd), dict(path="strip", **bwd))


# strip kernels (padding k/2, planes that do not stream): stride 2 with 2 x 2
# tiles a plane, a partial last stack of planes (forward: n c % pb, backward:
# n % pb), G > 1 at every (k, stride)
STRIP_CASES = [
    _strip((3, 3, 59, 135, 3, 2, 1), 13, dict(tw=34, th=28, pb=1, tx=2, ty=2),
           dict(tx=2, ty=2, pb=1, g=12, reducer="wreduce")),
    _strip((3, 3, 59, 135, 5, 2, 2), 15, dict(tw=34, th=28, pb=1, tx=2, ty=2),
           dict(tx=2, ty=2, pb=1, g=12, reducer="wreduce")),
    _strip((30, 1, 7, 9, 3, 2, 1), 13, dict(pb=28, blocks=2), dict(pb=28, g=2, reducer="wreduce")),
    _strip((7, 5, 6, 6, 5, 1, 2), 14, dict(pb=10, blocks=4), dict(pb=7, g=1, reducer="none")),
    _strip((3, 11, 4, 6, 3, 1, 1), 12, dict(pb=28, blocks=2), dict(pb=3, g=1, reducer="none")),
    _strip((2, 3, 21, 70, 5, 1, 2), 14, dict(tw=35, tx=2, ty=1, pb=1),
           dict(tx=2, ty=1, pb=1, g=4, reducer="wreduce")),
    _strip((2, 5, 17, 130, 3, 1, 1), 12, dict(tw=44, tx=3, ty=1, pb=1),
           dict(tx=3, ty=1, pb=1, g=6, reducer="wreduce")),
]


def _split(shape, ks, fwd, bwd):
    return (shape, 12 + ks, 16 + ks, dict(path="strip", **fwd),
            dict(path="split", reducer="wreduce", **bwd))


# other paddings: the forward is the strip kernel, the backward the split
# kernels.  The four shapes of test_dwconv_other_padding, a stride-2 plane of
# several tiles in both gradients, padding 0 at the smallest legal plane
SPLIT_CASES = [
    _split((2, 8, 30, 41, 5, 2, 1), 3, dict(pb=3), dict(tx=1, ty=2, tx2=1, ty2=1, p=2)),
    _split((2, 8, 30, 41, 3, 1, 0), 0, dict(pb=1, ty=2), dict(tx=1, ty=2, tx2=1, ty2=2, p=4)),
    _split((1, 6, 19, 70, 5, 1, 4), 2, dict(tx=2), dict(tx=2, ty=1, tx2=2, ty2=1, p=2)),
    _split((1, 4, 16, 16, 3, 2, 2), 1, dict(pb=4), dict(tx=1, ty=1, tx2=1, ty2=1, p=1)),
    _split((2, 3, 70, 150, 5, 2, 1), 3, dict(tx=2, ty=2), dict(tx=3, ty=4, tx2=2, ty2=2, p=8)),
    _split((2, 3, 3, 3, 3, 2, 0), 1, dict(ho=1, wo=1, pb=6), dict(tw=3, th=3, tw2=1, th2=1, p=2)),
    _split((2, 3, 5, 5, 5, 1, 0), 2, dict(ho=1, wo=1, pb=6), dict(tw=5, th=5, tw2=1, th2=1, p=2)),
]

ALL_CASES = STREAM_CASES + LAYOUT_CASES + STRIP_CASES + SPLIT_CASES

# rows no case reaches: {(pass, id): reason}
UNREACHED = {}

# values the lists must show somewhere (tests/test_dwconv_instances.py)
WPB_VALUES = {1, 2, 3, 4, 6, 8}


def case_id(shape):
    n, c, h, w, k, s, p = shape
    return f"{n}x{c}x{h}x{w}-k{k}s{s}p{p}"
