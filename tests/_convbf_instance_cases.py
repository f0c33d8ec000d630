"""Small cases for every compiled instance and patch-geometry edge of
csrc/convbf.hip (data only): checked against the launchers' own choice,
mde_convbf_instance, without a GPU (tests/test_convbf_instances.py) and run
against float64 (tests/test_gpu_convbf_instances.py, tests/_convbf_switch_child.py).

A case is ((n, cin, cout, h, w, ks, stride), instance id, properties): the
arguments of the FORWARD conv (the data-gradient entry takes the same ones),
the row of the pass's instance table (include/mde_abi.h) it is listed for, and
the geometry properties it is listed for -- each asserted from the query's
info record, never from a copy of the selection rules:

  flat / tile   patches are runs of mb pixels / pr x pc tiles
  pcol          tiles, partial last column only (wo % pc, not ho % pr)
  pband         tiles, partial last band only
  pboth         both at once
  clip          pr clipped to the plane's height (pr == ho < mb / pc)
  pcN           the tile width N
  exact         no partial patch: ho * wo % mb == 0 (flat), no partial tile
  per           more than one patch a block (resident kernel, weight gradient)
  short         ... and a short last block (blocks * per > np)
  span          ... and a block whose patches lie in two images
  cap           the staged image of the largest patch is at the capacity it is
                checked against, or the largest any swept shape attains under
                it (CAP_EDGE: capacity constant -> that img_px)
  capfull       img_px == the capacity exactly
  c32tile       weight gradient, cout % 64 != 0 (a half-empty M block) on tiles

The selection depends on the CU count (256 on the MI355X, and where there is
no device) through `per` / `blocks`; the GPU tests assert the id and the
properties again where they run.
"""

# forward / data-gradient table: 16 resident-filter rows, 30 chunked rows
#   0-2 1x1 S1, 3-5 1x1 S2, 6-8 1x1 U2: (WN1 NTW1), (WN2 NTW1), (WN2 NTW2)
#   9-11 3x3 S1; 12-13 3x3 S2, 14-15 3x3 U2: (WN1 NTW1), (WN2 NTW1)
#   16 + 5 * (3 * [ks == 3] + mode) + (WN1 MTW1, WN1 MTW2, WN2 MTW1, WN2 MTW2, WN2 MTW2 NW8)
FWD_CASES = [
    ((2, 32, 32, 5, 52, 1, 1), 0, ()),
    # persistent blocks with the statistics epilogue: one record a block, the last block short
    ((3, 32, 96, 4, 264, 1, 1), 0, ("tile", "exact", "per", "short", "span")),
    ((2, 32, 64, 4, 106, 1, 1), 1, ()),              # 424 staged pixels at 256: 128-pixel patches
    ((2, 32, 64, 5, 52, 1, 1), 2, ("flat",)),
    ((5, 32, 128, 4, 212, 1, 1), 2, ("tile", "pcol", "per", "short", "span")),
    ((2, 32, 32, 3, 264, 1, 2), 3, ()),
    ((2, 32, 64, 7, 212, 1, 2), 4, ()),
    ((2, 32, 64, 3, 264, 1, 2), 5, ()),
    ((2, 32, 32, 1, 136, 3, 1), 9, ("flat", "cap")),  # 3 x 140 staged pixels = kCapS1
    ((2, 32, 32, 7, 44, 3, 1), 9, ("pc4",)),
    ((2, 32, 32, 8, 64, 3, 1), 9, ("pc64",)),
    ((2, 32, 32, 17, 76, 3, 1), 9, ("pboth", "pc40")),
    ((2, 32, 64, 1, 200, 3, 1), 11, ("tile", "pcol", "clip", "pc32")),
    ((2, 32, 64, 4, 136, 3, 1), 11, ("pc8",)),
    ((2, 32, 64, 33, 136, 3, 1), 11, ("pboth", "pc20")),
    ((5, 32, 256, 2, 200, 3, 1), 11, ("pc16", "per", "short", "span")),
    ((2, 32, 32, 9, 56, 3, 2), 12, ("cap",)),         # 638 of kCapS2 = 640
    ((2, 32, 64, 17, 40, 3, 2), 13, ("pband", "pc20")),
    ((2, 32, 32, 4, 106, 1, 1), 16, ()),
    ((2, 1184, 32, 5, 52, 1, 1), 17, ()),
    ((2, 1184, 64, 2, 66, 1, 1), 19, ()),
    ((2, 32, 32, 7, 212, 1, 2), 21, ()),
    ((2, 1184, 32, 3, 264, 1, 2), 22, ()),
    ((2, 1184, 64, 1, 264, 1, 2), 24, ()),
    ((2, 32, 32, 4, 70, 3, 1), 31, ()),
    ((2, 160, 32, 1, 200, 3, 1), 32, ()),
    ((2, 32, 64, 4, 98, 3, 1), 33, ()),
    ((2, 160, 64, 2, 66, 3, 1), 34, ()),
    ((2, 32, 32, 31, 20, 3, 2), 36, ()),
    ((2, 160, 32, 1, 264, 3, 2), 37, ()),
    ((2, 32, 64, 7, 70, 3, 2), 38, ()),
    ((2, 160, 64, 17, 40, 3, 2), 39, ("pband", "pc20")),
]

DGRAD_CASES = [
    ((2, 32, 32, 5, 52, 1, 1), 0, ()),
    ((2, 64, 32, 4, 106, 1, 1), 1, ()),
    ((2, 64, 32, 5, 52, 1, 1), 2, ()),
    ((3, 96, 32, 4, 264, 1, 2), 6, ("tile", "exact", "clip", "pc8", "per", "short", "span")),
    ((2, 64, 32, 2, 264, 1, 2), 8, ("pc16",)),
    ((2, 64, 32, 17, 200, 1, 2), 8, ("pband", "pc40")),
    ((5, 64, 32, 8, 212, 1, 2), 8, ("tile", "exact", "clip", "pc4", "per", "short", "span")),
    ((2, 32, 32, 1, 200, 3, 1), 9, ()),
    ((2, 64, 32, 1, 200, 3, 1), 11, ()),
    ((2, 32, 32, 1, 212, 3, 2), 14, ("pcol", "pc32")),
    ((2, 32, 32, 2, 200, 3, 2), 14, ("pc16",)),
    ((2, 64, 32, 2, 64, 3, 2), 15, ()),
    ((2, 32, 32, 4, 106, 1, 1), 16, ()),
    ((2, 32, 1184, 5, 52, 1, 1), 17, ()),
    ((2, 64, 1184, 2, 66, 1, 1), 19, ()),
    ((2, 32, 1184, 6, 44, 1, 2), 27, ()),
    ((2, 64, 1184, 33, 4, 1, 2), 29, ()),
    ((2, 32, 32, 4, 70, 3, 1), 31, ()),
    ((2, 32, 160, 1, 136, 3, 1), 32, ("cap",)),
    ((2, 32, 160, 7, 44, 3, 1), 32, ("pc4",)),
    ((2, 32, 160, 8, 64, 3, 1), 32, ("pc64",)),
    ((2, 32, 160, 17, 76, 3, 1), 32, ("pboth", "pc40")),
    ((2, 64, 32, 4, 98, 3, 1), 33, ()),
    ((2, 64, 160, 2, 66, 3, 1), 34, ()),
    ((2, 32, 160, 1, 212, 3, 2), 42, ("tile", "pcol", "clip", "pc32")),
    ((2, 32, 160, 2, 200, 3, 2), 42, ("pc16",)),
    ((2, 32, 160, 4, 136, 3, 2), 42, ("pc8",)),
    ((2, 64, 160, 2, 64, 3, 2), 44, ("flat", "exact")),
]

# weight-gradient table: (ks, mode) = (1, S1), (1, S2), (3, S1), (3, S2)
WGRAD_CASES = [
    ((2, 32, 32, 2, 64, 1, 1), 0, ("flat", "exact")),
    ((2, 32, 32, 10, 212, 1, 1), 0, ("pc64",)),
    ((2, 32, 32, 1, 264, 1, 2), 1, ()),
    ((2, 32, 32, 5, 80, 3, 1), 2, ("cap",)),          # 588 of kCapS1W = 600
    ((2, 288, 288, 1, 200, 3, 1), 2, ("tile", "pcol", "clip", "pc32", "per", "short", "span", "c32tile")),
    ((2, 32, 32, 3, 136, 3, 2), 3, ("pc16",)),
    ((2, 32, 32, 5, 136, 3, 2), 3, ("pc40",)),
    ((2, 32, 32, 7, 72, 3, 2), 3, ("pc8",)),
    ((2, 32, 32, 17, 40, 3, 2), 3, ("pband", "pc20")),
    ((2, 32, 32, 25, 24, 3, 2), 3, ("pc4",)),
    ((2, 32, 32, 33, 72, 3, 2), 3, ("pboth",)),
]

# capacity constant -> the largest staged image the sweep of
# tests/test_convbf_instances.py finds under it (the "cap" cases attain it)
CAP_EDGE = {420: 420, 600: 588, 640: 638}

# Forward / data-gradient ids no shape reaches with the switches unset, and why.
ONLY_T21 = "only under MDE_CONVBF_RESMODE=t21: by default these shapes take the 256-pixel " \
           "patches (NTW 2) wherever the 128-pixel geometry exists -- 3x3 S1: the flat image of " \
           "256 pixels fits 600 wherever that of 128 fits 420; 1x1 U2: w % 4 == 0, tiles fit"
ONLY_NW8 = "only under MDE_CONVBF_NW8=1"
NO_SHAPE_11 = "no supported shape: the 1x1 image of a half-size patch is never smaller -- the " \
              "flat row count is the same at 128 and 64 pixels wherever 128 does not fit, and " \
              "tiles always fit"
NO_SHAPE_U2 = "no supported shape: a U2 plane has w % 4 == 0 (gy's width is even), so the " \
              "4-column tiles of the larger patch always fit"
UNREACHED = {
    7: ONLY_T21, 10: ONLY_T21,
    20: ONLY_NW8, 25: ONLY_NW8, 30: ONLY_NW8, 35: ONLY_NW8, 40: ONLY_NW8, 45: ONLY_NW8,
    18: NO_SHAPE_11, 23: NO_SHAPE_11, 28: NO_SHAPE_11, 26: NO_SHAPE_U2,
    41: NO_SHAPE_U2, 43: NO_SHAPE_U2,
}
UNREACHED_WGRAD = {}

# switch -> (environment, forward cases, data-gradient cases) for the ids that
# exist only under it; the child process also runs FWD_CASES / DGRAD_CASES
SWITCH_CASES = {
    "res0": ({"MDE_CONVBF_RES": "0"}, [], []),
    "t21": ({"MDE_CONVBF_RESMODE": "t21"},
            [((2, 32, 64, 2, 66, 3, 1), 10, ())],
            [((2, 64, 32, 33, 4, 1, 2), 7, ()), ((2, 64, 32, 2, 66, 3, 1), 10, ())]),
    # the 8-wave blocks need n * patches * (cout / 64) >= 512: large batches of small planes
    "nw8": ({"MDE_CONVBF_NW8": "1"},
            [((128, 1184, 256, 1, 4, 1, 1), 20, ()), ((128, 1184, 256, 1, 8, 1, 2), 25, ()),
             ((33, 160, 256, 1, 264, 3, 1), 35, ("tile",)), ((33, 160, 256, 3, 264, 3, 2), 40, ("tile",)),
             # the 8-wave capacities kCapS1W = 600 and kCapS2W = 1200, attained exactly
             ((11, 160, 1024, 8, 96, 3, 1), 35, ("flat", "capfull")),
             ((16, 160, 1024, 23, 46, 3, 2), 40, ("flat", "capfull"))],
            [((128, 256, 1184, 1, 4, 1, 1), 20, ()), ((128, 256, 1184, 1, 4, 1, 2), 30, ()),
             ((33, 256, 160, 1, 264, 3, 1), 35, ("tile",)), ((64, 256, 160, 1, 264, 3, 2), 45, ())]),
}

