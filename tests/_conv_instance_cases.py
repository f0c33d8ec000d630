"""One small case per row of the first-match instance tables of
csrc/conv3x3s2.hip (data only).  Position i of a list is the case for table
row i: the shape is confirmed by the library's own query, not by a copy of the
selection rules (tests/test_conv_instances.py, no GPU), and run against
float64 (tests/test_gpu_conv_instances.py).

Every case is (n, cin, cout, h, w), h and w the input sizes.  The shapes are
the smallest that still leave the kernel something to get wrong: several
pixel tiles per image with a ragged last one, odd heights (the data
gradient's missing last odd row), partial 2D tiles.
"""

# MDE_S2_FWD_GEOS: mde_conv3x3s2_fwd_instance / mde_conv3x3s2_fwd
S2_FWD_CASES = [
    (2, 32, 32, 5, 322),    # 0: 32 x 128, R 5, NJ 6 -- wo 161: wide, but no multiple of 32
    (2, 32, 64, 31, 130),   # 1: 64 x 128, R 7, NJ 3
    (2, 32, 64, 59, 70),    # 2: 64 x 128, R 11, NJ 2
    (2, 32, 64, 13, 38),    # 3: 64 x 64, R 11, NJ 1 -- planes under 1024 pixels
    (2, 32, 64, 21, 22),    # 4: 64 x 64, R 17, NJ 1 -- 7 output rows under a tile
    (2, 32, 32, 11, 256),   # 5: 32 x 128 in 2D tiles of 4 x 32 (wo 128), a partial tile row
    (2, 32, 64, 19, 256),   # 6: 64 x 128 in 2D tiles
    (2, 3, 32, 11, 256),    # 7: the stem's 3 input channels, 2D tiles
]

# MDE_S2_DGRAD_GEOS: mde_conv3x3s2_dgrad_instance / mde_conv3x3s2_bwd_data
S2_DGRAD_CASES = [
    (2, 32, 32, 5, 262),    # 0: 32 x 128, R 3, NJ 3
    (2, 64, 32, 5, 262),    # 1: 64 x 64, R 3, NJ 3
    (2, 32, 32, 7, 140),    # 2: 32 x 128, R 4, NJ 2
    (2, 64, 32, 5, 200),    # 3: 64 x 64, R 4, NJ 2
    (2, 64, 32, 13, 38),    # 4: 64 x 64, R 6, NJ 1
    (2, 64, 32, 21, 22),    # 5: 64 x 64, R 9, NJ 1
]

# MDE_S1_GEOS: mde_conv3x3_wide_instance.  Both passes produce `cout` channels
# from `cin`: pass 0 is the forward of the conv cin -> cout, pass 1 the data
# gradient of the mirrored conv cout -> cin (whose gx has cout channels), so
# one case selects the same row in both.  Rows 6 to 11 (the 2 x 2 wave tiles)
# need a grid of >= 512 blocks: the batch does that, not the plane.
S1_WIDE_CASES = [
    (2, 32, 32, 5, 130),      # 0: 32 x 128, R 4, NJ 3
    (2, 32, 64, 15, 70),      # 1: 64 x 128, R 5, NJ 2
    (2, 32, 64, 31, 34),      # 2: 64 x 128, R 7, NJ 1
    (2, 32, 64, 9, 21),       # 3: 64 x 64, R 7, NJ 1
    (2, 32, 64, 12, 11),      # 4: 64 x 64, R 10, NJ 1
    (2, 32, 64, 9, 130),      # 5: 64 x 128, R 4, NJ 3
    (104, 32, 32, 8, 130),    # 6: 32 x 256, R 5, NJ 3 -- 5 tiles an image, 520 blocks
    (32, 32, 128, 23, 78),    # 7: 64 x 256, R 7, NJ 2 -- 128 x 128 would give 480 blocks
    (32, 32, 128, 11, 163),   # 8: 64 x 256, R 5, NJ 3
    (128, 32, 128, 12, 42),   # 9: 128 x 128, R 7, NJ 1
    (32, 32, 128, 13, 148),   # 10: 128 x 128, R 4, NJ 3
    (32, 32, 128, 17, 113),   # 11: 128 x 128, R 5, NJ 2
]
