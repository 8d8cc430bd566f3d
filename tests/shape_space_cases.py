"""Degenerate image shapes and thin strips, one table for the CPU test (tests/test_shape_space_cpu.py: the oracle alone, what keeps the
cases from passing vacuously) and the GPU tests (tests/test_gpu_shape_space.py: the device against the oracle).

The scene is `scenes.make_quad_room()`, the options go on top of `bench_options()` (temporal + spatial reuse on, 32 candidates, 5
neighbours, 3 passes), 3 frames. Every shape is seen from two views (`camera(view, W, H)`) and run with two radii (RADII). What each
shape is there for: SHAPES[(W, H)], in terms of the 8 x 8 one-wavefront tile of the tracing kernels (frame_kernels.h TileShape<64>),
the 32 x 8 four-wavefront tile of k_spatial_coop, and tile_grid / tile_pixel_at, which spread the tiles over the 8 XCDs.
"""
import math

import numpy as np

FRAMES = (1, 2, 3)

SHAPES = {
    (1, 1): "one pixel: 63 of 64 lanes of the only wavefront are off the image, three of four spatial wavefronts hold no pixel",
    (1, 9): "one column, two tile rows: every lane but lane 0 of each row is off the image in x",
    (9, 1): "one row, two 8 x 8 tiles: every tile row but the first is off the image in y",
    (2, 3): "six pixels in the corner of one tile, neither side a power of two",
    (7, 7): "one pixel short of the 8 x 8 tile in both directions",
    (8, 8): "exactly one 8 x 8 tile: a quarter of a 32 x 8 spatial tile",
    (9, 9): "one pixel past the 8 x 8 tile in both directions: four tracing tiles, three of them a single row or column",
    (31, 7): "one pixel short of the 32 x 8 spatial tile in both directions",
    (32, 8): "exactly one 32 x 8 spatial tile, four whole tracing tiles",
    (33, 9): "one pixel past the first 32 x 8 tile in both directions",
    (64, 1): "one row of exactly two spatial tiles: seven of eight lanes of every wavefront are off the image",
    (65, 2): "two rows, one pixel past two spatial tiles: the third spatial tile holds two pixels",
    (70, 5): "a short wide image, 9 tracing tiles in one tile row: one more than the 8 XCDs",
    (5, 70): "a narrow tall image, 9 tile rows of one tile: tile_rows decides the automatic order",
    (257, 3): "33 one-wavefront tiles in a row: one more than four rounds of the 8 XCDs",
    (3, 257): "33 tile rows of one tile each: the same count down the other axis",
}

VIEWS = ("floor", "mixed")
RADII = (30.0, 3.0)  # the default (most picks fall off these images: the bounds path); halo_rows_needed = 9 (picks land on the image)

PI_4 = np.float32(np.pi) / np.float32(4)
MIXED_EYE, MIXED_AT = (0.5, 2.5, 6.0), (0.0, 1.5, -1.0)  # the suite's usual view
FLOOR_EYE, FLOOR_AT = (0.3, 3.0, 2.0), (0.0, 0.0, 0.0)
ONE_PIXEL_EYE, ONE_PIXEL_AT = (0.5, 4.0, 3.0), (0.0, 0.0, -1.0)  # 1 x 1: FLOOR's single pixel lands on a lamp


# Where the rule below misses what the view is for (tests/test_shape_space_cpu.py asserts it on the oracle: `floor` all shaded, `mixed`
# with sky AND shaded pixels from 49 pixels on), the shape names a vertical field of its own:
# - floor, the three square shapes: at pi / 4 their bottom left pixel lands on a lamp (triangle 78); 0.7 rad keeps it on the floor;
# - mixed, the two tall shapes: at pi / 4 a slit 3 or 5 pixels wide and 70 or 257 tall sees the back wall alone (the reference's
#   camera scales the horizontal field with W / H); at 2.0 rad it reaches past the wall's upper edge: sky, wall, floor and a lamp.
FLOOR_FOVY = {(7, 7): np.float32(0.7), (8, 8): np.float32(0.7), (9, 9): np.float32(0.7)}
MIXED_FOVY = {(5, 70): np.float32(2.0), (3, 257): np.float32(2.0)}


def camera(view, W, H):
    """(eye, lookat, fovy as binary32) of a view at a shape. The reference's camera widens the horizontal field with W / H, so `floor`
    narrows the vertical one until the image's half-width spans at most 0.45 of the distance: every pixel then lands on the floor."""
    if view == "mixed":
        return MIXED_EYE, MIXED_AT, MIXED_FOVY.get((W, H), PI_4)
    assert view == "floor"
    if (W, H) == (1, 1):
        return ONE_PIXEL_EYE, ONE_PIXEL_AT, PI_4
    fovy = np.float32(2.0 * math.atan(min(math.tan(math.pi / 8.0), 0.45 * H / W)))
    return FLOOR_EYE, FLOOR_AT, FLOOR_FOVY.get((W, H), fovy)


def case_id(W, H, view=None, radius=None):
    s = f"{W}x{H}"
    if view is not None:
        s += f"_{view}"
    if radius is not None:
        s += f"_r{radius:g}"
    return s


ALL_CASES = [(W, H, view, radius) for (W, H) in SHAPES for view in VIEWS for radius in RADII]

# ---- subsets of the GPU file (tests/test_gpu_shape_space.py)
SHADOWED_ACCUMULATE_SHAPES = [(1, 9), (9, 1), (7, 7), (33, 9), (3, 257)]            # 3a, with use_shadowed_target_function and accumulate
FRAME_FORM_SHAPES = [(1, 1), (1, 9), (9, 1), (9, 9), (33, 9), (65, 2), (257, 3), (3, 257)]  # 3b, floor view, radius 3
TILE_ORDER_SHAPES = [(33, 9), (257, 3), (3, 257), (1, 1)]                                # 3b, every order on every tracing / spatial / resolve key
EXPERIMENT_SHAPES = [(1, 9), (9, 1), (9, 9), (33, 9), (257, 3), (3, 257)]                # 3c
RESTATED_MODE_SHAPES = [(1, 9), (9, 1), (7, 7), (33, 9)]                                 # 3d

# ---- thin strips (3f): name -> (W, H, radius, bounds). halo = ceil(strips.halo_bound(radius)): 0.3 -> 1 row, 3.0 -> 9, 10.0 -> 29.
STRIP_RADII = {0.3: 1, 3.0: 9, 10.0: 29}


def _even(halo, n):
    return [(k * halo, (k + 1) * halo) for k in range(n)]


STRIP_CASES = {
    # every strip exactly `halo` rows tall: the smallest partition_rows and rt_mg_create allow
    "w1_h1x4": (1, 4, 0.3, _even(1, 4)),
    "w33_h1x3": (33, 3, 0.3, _even(1, 3)),
    "w5_h9x3": (5, 27, 3.0, _even(9, 3)),
    "w65_h9x2": (65, 18, 3.0, _even(9, 2)),
    "w33_h29x3": (33, 87, 10.0, _even(29, 3)),
    "w64_h9x3": (64, 27, 3.0, _even(9, 3)),  # a width of whole 32-bit words: rt_halo_mark takes its LDS-window form, word window (x >> 5) - 3
    "w1_h29x2": (1, 58, 10.0, _even(29, 2)),
    # one taller strip with interior rows (more than two halos tall), thin ones around it
    "w5_h1_interior": (5, 9, 0.3, [(0, 1), (1, 8), (8, 9)]),
    "w33_h9_interior": (33, 45, 3.0, [(0, 9), (9, 36), (36, 45)]),
    "w65_h29_interior": (65, 90, 10.0, [(0, 29), (29, 90)]),
    # a last strip taller than the halo, at most two: its lower halo is clipped by the image edge, its boundary bands merge
    "w65_h1_clipped": (65, 5, 0.3, [(0, 1), (1, 3), (3, 5)]),
    "w1_h9_clipped": (1, 31, 3.0, [(0, 9), (9, 18), (18, 31)]),
    "w5_h29_clipped": (5, 90, 10.0, [(0, 29), (29, 58), (58, 90)]),
}
MG_FLAGS = (0, 1, 2, 4)      # sparse two lanes, RT_MG_DENSE, RT_MG_ONE_LANE, RT_MG_SEPARATE_PACK
