"""The oracle alone on every case of tests/shape_space_cases.py: what keeps the GPU comparisons of tests/test_gpu_shape_space.py from
passing vacuously (a device that equals an all-sky oracle frame, or one whose spatial passes never found a neighbour on a 1 x 9 image,
has shown nothing about the lanes that stay alive off the image). One printed line per case: pixels per class and pixels the
passes changed."""
import math

import numpy as np
import pytest

import shape_space_cases as ssc

_tris = None
_cache = {}


def oracle_case(oracle, W, H, view, radius, **optkw):
    """3 oracle frames of one case (portable math), cached: dict(scene, state, options, sky / shaded / emissive masks)"""
    global _tris
    from cedec_2024_rt_amd import scenes

    key = (W, H, view, radius, tuple(sorted(optkw.items())))
    if key not in _cache:
        if _tris is None:
            _tris = scenes.make_quad_room()
        eye, at, fovy = ssc.camera(view, W, H)
        oracle.set_math_mode(oracle.MATH_PORTABLE)
        sc = oracle.Scene(_tris, use_bvh=True)
        rg = oracle.raygen_lookat(eye, at, (0, 1, 0), fovy, W, H)
        st = oracle.new_state(W, H)
        opt = oracle.bench_options(spatial_resampling_radius=radius, **optkw)
        for frame in ssc.FRAMES:
            sc.frame(W, H, frame, rg, np.asarray(eye, np.float32), opt, st)
        idx = st["vis"]["index"]
        emissive = (idx >= 0) & np.isin(idx, sc.lights)
        _cache[key] = dict(scene=sc, st=st, opt=opt, sky=idx < 0, emissive=emissive, shaded=(idx >= 0) & ~emissive)
    return _cache[key]


def changed_by_the_passes(oracle, W, H, view, radius):
    """shaded pixels whose accumulation after frames 1..3 differs from the same frames without the spatial passes"""
    a = oracle_case(oracle, W, H, view, radius)
    b = oracle_case(oracle, W, H, view, radius, use_spatial_resampling=0)
    differ = (a["st"]["accum"].view(np.uint32) != b["st"]["accum"].view(np.uint32)).any(axis=1)
    assert not differ[~a["shaded"]].any()  # sky and lamps never depend on a reservoir
    return int(differ[a["shaded"]].sum())


def test_the_table_is_the_one_the_issue_asks_for():
    assert list(ssc.SHAPES) == [(1, 1), (1, 9), (9, 1), (2, 3), (7, 7), (8, 8), (9, 9), (31, 7), (32, 8), (33, 9), (64, 1), (65, 2),
                                (70, 5), (5, 70), (257, 3), (3, 257)]
    assert all(len(why) > 20 for why in ssc.SHAPES.values())
    assert max(W * H for W, H in ssc.SHAPES) == 771 and len(ssc.ALL_CASES) == 64
    assert ssc.RADII == (30.0, 3.0) and ssc.VIEWS == ("floor", "mixed")
    for shapes in (ssc.SHADOWED_ACCUMULATE_SHAPES, ssc.FRAME_FORM_SHAPES, ssc.TILE_ORDER_SHAPES, ssc.EXPERIMENT_SHAPES, ssc.RESTATED_MODE_SHAPES):
        assert set(shapes) <= set(ssc.SHAPES)
    from cedec_2024_rt_amd import strips

    for radius, halo in ssc.STRIP_RADII.items():
        assert math.ceil(strips.halo_bound(radius)) == halo
    assert math.ceil(strips.halo_bound(3.0)) == 9  # halo_rows_needed of the small radius of RADII
    kinds = {"x": 0, "interior": 0, "clipped": 0}
    for name, (W, H, radius, bounds) in ssc.STRIP_CASES.items():
        halo = ssc.STRIP_RADII[radius]
        assert W in (1, 5, 33, 64, 65) and H <= 90 and bounds[0][0] == 0 and bounds[-1][1] == H, name
        assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:])) and min(b - a for a, b in bounds) == halo, name
        heights = [b - a for a, b in bounds]
        if name.endswith("interior"):
            assert max(heights) > 2 * halo, name  # rows no neighbour's halo reaches
            kinds["interior"] += 1
        elif name.endswith("clipped"):
            assert halo < heights[-1] <= 2 * halo, name
            kinds["clipped"] += 1
        else:
            assert set(heights) == {halo}, name
            kinds["x"] += 1
    assert min(kinds.values()) >= 3 and {c[2] for c in ssc.STRIP_CASES.values()} == set(ssc.STRIP_RADII)
    assert {c[0] for c in ssc.STRIP_CASES.values()} == {1, 5, 33, 64, 65}


@pytest.mark.parametrize("W,H", list(ssc.SHAPES), ids=[ssc.case_id(W, H) for W, H in ssc.SHAPES])
def test_floor_view_is_all_shaded_and_the_passes_work(oracle, W, H):
    """every pixel of the `floor` view is shaded; with radius 3 the spatial passes change at least a quarter of them (where there are 8
    or more); the temporal history is live (some M above the candidate count) at both radii"""
    for radius in ssc.RADII:
        c = oracle_case(oracle, W, H, "floor", radius)
        n = int(c["shaded"].sum())
        changed = changed_by_the_passes(oracle, W, H, "floor", radius)
        m = c["st"]["temporal"]["M"][c["shaded"]]
        print(f"{ssc.case_id(W, H, 'floor', radius)}: sky {int(c['sky'].sum())} shaded {n} emissive {int(c['emissive'].sum())}; "
              f"changed by the passes {changed} of {n}; max temporal M {int(m.max()) if n else 0}")
        assert n == W * H and np.isfinite(c["st"]["accum"]).all()
        assert m.max() > int(c["opt"]["ris_sample_count"][0])
        if radius == 3.0 and n >= 8:
            assert 4 * changed >= n, (changed, n)


@pytest.mark.parametrize("W,H", list(ssc.SHAPES), ids=[ssc.case_id(W, H) for W, H in ssc.SHAPES])
def test_mixed_view_holds_sky_and_shaded_pixels(oracle, W, H):
    for radius in ssc.RADII:
        c = oracle_case(oracle, W, H, "mixed", radius)
        n = int(c["shaded"].sum())
        changed = changed_by_the_passes(oracle, W, H, "mixed", radius)
        m = c["st"]["temporal"]["M"][c["shaded"]]
        print(f"{ssc.case_id(W, H, 'mixed', radius)}: sky {int(c['sky'].sum())} shaded {n} emissive {int(c['emissive'].sum())}; "
              f"changed by the passes {changed} of {n}; max temporal M {int(m.max()) if n else 0}")
        assert np.isfinite(c["st"]["accum"]).all()
        if W * H >= 49:
            assert c["sky"].any() and n > 0
        if n:
            assert m.max() > int(c["opt"]["ris_sample_count"][0])
    if (W, H) == (33, 9):
        assert (int(c["sky"].sum()), n, int(c["emissive"].sum())) == (205, 91, 1)


def test_at_least_three_mixed_cases_hold_an_emissive_pixel(oracle):
    with_lamp = [(W, H) for W, H in ssc.SHAPES if oracle_case(oracle, W, H, "mixed", 30.0)["emissive"].any()]
    print("mixed cases with an emissive pixel:", with_lamp)
    assert len(with_lamp) >= 3


def test_default_radius_reaches_a_neighbour_only_on_the_long_images(oracle):
    """radius 30: the passes cannot change the single pixel of 1 x 1 (every neighbour is off the image or the pixel itself), and do
    change pixels of 3 x 257 and 257 x 3"""
    assert changed_by_the_passes(oracle, 1, 1, "floor", 30.0) == 0
    for W, H in ((3, 257), (257, 3)):
        n = changed_by_the_passes(oracle, W, H, "floor", 30.0)
        print(f"{W}x{H} radius 30: {n} pixels changed by the passes")
        assert n > 0


@pytest.mark.parametrize("case", list(ssc.STRIP_CASES))
def test_strip_cases_are_shaded_and_merge_across_rows(oracle, case):
    """the thin-strip cases in their `floor` view: most pixels shaded, and with the case's radius (0.3: a reach below one pixel, where only
    the truncation of a negative offset leaves the pixel) the passes still change pixels, so a halo record that did not arrive shows"""
    global _tris
    from cedec_2024_rt_amd import scenes

    W, H, radius, bounds = ssc.STRIP_CASES[case]
    if _tris is None:
        _tris = scenes.make_quad_room()
    eye, at, fovy = ssc.camera("floor", W, H)
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    sc = oracle.Scene(_tris, use_bvh=True)
    rg = oracle.raygen_lookat(eye, at, (0, 1, 0), fovy, W, H)
    out = []
    for spatial in (1, 0):
        st = oracle.new_state(W, H)
        opt = oracle.bench_options(spatial_resampling_radius=radius, use_spatial_resampling=spatial)
        for frame in ssc.FRAMES:
            sc.frame(W, H, frame, rg, np.asarray(eye, np.float32), opt, st)
        out.append(st)
    shaded = (out[0]["vis"]["index"] >= 0) & ~np.isin(out[0]["vis"]["index"], sc.lights)
    differ = (out[0]["accum"].view(np.uint32) != out[1]["accum"].view(np.uint32)).any(axis=1).reshape(H, W)
    # rows next to a strip boundary: the ones whose neighbours lie in another strip's rows
    edge_rows = sorted({r for a, b in bounds[1:] for r in (a - 1, a)})
    at_edges = int(differ[edge_rows].sum())
    print(f"{case}: {W}x{H} radius {radius:g}: shaded {int(shaded.sum())} of {W * H}; changed by the passes {int(differ.sum())}, {at_edges} of them in the rows at a strip boundary")
    assert 2 * int(shaded.sum()) > W * H and differ.sum() > 0 and at_edges > 0
