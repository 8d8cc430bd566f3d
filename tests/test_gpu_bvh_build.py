"""The device BVH build (csrc/bvh_build_device.h, builder 3) beyond "its tree answers like brute force", which any valid tree does.
Scenes and rays: tests/bvh_build_scenes.py; tests/test_bvh_build_scenes_cpu.py checks on the CPU that the brute-force reference
alone meets the hit fraction asserted here.

  A1  sizes on the borders of the three regimes (root of 2..5, 63..66, 4095..4098 references; forced first splits whose children
      are 64 | 65, 1 | 65, 4096 | 4097, 64 | 4097): every product walk == brute force, and the bounds on what the build reports.
  A2  the device tree IS the host builder's (builder 1, experiments library): record count, heights, SAH cost and the per-ray
      node / triangle counts of the closest-hit walk, which no two different trees share over 4096 rays.
  A3  centroid distributions that take the degenerate paths: one point, a line, a plane, two far clusters, an enclosing triangle.
  A4  the pre-split stays within 4 * triangles + 1024 references (csrc/bvh_fragment.h::frag_fit_length), and the bench scenes'
      trees are the ones every measurement was taken on.
"""
import math

import numpy as np
import pytest

import bvh_build_scenes as S
from test_gpu_targeted_rays import _product_walks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def portable(oracle):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    return oracle


def _tris(v):
    return S.T.make_tris(v)


def _build(api, v, split, builder=None):
    """builder None: the product library (builder 3); 1 or 3: the experiments library"""
    r = api.Renderer(8, 8, exp=builder is not None)
    if builder is not None:
        r.tuning(api.Tune.BVH_BUILDER, builder)
    if split is not None:
        r.bvh_config(split)
    r.set_scene(_tris(v))
    return r


def _tree(r, rays=None):
    info = r.bvh_info()
    now, at_build = r.bvh_cost()
    d = dict(info=info, height=r.scene_info()["bvh_height"], cost=now, at_build=at_build)
    if rays is not None:
        d["stats"] = r.trace_stats(rays).copy()
    return d


def _check_bounds(t, n_refs, what):
    """what the build reports: the reference count, the allocation bound of the records, a height the walks' stack holds, and
    a cost"""
    info = t["info"]
    print(f"{what}: {info}, binary height {t['height']}, cost {t['cost']!r}")
    assert info["references"] == n_refs, what
    assert n_refs + 1 <= info["wide_records"] <= 2 * n_refs + 8, what
    assert 3 * info["wide_height"] + 1 <= 64, what
    assert math.isfinite(t["cost"]) and t["cost"] > 0, what
    assert t["cost"] == t["at_build"], what


def _same_tree(a, b, what, stats=True):
    """COST_RTOL: rt_bvh_cost sums at most 2 n terms of magnitude at most 1 in float64, in the order the records lie in, which
    differs between the host's and the device's collapse: reordering moves the sum by at most n * 2^-53 < 1e-11 relative"""
    assert a["info"] == b["info"], f"{what}: {a['info']} != {b['info']}"
    assert a["height"] == b["height"], f"{what}: binary heights {a['height']} != {b['height']}"
    print(f"{what}: cost {a['cost']!r} against {b['cost']!r}")
    assert abs(a["cost"] - b["cost"]) <= 1e-9 * abs(b["cost"]), f"{what}: SAH cost {a['cost']!r} != {b['cost']!r}"
    if stats:
        bad = (a["stats"] != b["stats"]).any(axis=1)
        assert not bad.any(), (f"{what}: {int(bad.sum())} of {len(bad)} rays visit other node / triangle counts, first {np.flatnonzero(bad)[:5]}: "
                               f"{a['stats'][bad][:3].tolist()} != {b['stats'][bad][:3].tolist()}")


def _three_builds(api, v, rays, split, what, stats=True):
    """host builder 1 and device builder 3 of the experiments library, and the product library: the same tree"""
    trees = {}
    for key, builder in (("host", 1), ("device", 3), ("product", None)):
        r = _build(api, v, split, builder)
        trees[key] = _tree(r, rays)
        r.close()
    _same_tree(trees["device"], trees["host"], f"{what}: device builder 3 against host builder 1", stats)
    _same_tree(trees["product"], trees["device"], f"{what}: product library against experiments library", True)
    return trees


# ---------------------------------------------------------------- A1
@pytest.mark.parametrize("name", S.SOUPS + S.CLUSTERS)
def test_a1_regime_sizes(api, portable, name):
    """split off, so references == triangles and the sizes are exactly the regime borders"""
    v, rays, ref, split = S.reference(portable, name)
    assert split == 0.0
    r = _build(api, v, split)
    _product_walks(api, r, rays, ref, name)
    _check_bounds(_tree(r), len(v), name)
    r.close()


# ---------------------------------------------------------------- A2
@pytest.mark.parametrize("name", S.SOUPS + S.CLUSTERS + S.LARGE)
def test_a2_device_tree_is_the_host_tree(api, name):
    """Generic position: no two centroids share a coordinate and no two boxes an area, so every choice either builder makes (the
    first minimum over 3 x 31 planes, the larger child to open and the ascending-area child order of the collapse) has one
    answer, and the per-ray counts must be equal, not merely the totals. "large:*" has a few triangles of 50 median extents,
    which the default split factor cuts into fragments."""
    v, rays, split = S.scene(name)
    trees = _three_builds(api, v, rays, split, name)
    if name.startswith("large:") and len(v) > 2:  # of two triangles the larger one is the median: ten of its extents cut nothing
        assert trees["device"]["info"]["references"] > len(v), "nothing was split"
    else:
        assert trees["device"]["info"]["references"] == len(v)


# ---------------------------------------------------------------- A3
@pytest.mark.parametrize("name", S.DEGENERATE)
def test_a3_degenerate_centroids(api, portable, name):
    """Every axis of zero centroid extent is skipped (`!(ext > 0)`), and a node whose centroids all coincide is halved by
    position (SahSplit.axis = -1) in each of the three regimes.

    a_copies leaves per-ray counts out: all areas tie, and the collapse's child order among equal areas is the host sort's.
    b_concentric: a positional split of a medium or large node gives both halves the PARENT's box on the device (their own
    boxes are not known there), the host gives each half its own union: the device tree may be looser, never tighter
    (docs/MEASUREMENT_LOG_r18.md has the measured ratio); at 40 references the whole tree is one small subtree, whose
    wave reductions are exact, and the trees are equal."""
    v, rays, ref, split = S.reference(portable, name)
    kind = name.split(":")[1].split("@")[0]
    n = len(v)
    r = _build(api, v, split)
    _product_walks(api, r, rays, ref, name)
    product = _tree(r, rays)
    _check_bounds(product, n, name)
    r.close()
    h = _build(api, v, split, 1)
    host = _tree(h, rays)
    h.close()
    if kind == "b_concentric" and n > S.SAH_SMALL:
        print(f"{name}: device cost / host cost = {product['cost'] / host['cost']!r}")
        assert product["info"]["references"] == host["info"]["references"]
        assert product["cost"] >= host["cost"] * (1 - 1e-9), f"{name}: device cost {product['cost']!r} below the host's {host['cost']!r}"
    else:
        _same_tree(product, host, f"{name}: product (builder 3) against host builder 1", stats=kind != "a_copies")


# ---------------------------------------------------------------- A4
def test_a4_presplit_budget(api, portable):
    """bvh_build_scenes.budget_scene: the 16 steps of 1.5 x end at 41 078 references for 2000 triangles
    (tests/test_bvh_presplit_budget_cpu.py); the build goes on to a length that fits"""
    v, rays, ref, split = S.reference(portable, S.BUDGET)
    assert split == 10.0
    trees = {}
    for key, builder in (("host", 1), ("device", 3), ("product", None)):
        r = _build(api, v, split, builder)
        trees[key] = _tree(r, rays)
        if builder is None:
            refs = r.bvh_info()["references"]
            print(f"{S.BUDGET}: {refs} references, build {r.build_ms():.3f} ms")
            assert len(v) < refs <= 4 * len(v) + 1024
            _product_walks(api, r, rays, ref, S.BUDGET)
            _check_bounds(trees[key], refs, S.BUDGET)
        r.close()
    _same_tree(trees["device"], trees["host"], f"{S.BUDGET}: device builder 3 against host builder 1")
    _same_tree(trees["product"], trees["device"], f"{S.BUDGET}: product library against experiments library")


# bvh_info and bvh_cost of the two bench scenes as commit 01c51d0 builds them (the parent of the change that gave the
# pre-split's length search one owner), default split factor, product library, on an MI355X: the scenes every recorded frame
# time was measured on (docs/MEASUREMENT_LOG_r18.md)
BENCH_TREES = {
    "make_blocks_restir": (dict(references=252525, wide_records=380779, wide_height=15), 9.152963352276226),
    "make_blocks_pt": (dict(references=179259, wide_records=263866, wide_height=16), 13.460919940715721),
}


@pytest.mark.parametrize("scene_fn", sorted(BENCH_TREES))
def test_a4_bench_scene_trees_are_the_recorded_ones(api, scene_fn):
    """the counts are equal; the cost is a float64 sum whose order follows the order of atomics (k_refit_topo's list, k_bvh_cost's
    final adds), so two runs of one build differ in its last bits: the reordering bound of _same_tree applies, here with
    n = 380 779 records at most, 4e-11"""
    from cedec_2024_rt_amd import scenes

    want_info, want_cost = BENCH_TREES[scene_fn]
    r = api.Renderer(8, 8)
    r.set_scene(getattr(scenes, scene_fn)())
    info, (now, at_build) = r.bvh_info(), r.bvh_cost()
    print(f"{scene_fn}: {info}, cost {now!r}, build {r.build_ms():.3f} ms")
    r.close()
    assert info == want_info
    assert abs(now - want_cost) <= 1e-9 * want_cost and at_build == now
