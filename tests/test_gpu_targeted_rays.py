"""Every BVH walk of the device against brute force, on rays aimed AT the geometry (tests/targeted_rays.py): at vertices, at
points of edges, ending at the target, starting in box face planes, running along tile seams, and on every scene doubled (the
later copy must win every tie). The random rays of test_gpu_parity.py never come within ulps of a box face, where alone a
cull can be wrong; csrc/bvh_cull.h holds the argument these tests check.

The reference is the oracle's brute-force loop, which tests/test_targeted_rays_cpu.py anchors against the oracle's own BVH.
"""
import numpy as np
import pytest

import targeted_rays as T

pytestmark = pytest.mark.gpu

SCENE_NAMES = sorted(T.SCENES)


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def portable(oracle):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    return oracle


def _differ(dev, ref):
    return (np.ascontiguousarray(dev).view(np.uint32) != ref.view(np.uint32)).any(axis=1)


def _closest(r, mode, rays, ref, what):
    r.trace_mode(mode)
    bad = _differ(r.trace_closest(rays), ref)
    assert not bad.any(), f"{what} mode {mode!r}: {int(bad.sum())} of {len(rays)} rays differ from brute force, first {np.flatnonzero(bad)[:5]}"


def _any_hit(r, mode, rays, ref, what):
    r.trace_mode(mode)
    occ = r.trace_closest(rays)[:, 3].view(np.int32) >= 0
    hit = ref[:, 3].view(np.int32) >= 0
    assert (occ == hit).all(), f"{what} any-hit mode {mode!r}: {int((occ != hit).sum())} rays differ, {int((hit & ~occ).sum())} of them lost hits"


def _work_sharing(r, rays, ref, what):
    """trace_occluded_ws, also with a third of the lanes holding no ray (tmax < 0: they only help)"""
    hit = ref[:, 3].view(np.int32) >= 0
    occ, _, _ = r.trace_occluded_ws(rays)
    assert (occ == hit).all(), f"{what} work-sharing walk: {int((occ != hit).sum())} rays differ"
    holes = rays.copy()
    holes[::3, 7] = -1.0
    occ, _, _ = r.trace_occluded_ws(holes)
    want = hit.copy()
    want[::3] = False
    assert (occ == want).all(), f"{what} work-sharing walk with idle lanes: {int((occ != want).sum())} rays differ"


def _product_walks(api, r, rays, ref, what):
    M = api.TraceMode
    _closest(r, M.WIDE, rays, ref, what)
    for mode in (M.WIDE_ANY, M.OCCLUDED_LANE):
        _any_hit(r, mode, rays, ref, what)
    _work_sharing(r, rays, ref, what)
    r.trace_mode(M.WIDE)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_product_walks_equal_brute_force(api, portable, name):
    """the product library (builder 3): WIDE == brute force bit for bit (t, u, v, index); WIDE_ANY, OCCLUDED_LANE and the
    work-sharing walk are occluded iff brute force hits"""
    r = api.Renderer(8, 8)
    r.set_scene(T.make_tris(T.SCENES[name]))
    for dist in T.DISTS:
        rays, _, ref = T.reference(portable, name, dist)
        _product_walks(api, r, rays, ref, f"{name} dist {dist}")
    r.close()


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_every_builder_and_walk_equals_brute_force(api, portable, name):
    """the experiments library: builders 0 to 3, the binary stackless walk, the ray queue in both forms, four lanes per ray"""
    M = api.TraceMode
    for builder in (0, 1, 2, 3):
        r = api.Renderer(8, 8, exp=True)
        r.tuning(api.Tune.BVH_BUILDER, builder)
        r.set_scene(T.make_tris(T.SCENES[name]))
        for dist in T.DISTS:
            rays, _, ref = T.reference(portable, name, dist)
            what = f"{name} dist {dist} builder {builder}"
            for mode in (M.WIDE, M.BINARY, M.QUEUE_CLOSEST, M.CLOSEST_QUAD):
                _closest(r, mode, rays, ref, what)
            _any_hit(r, M.QUEUE_ANY, rays, ref, what)
        r.close()


def _tiles_with_big_quad():
    """(a) and one 8 x 8 quad half a unit under it: the tiles are all one size, this gives the pre-split something to cut"""
    big = np.asarray(T._quad((0, -0.5, 0), (8, 0, 0), (0, 0, 8)), np.float32)
    return np.concatenate([T.SCENES["a_tiles"], big])


@pytest.mark.parametrize("split", (0.0, None), ids=("no_presplit", "default_presplit"))
def test_presplit_fragments(api, portable, split):
    """rt_bvh_config split factor 0 and default: the fragments' boxes cull like any other"""
    v = _tiles_with_big_quad()
    r = api.Renderer(8, 8)
    if split is not None:
        r.bvh_config(split)
    r.set_scene(T.make_tris(v))
    for dist in T.DISTS:
        rays, _, _ = T.rays_for("a_tiles", dist, tri_v=v, seed_salt=11)
        ref = T.brute_force(portable, v, rays)
        assert (ref[:, 3].view(np.int32) >= 0).mean() >= 0.8
        _product_walks(api, r, rays, ref, f"tiles + 8x8 quad, split {split}, dist {dist}")
    r.close()


def test_after_scene_update(api, portable):
    """rt_scene_update moves the tiles of (a) by (+3, 0, -2) and then by (+0.1, 0, 0) more; the refit writes the same quantisation,
    and rays aimed at the MOVED triangles find what brute force over the new array finds"""
    v = T.SCENES["a_tiles"]
    r = api.Renderer(8, 8)
    r.set_scene(T.make_tris(v))
    for salt, shift in ((21, (3.0, 0.0, -2.0)), (22, (0.1, 0.0, 0.0))):
        v = (v + np.float32(shift)).astype(np.float32)
        r.update_scene(T.make_tris(v))
        for dist in T.DISTS:
            rays, _, _ = T.rays_for("a_tiles", dist, tri_v=v, seed_salt=salt)
            ref = T.brute_force(portable, v, rays)
            assert (ref[:, 3].view(np.int32) >= 0).mean() >= 0.8
            _product_walks(api, r, rays, ref, f"tiles moved by {shift}, dist {dist}")
    r.close()


def test_frame_with_the_eye_in_a_tile_plane(api, portable):
    """frame level: (a) under a lamp quad, 64 x 48, the eye exactly in the tile plane x = 4 and looking along it, so the middle
    pixel columns run along the seam x = 4 at grazing angles. Two frames with bench_options: RT_BUF_VISIBILITY and the
    accumulation equal the oracle's frame bit for bit (as test_random_triangle_soups_differential compares them)."""
    from cedec_2024_rt_amd.types import bench_options

    tris = T.make_tris(np.concatenate([T.SCENES["a_tiles"], np.asarray(T._quad((3, 3, 3), (2, 0, 0), (0, 0, 2)), np.float32)]))
    tris["emissive"][-2:] = 10.0
    W, H = 64, 48
    eye, center = (4.0, 2.0, 12.0), (4.0, 0.0, 0.0)
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(eye, center)
    r.set_options(bench_options())
    sc = portable.Scene(tris, use_bvh=True)
    rg = portable.raygen_lookat(eye, center, (0, 1, 0), np.float32(np.pi) / np.float32(4), W, H)
    assert rg.tobytes() == r.raygen().tobytes()
    st = portable.new_state(W, H)
    opt = portable.bench_options()
    for frame in (1, 2):
        r.frame(frame)
        sc.frame(W, H, frame, rg, np.asarray(eye, np.float32), opt, st)
        vis = r.download(api.RT_BUF_VISIBILITY)
        ref_vis = st["vis"].reshape(vis.shape)
        assert np.array_equal(np.ascontiguousarray(vis).view(np.uint8), np.ascontiguousarray(ref_vis).view(np.uint8)), f"visibility, frame {frame}"
        acc = r.download(api.RT_BUF_ACCUMULATION)
        bad = _differ(acc, np.ascontiguousarray(st["accum"].reshape(acc.shape)))
        assert not bad.any(), f"frame {frame}: {int(bad.sum())} pixels differ, first {np.flatnonzero(bad)[:5]}"
    assert (vis["index"] >= 0).mean() > 0.3  # the floor is on screen
    r.close()
