"""rt_scene_update with fragments that follow their triangle (csrc/bvh_fragment.h, csrc/bvh_refit.h) and rt_bvh_cost.

The build cuts large triangles into box fragments, one leaf each. A refit used to give every such leaf the WHOLE triangle's
box: exact (boxes only prune) and slow. Now a leaf gets the box of its own piece of the moved triangle. Scene "floor": a 16 x 16
quad of two triangles under 512 small ones, rt_bvh_config(4), so the two floor triangles hold some 900 fragments.
* walks after fragment-following refits == brute force (rigid move, rotation, 100x scale, mirror, collapse to a line and back,
  a span that separates the two floor triangles, two updates in a row), with rays aimed at the seams of the moved floor;
* vertical rays onto the moved floor test at most 16 triangles each (every leaf of both triangles before: several hundred);
* moving away and back gives the counters of an identity update: no drift;
* walk work and rt_bvh_cost after a rigid move against a rebuild, pinned to what was measured (docs/MEASUREMENT_LOG_r14.md);
* rt_bvh_cost's contract; the fallback (no pre-split, the experiments library's builder 1) is still exact.
"""
import ctypes as C

import numpy as np
import pytest

from cedec_2024_rt_amd.types import TRIANGLE, Tune
from test_gpu_scene_update import _check_walks, _random_rays

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_STATE = 0, 3
N_FLOOR = 2
TMAX = np.float32(3.402823466e38)

# measured on the MI355X for the rigid move of test_against_a_rebuild (docs/MEASUREMENT_LOG_r14.md section 2); the parent
# commit's walk ratio there is 118.40 (7 435 715 against 62 800 node visits + triangle tests)
WALK_RATIO_MEASURED = 1.0106  # 63 468 / 62 800
COST_RATIO_MEASURED = 1.0014  # 8.5312 / 8.5194


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def scenes():
    from cedec_2024_rt_amd import scenes as s
    return s


def floor_scene():
    """triangles 0, 1: the quad (-8, 0, -8) .. (8, 0, 8) as A B C / A C D; 512 triangles of extent <= 0.25 above it"""
    rng = np.random.default_rng(11)
    t = np.zeros(N_FLOOR + 512, TRIANGLE)
    t["v"][0] = [[-8, 0, -8], [8, 0, -8], [8, 0, 8]]
    t["v"][1] = [[-8, 0, -8], [8, 0, 8], [-8, 0, 8]]
    c = (rng.random((512, 1, 3), dtype=np.float32) * np.float32([14, 3, 14]) + np.float32([-7, 0.5, -7])).astype(np.float32)
    t["v"][N_FLOOR:] = (c + (rng.random((512, 3, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.25)).astype(np.float32)
    t["color"] = 0.5
    t["emissive"][5::64] = 2.0
    return t


def _all(tris):
    return np.ones(len(tris), bool)


def _floor_only(tris):
    m = np.zeros(len(tris), bool)
    m[:N_FLOOR] = True
    return m


def _map(tris, mask, fn):
    out = tris.copy()
    out["v"][mask] = fn(out["v"][mask]).astype(np.float32)
    return out


def _rot90x(v):
    return np.stack([v[..., 0], -v[..., 2], v[..., 1]], -1)


def floor_rays(tris, side=128):
    """side x side rays perpendicular to the floor as it lies now, through A + s (B - A) + t (D - A), s, t = k / side (on the
    original floor: coordinates on multiples of 1/8, where the fragments' seams are), both ways; and rays grazing it"""
    A, B, D = (tris["v"][0, 0].astype(np.float32), tris["v"][0, 1].astype(np.float32), tris["v"][1, 2].astype(np.float32))
    e1, e2 = B - A, D - A
    n = np.cross(e1, e2).astype(np.float32)
    ln = np.float32(np.sqrt((n * n).sum()))
    n = (n / ln).astype(np.float32) if ln > 0 else np.float32([0, 1, 0])  # a collapsed floor: any direction will do
    size = np.float32(max(float(np.abs(e1).max()), float(np.abs(e2).max()), 1.0))
    k = (np.arange(side, dtype=np.float32) / np.float32(side)).astype(np.float32)
    s, t = np.meshgrid(k, k)
    P = (A + s.reshape(-1, 1) * e1 + t.reshape(-1, 1) * e2).astype(np.float32)
    rays = np.zeros((side * side + 512, 8), np.float32)
    m = side * side
    up = (np.arange(m) % 2 == 0)[:, None]
    rays[:m, 0:3] = np.where(up, P + n * (np.float32(0.5) * size), P - n * (np.float32(0.5) * size))
    rays[:m, 3:6] = np.where(up, -n, n)
    # grazing: along the diagonal and along an edge, a hair above and tilted a hair towards the floor
    rng = np.random.default_rng(3)
    d = np.where((np.arange(512) % 2 == 0)[:, None], e1 + e2, e1).astype(np.float32)
    tilt = (rng.random((512, 1), dtype=np.float32) * np.float32(2e-3)).astype(np.float32)
    start = (A + rng.random((512, 1), dtype=np.float32) * e2 * np.float32(0.999)).astype(np.float32)
    rays[m:, 0:3] = start - d * np.float32(0.05) + n * (tilt * size * np.float32(0.5))
    rays[m:, 3:6] = d - n * (tilt * size)
    rays[:, 7] = TMAX
    return rays


def vertical_rays(side, offset):
    g = ((np.arange(side, dtype=np.float32) + np.float32(0.5)) / np.float32(side) * np.float32(15.0) - np.float32(7.5)).astype(np.float32)
    x, z = np.meshgrid(g + np.float32(offset[0]), g + np.float32(offset[2]))
    rays = np.zeros((side * side, 8), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2] = x.ravel(), 10.0, z.ravel()
    rays[:, 4] = -1.0
    rays[:, 7] = TMAX
    return rays


def _renderer(api, split=4.0, bfs=None, **kw):
    r = api.Renderer(8, 8, **kw)
    r.bvh_config(split)
    if bfs is not None:
        r.tuning(Tune.BVH_BFS_RECORDS, bfs)
    return r


def _update_sequence(scenes, tris):
    """(label, [(first, span), ...] calls, the whole array afterwards)"""
    fl, al = _floor_only(tris), _all(tris)
    out = []
    cur = scenes.move_triangles(tris, al, (0.5, 0.0, 0.25))
    out.append(("rigid move", [(0, cur)], cur))
    cur = _map(cur, fl, _rot90x)
    out.append(("floor rotated 90 degrees about x", [(0, cur)], cur))
    cur = _map(cur, fl, lambda v: v * np.float32(100.0))
    out.append(("floor scaled 100x", [(0, cur)], cur))
    cur = _map(cur, al, lambda v: v * np.float32([-1, 1, 1]))
    out.append(("mirrored", [(0, cur)], cur))
    line = _map(tris, fl, lambda v: v * np.float32([1, 1, 0]))
    out.append(("floor collapsed to a line", [(0, line)], line))
    cur = scenes.move_triangles(tris, al, (-0.25, 0.125, 0.375))
    out.append(("floor restored", [(0, cur)], cur))
    nxt = _map(cur, al, lambda v: _rot90x(v) + np.float32([0.0, 2.0, 0.0]))
    half = cur.copy()
    half[:1] = nxt[:1]
    out.append(("span [0, 1): one floor triangle of the two", [(0, nxt[:1])], half))
    out.append(("span [1, n): the other one and the clutter", [(1, nxt[1:])], nxt))
    mid = scenes.move_triangles(nxt, al, (3.0, 0.0, -2.0))
    end = _map(mid, fl, lambda v: v * np.float32(0.5))
    out.append(("two updates in a row", [(0, mid), (0, end[:N_FLOOR])], end))
    return out


@pytest.mark.parametrize("split,bfs", [(10.0, None), (4.0, None), (0.0, None), (4.0, 0)])
def test_walks_equal_brute_force_after_fragment_following_refits(api, oracle, scenes, split, bfs):
    tris = floor_scene()
    rng = np.random.default_rng(31)
    r = _renderer(api, split, bfs)
    r.set_scene(tris)
    info = r.bvh_info()
    if split == 4.0:
        assert info["references"] - len(tris) >= 200, info
    if split == 0.0:
        assert info["references"] == len(tris)
    hit_floor = []
    for label, calls, whole in _update_sequence(scenes, tris):
        for first, span in calls:
            r.update_scene(span, first)
        v = whole["v"].reshape(-1, 3)
        rays = np.concatenate([_random_rays(rng, 4096, v.min(0) - 0.5, v.max(0) + 0.5), floor_rays(whole)])
        _check_walks(r, whole, rays, oracle, f"split {split} bfs {bfs}: {label}")
        ref = r.trace_closest(rays[4096:4096 + 128 * 128])  # == brute force, just checked
        hit_floor.append((label, float((ref[:, 3].view(np.int32) >= 0).mean())))
        assert r.bvh_info() == info
    # the perpendicular grid does hit the floor wherever the floor has an area (a hole would be a miss against brute force
    # above; this guards the rays themselves)
    for label, share in hit_floor:
        if "line" not in label and "span [0, 1)" not in label:  # (a floor without area; A, B and D of two different planes)
            assert share > 0.9, (label, share)
    r.close()


def test_vertical_rays_onto_the_moved_floor_test_few_triangles(api, scenes):
    """After a rigid move of the whole scene by (0.5, 0, 0.25), 4096 vertical rays onto the floor: a mean of at most 16
    triangle tests per ray. Fragment boxes are grid cells of side <= L that tile each triangle, a point meets at most 4 cells
    of one tiling, there are two triangles, and a factor 2 covers quantisation slop and clutter. With whole-triangle boxes every
    ray meets every leaf of both floor triangles: the parent commit measures 922.86 tests per ray here and fails this test, this
    commit 1.08."""
    tris = floor_scene()
    r = _renderer(api)
    r.set_scene(tris)
    info = r.bvh_info()
    assert info["references"] - len(tris) >= 200, info
    d = (0.5, 0.0, 0.25)
    r.update_scene(scenes.move_triangles(tris, _all(tris), d))
    st = r.trace_stats(vertical_rays(64, d))
    mean_tests = float(st[:, 1].mean())
    print(f"mean triangle tests per ray after the move: {mean_tests:.2f} (nodes {float(st[:, 0].mean()):.2f})")
    r.close()
    assert mean_tests <= 16.0, mean_tests


def test_moving_away_and_back_does_not_drift(api, scenes):
    """B lies inside A's bounds, so the pad does not grow: A -> B -> A leaves the per-ray counters of A -> A."""
    tris = floor_scene()
    B = _map(tris, _all(tris), lambda v: v * np.float32(0.5) + np.float32([0.5, 0.25, 0.25]))
    rng = np.random.default_rng(41)
    v = tris["v"].reshape(-1, 3)
    rays = np.concatenate([vertical_rays(64, (0, 0, 0)), _random_rays(rng, 4096, v.min(0) - 0.5, v.max(0) + 0.5)])
    a = _renderer(api)
    a.set_scene(tris)
    a.update_scene(tris)
    want = a.trace_stats(rays)
    want_cost = a.bvh_cost()
    b = _renderer(api)
    b.set_scene(tris)
    for k in range(3):
        b.update_scene(B)
        b.update_scene(tris)
    got = b.trace_stats(rays)
    assert np.array_equal(got, want), f"{int((got != want).any(axis=1).sum())} rays count differently after moving away and back"
    assert b.bvh_cost()[0] == pytest.approx(want_cost[0], rel=1e-9)
    a.close()
    b.close()


def test_against_a_rebuild(api, scenes):
    """Rigid move: walk work (nodes + tests over the vertical and the random rays) and rt_bvh_cost of the refitted tree against
    a fresh context built on the moved array. Pinned at the measured ratios + 25 % (the counts are deterministic; the margin is for
    compiler-version differences in leaf batching)."""
    tris = floor_scene()
    d = (0.5, 0.0, 0.25)
    moved = scenes.move_triangles(tris, _all(tris), d)
    rng = np.random.default_rng(51)
    v = moved["v"].reshape(-1, 3)
    rays = np.concatenate([vertical_rays(64, d), _random_rays(rng, 4096, v.min(0) - 0.5, v.max(0) + 0.5)])
    r = _renderer(api)
    r.set_scene(tris)
    r.update_scene(moved)
    f = _renderer(api)
    f.set_scene(moved)
    work_r, work_f = int(r.trace_stats(rays).astype(np.int64).sum()), int(f.trace_stats(rays).astype(np.int64).sum())
    walk_ratio = work_r / work_f
    now, at_build = r.bvh_cost()
    fresh = f.bvh_cost()[1]
    cost_ratio = now / fresh
    print(f"walk ratio {walk_ratio:.4f} ({work_r} / {work_f}); cost ratio {cost_ratio:.4f} ({now:.4f} / {fresh:.4f}); now / at_build {now / at_build:.4f}")
    r.close()
    f.close()
    assert walk_ratio <= WALK_RATIO_MEASURED * 1.25, walk_ratio
    assert cost_ratio <= COST_RATIO_MEASURED * 1.25, cost_ratio


def test_bvh_cost_contract(api, scenes):
    tris = floor_scene()
    r = api.Renderer(8, 8)
    assert r.L.rt_bvh_cost(r.h, None, None) == RT_ERR_STATE  # no scene
    now, at = C.c_double(), C.c_double()
    assert r.L.rt_bvh_cost(r.h, C.byref(now), C.byref(at)) == RT_ERR_STATE
    r.bvh_config(4.0)
    r.set_scene(tris)
    assert r.L.rt_bvh_cost(r.h, None, None) == RT_OK  # NULL pointers are accepted
    assert r.L.rt_bvh_cost(r.h, C.byref(now), None) == RT_OK
    assert r.L.rt_bvh_cost(r.h, None, C.byref(at)) == RT_OK
    assert now.value > 1.0 and at.value == pytest.approx(now.value, rel=1e-9)  # equal before any update
    first, second = r.bvh_cost(), r.bvh_cost()
    assert first == (pytest.approx(now.value, rel=1e-9), pytest.approx(at.value, rel=1e-9))  # Renderer.bvh_cost mirrors the call
    assert second[0] == pytest.approx(first[0], rel=1e-9) and second[1] == pytest.approx(first[1], rel=1e-9)
    r.update_scene(tris)  # an identity update: the same pad, the same boxes up to the rounding of the fragments' evaluation
    n1, a1 = r.bvh_cost()
    assert a1 == pytest.approx(at.value, rel=1e-9), "at_build is the cost before the first refit"
    assert n1 == pytest.approx(at.value, rel=1e-3)
    # the small triangles trade places at random inside the same bounds: every low inner box now spans the scene
    shuffled = tris.copy()
    shuffled[N_FLOOR:] = tris[N_FLOOR:][np.random.default_rng(71).permutation(len(tris) - N_FLOOR)]
    r.update_scene(shuffled)
    n2, a2 = r.bvh_cost()
    assert a2 == pytest.approx(at.value, rel=1e-9)
    assert n2 > 2.0 * a2, (n2, a2)
    r.update_scene(tris)
    n3, a3 = r.bvh_cost()
    assert a3 == pytest.approx(at.value, rel=1e-9) and n3 == pytest.approx(n1, rel=1e-9), "back where it was: no drift"
    r.set_scene(shuffled)
    n4, a4 = r.bvh_cost()
    assert n4 == pytest.approx(a4, rel=1e-9) and n4 < 0.5 * n2, "rt_scene_set starts over"
    r.close()
    assert hasattr(api.load_library(exp=True), "rt_bvh_cost")


@pytest.mark.parametrize("exp_builder", [None, 1])
def test_fallback_without_a_fragment_table(api, oracle, scenes, exp_builder):
    """rt_bvh_config(0) on the product, builder 1 (host SAH, host collapse) of the experiments library: every leaf of a triangle
    gets the whole triangle's box, as before; updates still equal brute force and rt_bvh_cost works."""
    tris = floor_scene()
    rng = np.random.default_rng(61)
    if exp_builder is None:
        r = _renderer(api, 0.0)
    else:
        r = _renderer(api, 4.0, exp=True)
        r.tuning(Tune.BVH_BUILDER, exp_builder)
    r.set_scene(tris)
    c0 = r.bvh_cost()
    assert c0[0] > 1.0 and c0[0] == pytest.approx(c0[1], rel=1e-9)
    for label, calls, whole in _update_sequence(scenes, tris)[:2]:
        for first, span in calls:
            r.update_scene(span, first)
        v = whole["v"].reshape(-1, 3)
        rays = np.concatenate([_random_rays(rng, 4096, v.min(0) - 0.5, v.max(0) + 0.5), floor_rays(whole, 64)])
        _check_walks(r, whole, rays, oracle, f"fallback {exp_builder}: {label}")
    c1 = r.bvh_cost()
    assert c1[1] == pytest.approx(c0[1], rel=1e-9) and c1[0] > 0.0
    r.close()


def test_restir_app_prints_the_cost_ratio_after_its_last_update(tmp_path, api, scenes):
    """restir_app --move-lights prints rt_bvh_cost's now / at_build once, after the last update: the figures the Renderer
    reports when driven through the same updates (printed with four decimals)."""
    import os
    import re
    import subprocess

    from test_gpu_scene_update import APP, AT, EYE

    A = scenes.make_quad_room()
    path = os.path.join(str(tmp_path), "room.tris")
    A.tofile(path)
    d = (0.25, -0.125, 0.5)
    cmd = [APP, "--example", "10", "--tris", path, "--size", "32", "32", "--eye", *map(str, EYE), "--lookat", *map(str, AT),
           "--frames", "3", "--move-lights", *map(str, d)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = re.findall(r"^bvh cost now / at build: ([0-9.]+) / ([0-9.]+) = ([0-9.]+)$", p.stdout, re.M)
    assert len(lines) == 1, p.stdout
    now, at_build, ratio = map(float, lines[0])
    assert p.stdout.index("frame 3 scene update:") < p.stdout.index("bvh cost now")
    lights = scenes.light_indices(A)
    lmask = np.zeros(len(A), bool)
    lmask[lights] = True
    lo, hi = int(lights.min()), int(lights.max()) + 1
    r = api.Renderer(32, 32)
    r.set_scene(A)
    cur = A
    for _ in range(2):
        cur = scenes.move_triangles(cur, lmask, d)
        r.update_scene(cur[lo:hi], lo)
    want = r.bvh_cost()
    r.close()
    assert now == pytest.approx(want[0], abs=1e-4) and at_build == pytest.approx(want[1], abs=1e-4)
    assert ratio == pytest.approx(want[0] / want[1], abs=2e-3)
