"""rt_scene_update (include/restir_rt_internal.h): triangles replaced in place, the 4-wide tree refitted on the device
(csrc/bvh_refit.h) — the counterpart of HIPRT's hiprtBuildOperationUpdate.

The parity contract makes a refit checkable bit for bit: a walk's answer is the brute-force closest hit over all triangles
whatever tree is walked, so after an update every result equals what rt_scene_set on the new array gives.
* walks on refitted trees (rigid moves, jitter, a block thrown far across the scene, a sub-range, two updates in a row)
  == brute force, every trace mode of the product, every builder of both libraries; rt_bvh_info unchanged;
* ReSTIR DI frame sequences across updates (lights moved, a block moved, lights switched on / off) == the oracle,
  accumulation, pixels and temporal history;
* 12 back-to-back frames with updates in between == the oracle;
* path tracing (07 / 08 / 09) and AO (06) after an update == a fresh context built on the new array;
* strip contexts updated between frames == a single context;
* the deep-traversal deck deformed and refitted == brute force;
* error codes; restir_app --move-lights == the Python Renderer.
"""
import os
import subprocess

import numpy as np
import pytest

from cedec_2024_rt_amd.types import TraceMode, Tune

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "app", "restir_app")
FOVY = np.float32(np.pi) / np.float32(4)
RT_OK, RT_ERR_ARG, RT_ERR_STATE = 0, 1, 3
EYE, AT = np.float32([0.5, 2.5, 6.0]), np.float32([0.0, 1.5, -1.0])
QUAD_ROOM_BOX = slice(64, 76)  # make_quad_room: floor (32) + wall (32), then the box (12), then the lights


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def scenes():
    from cedec_2024_rt_amd import scenes as s
    return s


@pytest.fixture(scope="module")
def golden_scenes(golden_dir):
    return np.load(os.path.join(golden_dir, "scenes.npz"))


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _diff(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).reshape(len(a), -1).any(axis=1).sum())


def _random_rays(rng, n, lo, hi):
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = (rng.random((n, 3), dtype=np.float32) * (hi - lo) + lo).astype(np.float32)
    rays[:, 3:6] = (rng.random((n, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    rays[:, 7] = 3.402823466e38
    rays[: n // 16, 3] = 0.0
    rays[n // 16: n // 8, 4] = 0.0
    rays[n // 8: n // 4, 7] = 0.99
    return rays


def _soup(seed, n):
    """random triangles in a 10-unit cube, a tenth of them degenerate (repeated / collinear vertices), some emissive"""
    from cedec_2024_rt_amd.types import TRIANGLE

    rng = np.random.default_rng(seed)
    t = np.zeros(n, TRIANGLE)
    c = rng.random((n, 1, 3), dtype=np.float32) * 10 - 5
    t["v"] = (c + rng.normal(size=(n, 3, 3)).astype(np.float32) * 0.6).astype(np.float32)
    d = rng.random(n) < 0.05
    t["v"][d, 1] = t["v"][d, 0]
    col = (rng.random(n) < 0.05) & ~d
    t["v"][col, 2] = (t["v"][col, 0] + (t["v"][col, 1] - t["v"][col, 0]) * np.float32(2.0)).astype(np.float32)
    t["color"] = 0.5
    t["emissive"][rng.random(n) < 0.1] = 3.0
    return t


def _updates(scenes, tris, seed):
    """(label, first, new triangles of the span, whole new array) for the five kinds of update, in sequence: each starts
    from the array the previous one left"""
    rng = np.random.default_rng(seed)
    n = len(tris)
    v = tris["v"].reshape(-1, 3)
    ext = np.float32(max(float((v.max(0) - v.min(0)).max()), 1.0))
    cur = tris.copy()
    out = []
    mask = rng.random(n) < 0.3
    nxt = scenes.move_triangles(cur, mask, (0.3 * ext, -0.1 * ext, 0.2 * ext))
    out.append(("rigid move of a subset", 0, nxt, nxt))
    cur = nxt
    nxt = cur.copy()
    nxt["v"] = (nxt["v"] + rng.normal(size=nxt["v"].shape).astype(np.float32) * np.float32(0.02) * ext).astype(np.float32)
    out.append(("per-vertex jitter", 0, nxt, nxt))
    cur = nxt
    blk = np.zeros(n, bool)
    blk[n // 3: n // 3 + max(n // 8, 1)] = True
    nxt = scenes.move_triangles(cur, blk, (3.0 * ext, 1.5 * ext, -2.0 * ext))
    out.append(("block thrown far across the scene", 0, nxt, nxt))
    cur = nxt
    a, b = n // 4, max(n // 4 + 1, (3 * n) // 5)
    nxt = cur.copy()
    sub = np.zeros(n, bool)
    sub[a:b] = True
    nxt = scenes.move_triangles(nxt, sub, (-0.2 * ext, 0.25 * ext, 0.1 * ext))
    out.append(("sub-range in the middle", a, nxt[a:b], nxt))
    cur = nxt
    # the second of two in a row: back part of the way, over another span
    c0, c1 = n // 2, n
    nxt = scenes.move_triangles(cur, np.arange(n) >= c0, (0.0, 0.1 * ext, -0.3 * ext))
    out.append(("second update in a row", c0, nxt[c0:c1], nxt))
    return out


def _check_walks(r, tris, rays, oracle, what):
    ref = oracle.Scene(tris, use_bvh=False).trace_closest(rays, force_brute=True)
    for mode in (TraceMode.WIDE,):
        r.trace_mode(mode)
        dev = r.trace_closest(rays)
        assert _eq_bits(dev, ref), f"{what}: mode {mode}: {_diff(dev, ref)} rays differ"
    hit = ref[:, 3].view(np.int32) >= 0
    for mode in (TraceMode.WIDE_ANY, TraceMode.OCCLUDED_WS, TraceMode.OCCLUDED_LANE):  # any-hit walks: occluded <=> a closest hit exists
        r.trace_mode(mode)
        occ = r.trace_closest(rays)[:, 3].view(np.int32) >= 0
        assert (occ == hit).all(), f"{what}: any-hit mode {mode}: {int((occ != hit).sum())} rays differ"
    r.trace_mode(TraceMode.WIDE)
    occ, _, _ = r.trace_occluded_ws(rays)
    assert (occ == hit).all(), f"{what}: work-sharing walk"
    holes = rays.copy()
    holes[::3, 7] = -1.0
    occ_h, _, _ = r.trace_occluded_ws(holes)
    want = hit.copy()
    want[::3] = False
    assert (occ_h == want).all(), f"{what}: work-sharing walk with idle lanes"
    return hit


def _scene_set(golden_scenes, scenes):
    return [("cornellbox1", golden_scenes["cornellbox1"]), ("cornellbox2", golden_scenes["cornellbox2"]),
            ("quad_room", scenes.make_quad_room()), ("soup", _soup(3, 3000)), ("one triangle", _soup(4, 1))]


def test_refitted_walks_equal_brute_force(api, oracle, scenes, golden_scenes):
    """Product library (builder 3, key 7 default and 0): every update kind, every product trace mode == brute force;
    rt_bvh_info unchanged, the light count follows the emissive set."""
    rng = np.random.default_rng(21)
    hits = []
    for name, tris in _scene_set(golden_scenes, scenes):
        for bfs in (None, 0):
            r = api.Renderer(8, 8)
            if bfs is not None:
                r.tuning(Tune.BVH_BFS_RECORDS, bfs)
            r.set_scene(tris)
            info = r.bvh_info()
            for label, first, span, whole in _updates(scenes, tris, 5):
                r.update_scene(span, first)
                v = whole["v"].reshape(-1, 3)
                rays = _random_rays(rng, 6000, v.min(0) - 0.5, v.max(0) + 0.5)
                hits.append(_check_walks(r, whole, rays, oracle, f"{name} bfs={bfs}: {label}").mean())
                assert r.bvh_info() == info, f"{name}: {label}: rt_bvh_info changed"
                assert r.scene_info()["lights"] == len(scenes.light_indices(whole))
            r.close()
    assert np.mean(hits) > 0.05  # rays aimed at the (growing) bounds of the updated scenes still hit something


def test_refit_every_builder_of_the_experiments_library(api, oracle, scenes, golden_scenes):
    """Builders 0 (LBVH, host collapse), 1 (host SAH), 2 (PLOC), 3 (device SAH) and a long breadth-first prefix (key 7):
    the refit reads topology from the records, whatever order a builder allocated them in. The binary tree is not refitted:
    its walk (trace mode 1) refuses after an update."""
    rng = np.random.default_rng(22)
    for name, tris in (("cornellbox1", golden_scenes["cornellbox1"]), ("soup", _soup(6, 4000))):
        for builder, bfs in ((0, None), (1, None), (2, None), (3, None), (0, 100000), (1, 0)):
            r = api.Renderer(8, 8, exp=True)
            r.tuning(Tune.BVH_BUILDER, builder)
            if bfs is not None:
                r.tuning(Tune.BVH_BFS_RECORDS, bfs)
            r.set_scene(tris)
            info = r.bvh_info()
            for label, first, span, whole in _updates(scenes, tris, 9)[2:4]:
                r.update_scene(span, first)
                v = whole["v"].reshape(-1, 3)
                rays = _random_rays(rng, 4000, v.min(0) - 0.5, v.max(0) + 0.5)
                _check_walks(r, whole, rays, oracle, f"{name} builder {builder} bfs {bfs}: {label}")
                assert r.bvh_info() == info
            r.trace_mode(TraceMode.BINARY)
            assert r.L.rt_trace_closest(r.h, rays.ctypes.data, len(rays), np.zeros((len(rays), 4), np.float32).ctypes.data) == RT_ERR_STATE
            r.trace_mode(TraceMode.WIDE)
            r.close()


def _box_and_lights(scenes, tris):
    lights = scenes.light_indices(tris)
    box = np.zeros(len(tris), bool)
    box[QUAD_ROOM_BOX] = True
    assert not np.isin(np.arange(len(tris))[QUAD_ROOM_BOX], lights).any()
    return lights, box


def test_frame_sequence_across_an_update(api, oracle, scenes):
    """Frames 1-2 on scene A; update (lights moved, the box moved); frames 3-5; an update that switches one light off and
    two wall triangles on (n_lights changes); frames 6-7. Accumulation, pixels and temporal history == the oracle driven
    through the same sequence (a new oracle.Scene per scene, the same frame state)."""
    from cedec_2024_rt_amd.types import bench_options

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    A = scenes.make_quad_room()
    lights, box = _box_and_lights(scenes, A)
    lmask = np.zeros(len(A), bool)
    lmask[lights] = True
    B = scenes.move_triangles(scenes.move_triangles(A, lmask, (0.5, -0.25, 0.75)), box, (1.5, 0.0, -0.5))
    Cs = B.copy()
    Cs["emissive"][lights[0]] = 0.0
    Cs["emissive"][40] = (6.0, 5.0, 4.0)
    Cs["emissive"][41] = (2.0, 7.0, 3.0)
    W, H = 96, 54
    rg = oracle.raygen_lookat(EYE, AT, (0, 1, 0), FOVY, W, H)
    for optkw in (dict(accumulate=1), dict(accumulate=1, use_shadowed_target_function=1, spatial_resampling_passes=2)):
        r = api.Renderer(W, H)
        r.set_scene(A)
        r.lookat(EYE, AT)
        r.set_options(bench_options(**optkw))
        r.clear()
        oopt = oracle.bench_options(**optkw)
        st = oracle.new_state(W, H)
        sc, cur = oracle.Scene(A, use_bvh=True), A
        for frame in range(1, 8):
            upd = frame in (3, 6)
            if frame == 3:
                r.update_scene(B[: int(lights.max()) + 1])
                sc, cur = oracle.Scene(B, use_bvh=True), B
            if frame == 6:
                a, b = 40, int(lights[0]) + 1
                r.update_scene(Cs[a:b], a)
                sc, cur = oracle.Scene(Cs, use_bvh=True), Cs
                assert r.scene_info()["lights"] == len(lights) + 1  # one off, two on
                assert len(sc.lights) == len(lights) + 1
            if upd:
                oracle.clear(st["accum"], W, H)
            r.frame(frame, clear_first=upd)
            sc.frame(W, H, frame, rg, EYE, oopt, st)
            acc = r.download(api.RT_BUF_ACCUMULATION)
            assert _eq_bits(acc, st["accum"].reshape(acc.shape)), f"{optkw} frame {frame}: accumulation"
            assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), st["pixels"]), f"{optkw} frame {frame}: pixels"
            hist = r.download(api.RT_BUF_RES_TEMPORAL)
            vis = r.download(api.RT_BUF_VISIBILITY)
            shaded = (vis["index"] >= 0) & ~np.isin(vis["index"], scenes.light_indices(cur))
            tmp = st["temporal"].reshape(hist.shape)
            for f in hist.dtype.names:
                if f != "pad":
                    assert _eq_bits(np.ascontiguousarray(hist[f][shaded]), np.ascontiguousarray(tmp[f][shaded])), f"{optkw} frame {frame}: temporal {f}"
        r.close()


def test_back_to_back_frames_with_updates(api, oracle, scenes):
    """The timed path: 12 rt_frames with the look-ahead at its defaults, updates before frames 4 and 8, nothing synchronised
    by the test in between; the final state == the oracle."""
    from cedec_2024_rt_amd.types import bench_options

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    A = scenes.make_quad_room()
    lights, box = _box_and_lights(scenes, A)
    lmask = np.zeros(len(A), bool)
    lmask[lights] = True
    W, H = 96, 54
    rg = oracle.raygen_lookat(EYE, AT, (0, 1, 0), FOVY, W, H)
    r = api.Renderer(W, H)
    r.set_scene(A)
    r.lookat(EYE, AT)
    r.set_options(bench_options(accumulate=1))
    r.clear()
    oopt = oracle.bench_options(accumulate=1)
    st = oracle.new_state(W, H)
    cur = A
    sc = oracle.Scene(cur, use_bvh=True)
    lo, hi = int(lights.min()), int(lights.max()) + 1
    for frame in range(1, 13):
        upd = frame in (4, 8)
        if upd:
            cur = scenes.move_triangles(cur, lmask, (0.25, 0.0, -0.5) if frame == 4 else (-0.75, 0.25, 0.25))
            r.update_scene(cur[lo:hi], lo)
            sc = oracle.Scene(cur, use_bvh=True)
            oracle.clear(st["accum"], W, H)
        r.frame(frame, clear_first=upd)
        sc.frame(W, H, frame, rg, EYE, oopt, st)
    acc = r.download(api.RT_BUF_ACCUMULATION)
    assert _eq_bits(acc, st["accum"].reshape(acc.shape)), "accumulation after 12 frames"
    assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), st["pixels"])
    r.close()


def test_path_trace_and_ao_after_an_update_equal_a_rebuild(api, scenes, golden_scenes):
    """rt_path_trace 7 / 8 / 9 (three frames from a cleared accumulation) and 6 (AO) on an updated context == a fresh context
    that called rt_scene_set on the new array: pixels, accumulation and ray counts."""
    from cedec_2024_rt_amd.types import default_options

    W, H = 64, 48
    for name, tris, eye, at in (("quad_room", scenes.make_quad_room(), EYE, AT),
                                ("cornellbox1", golden_scenes["cornellbox1"], np.float32([0.0, 2.7, 10.0]), np.float32([0.0, 2.7, -2.8]))):
        upd = _updates(scenes, tris, 13)
        new = upd[3][3]

        def make(t):
            r = api.Renderer(W, H)
            r.set_scene(t)
            r.lookat(eye, at)
            r.set_options(default_options())
            return r

        a = make(tris)
        for label, first, span, whole in upd[:4]:
            a.update_scene(span, first)
        b = make(new)
        for ex in (7, 8, 9):
            for r in (a, b):
                r.clear()
                for frame in (1, 2, 3):
                    r.path_trace(ex, frame)
                r.tone_mapping()
            for buf in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS):
                assert _eq_bits(a.download(buf), b.download(buf)), f"{name} example {ex}: buffer {buf}"
            assert a.path_trace_rays() == b.path_trace_rays(), f"{name} example {ex}: rays"
        pa, pb = a.ambient_occlusion(6), b.ambient_occlusion(6)
        assert np.array_equal(pa, pb), f"{name} AO: {int((pa != pb).any(axis=2).sum())} pixels"
        assert a.path_trace_rays() == b.path_trace_rays()
        a.close()
        b.close()


def test_strip_contexts_updated_between_frames(api, scenes):
    """Three strip contexts on the in-process LOCAL hub (sparse halos), every rank updated between frames == one context
    with the same updates."""
    from cedec_2024_rt_amd.types import bench_options

    A = scenes.make_quad_room()
    lights, box = _box_and_lights(scenes, A)
    lmask = np.zeros(len(A), bool)
    lmask[lights] = True
    W, H = 128, 300
    bounds = api.mg_partition(H, 3)
    opt = bench_options(accumulate=1)

    def make(rows=None, halo=0):
        r = api.Renderer(W, H, rows=rows, halo=halo)
        r.set_scene(A)
        r.lookat(EYE, AT)
        r.set_options(opt)
        return r

    full = make()
    ctxs = [make(rows=b, halo=87) for b in bounds]
    hub = api.MgHub(len(bounds), renderer=ctxs[0])
    mgs = [api.MultiGpu(c, k, bounds, transport=api.RT_MG_TRANSPORT_LOCAL, hub=hub) for k, c in enumerate(ctxs)]
    cur = A
    try:
        for frame in range(1, 7):
            upd = frame in (3, 5)
            if upd:
                cur = scenes.move_triangles(cur, lmask if frame == 3 else box, (0.5, 0.25, -0.5) if frame == 3 else (-1.0, 0.0, 0.5))
                for c in [full] + ctxs:
                    c.update_scene(cur)
            full.frame(frame, upd)
            api.mg_frame_lockstep(mgs, frame, upd)
            ref = full.download(api.RT_BUF_ACCUMULATION).reshape(H, W, 4)
            refpx = full.download(api.RT_BUF_PIXELS).reshape(H, W, 4)
            for c, (a, b) in zip(ctxs, bounds):
                acc = c.download(api.RT_BUF_ACCUMULATION).reshape(c.local_rows, W, 4)[a - c.local_row0: b - c.local_row0]
                assert _eq_bits(acc, ref[a:b]), f"frame {frame}: rows {a}:{b}"
                px = c.download(api.RT_BUF_PIXELS).reshape(c.local_rows, W, 4)[a - c.local_row0: b - c.local_row0]
                assert np.array_equal(px, refpx[a:b]), f"frame {frame}: pixels of rows {a}:{b}"
    finally:
        for m in mgs:
            m.close()
        hub.close()
        for c in [full] + ctxs:
            c.close()


def test_deep_deck_deformed_and_refitted(api, oracle):
    """The deck of test_deep_traversal_stack_spills_past_lds, its cards bent and shifted, refitted: the walks still spill
    past the LDS stack and == brute force."""
    from cedec_2024_rt_amd.types import TRIANGLE

    n = 1100000
    tris = np.zeros(n, TRIANGLE)
    z = (np.arange(n, dtype=np.float32) * np.float32(0.004)).astype(np.float32)
    tris["v"][:, 0] = np.stack([np.zeros(n), np.zeros(n), z], 1)
    tris["v"][:, 1] = np.stack([np.full(n, 2.0), np.zeros(n), z], 1)
    tris["v"][:, 2] = np.stack([np.zeros(n), np.full(n, 2.0), z], 1)
    tris["color"] = 0.5
    r = api.Renderer(8, 8)
    r.set_scene(tris)
    info = r.bvh_info()
    assert 3 * (info["wide_height"] - 1) >= 24 + 6, info
    new = tris.copy()
    bend = (np.float32(0.1) * np.sin(np.arange(n, dtype=np.float32) * np.float32(1e-4))).astype(np.float32)
    new["v"][:, :, 0] = (new["v"][:, :, 0] + bend[:, None]).astype(np.float32)
    new["v"][:, 1, 2] = (new["v"][:, 1, 2] + np.float32(0.001)).astype(np.float32)
    r.update_scene(new)
    assert r.bvh_info() == info
    rng = np.random.default_rng(5)
    m = 192
    rays = np.zeros((m, 8), np.float32)
    rays[:, 0:2] = rng.random((m, 2), dtype=np.float32) * 0.9 + 0.12
    rays[:, 2] = np.where(np.arange(m) % 2 == 0, -1.0, z[-1] + 1.0)
    rays[:, 3:6] = rng.normal(size=(m, 3)).astype(np.float32) * 0.002
    rays[:, 5] = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    rays[:, 7] = np.where(np.arange(m) % 3 == 0, 3.0e38, rng.random(m, dtype=np.float32) * 4000.0)
    rays[::7, 6] = 500.0
    ref = oracle.Scene(new, use_bvh=False).trace_closest(rays, force_brute=True)
    assert (ref[:, 3].view(np.int32) >= 0).mean() > 0.5
    for mode in (TraceMode.WIDE,):
        r.trace_mode(mode)
        dev = r.trace_closest(rays)
        assert _eq_bits(dev, ref), f"mode {mode}: {_diff(dev, ref)} rays differ"
    for mode in (TraceMode.WIDE_ANY, TraceMode.OCCLUDED_LANE):
        r.trace_mode(mode)
        occ = r.trace_closest(rays)[:, 3].view(np.int32) >= 0
        assert (occ == (ref[:, 3].view(np.int32) >= 0)).all(), f"any-hit mode {mode}"
    r.close()


def test_update_error_codes(api, scenes):
    import ctypes as C

    A = scenes.make_quad_room()
    r = api.Renderer(16, 16)
    assert r.L.rt_scene_update(r.h, A.ctypes.data, 0, len(A)) == RT_ERR_STATE  # no scene yet
    r.set_scene(A)
    n = len(A)
    e0 = C.c_uint64()
    r.L.rt_state_epoch(r.h, C.byref(e0))
    assert r.L.rt_scene_update(r.h, A.ctypes.data, 1, n) == RT_ERR_ARG          # past the end
    assert r.L.rt_scene_update(r.h, A.ctypes.data, n, 1) == RT_ERR_ARG
    assert r.L.rt_scene_update(r.h, A.ctypes.data, 0xffffffff, 2) == RT_ERR_ARG  # no wrap-around
    assert r.L.rt_scene_update(r.h, None, 0, 1) == RT_ERR_ARG                   # null pointer with count > 0
    assert r.L.rt_scene_update(r.h, None, 0, 0) == RT_OK                        # count == 0: nothing changes
    assert r.L.rt_scene_update(r.h, None, n, 0) == RT_OK
    e1 = C.c_uint64()
    r.L.rt_state_epoch(r.h, C.byref(e1))
    assert e1.value == e0.value
    with pytest.raises(api.RtError):
        r.update_scene(A[:5], n - 4)
    r.update_scene(A[10:20], 10)
    r.L.rt_state_epoch(r.h, C.byref(e1))
    assert e1.value != e0.value, "an update must change the state epoch"
    r.close()
    empty = api.Renderer(8, 8)
    empty.set_scene(A[:0])
    assert empty.L.rt_scene_update(empty.h, None, 0, 0) == RT_OK
    assert empty.L.rt_scene_update(empty.h, A.ctypes.data, 0, 1) == RT_ERR_ARG
    empty.close()


def test_restir_app_move_lights_equals_the_renderer(tmp_path, api, scenes):
    """restir_app --example 10 --move-lights: the same RGBA8 bytes as the Renderer driven through update_scene with
    scenes.move_triangles (the same float32 add on both sides)."""
    from cedec_2024_rt_amd.types import bench_options

    A = scenes.make_quad_room()
    path = os.path.join(str(tmp_path), "room.tris")
    A.tofile(path)
    out = os.path.join(str(tmp_path), "out.raw")
    W, H, d = 96, 64, (0.25, -0.125, 0.5)
    cmd = [APP, "--example", "10", "--tris", path, "--size", str(W), str(H), "--eye", *map(str, EYE), "--lookat", *map(str, AT),
           "--accumulate", "1", "--frames", "4", "--move-lights", *map(str, d), "--rgba", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("scene update:") == 3, p.stdout
    app_px = np.fromfile(out, np.uint8).reshape(H, W, 4)

    lights = scenes.light_indices(A)
    lmask = np.zeros(len(A), bool)
    lmask[lights] = True
    lo, hi = int(lights.min()), int(lights.max()) + 1
    r = api.Renderer(W, H)
    r.set_scene(A)
    r.lookat(EYE, AT)
    r.set_options(bench_options(accumulate=1))  # restir_app's defaults (common/options.hpp + keys 1, 2), --accumulate 1
    r.clear()
    cur = A
    for frame in range(1, 5):
        upd = frame >= 2
        if upd:
            cur = scenes.move_triangles(cur, lmask, d)
            r.update_scene(cur[lo:hi], lo)
        r.frame(frame, clear_first=upd)
    px = r.download(api.RT_BUF_PIXELS).reshape(H, W, 4)
    r.close()
    assert np.array_equal(app_px, px), f"{int((app_px != px).any(axis=2).sum())} pixels differ"

