"""rt_light_grid on the device: the tables the library builds and uploads, and every form of k_generate_candidate<.., GRID>, against
tests/light_grid_ref.py (the restatement compiled from the kernel's own headers, anchored by tests/test_light_grid_cpu.py), bit for
bit. Everything around the candidates (primary rays, temporal merge, spatial passes, resolve, tone mapping) is the oracle's, as in
tests/test_gpu_light_sampling.py; the reprojected and the followed temporal merge are their restatements'.

Sizes: 64 x 48 (whole tiles), 37 x 29 (partial tiles in both directions), 8 x 8 (one tile, one wavefront). Scenes: the lamp field
(light_grid_ref.make_lamp_field: 512 equal lamps), the lamp room (one bright panel, 40 dim tiles) and the soup of
tests/test_gpu_restir_unbiased.py. (cells, clusters): (1, 1), (2, 3), (4, 256) (more clusters than the room's and the soup's lights:
one light per run), (16, 64) and (32, 7)."""
import ctypes as C

import numpy as np
import pytest

import light_grid_ref as lg
import light_sampling_ref as ls
import temporal_motion_ref as tm
import temporal_reproject_ref as tr
from test_temporal_motion_cpu import BOX_HI, BOX_LO, Worlds, move
from test_temporal_reproject_cpu import _orbit

pytestmark = pytest.mark.gpu

FOVY = np.float32(0.9)
RT_ERR_ARG, RT_ERR_STATE, RT_ERR_UNSUPPORTED = 1, 3, 5  # include/restir_rt.h
SIZES = [(64, 48), (37, 29), (8, 8)]
GRIDS = [(1, 1), (2, 3), (4, 256), (16, 64), (32, 7)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _eq_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _res_diff(a, b, mask=None):
    """fields of two reservoir arrays (padding excluded) that differ on `mask`, with the number of records"""
    mask = np.ones(len(a), bool) if mask is None else mask
    bad = []
    for f in a.dtype.names:
        if f == "pad":
            continue
        x, y = np.ascontiguousarray(a[f][mask]), np.ascontiguousarray(b[f][mask])
        if not _eq_bits(x, y):
            bad.append((f, int((_bits(x).reshape(len(x), -1) != _bits(y).reshape(len(y), -1)).any(axis=1).sum())))
    return bad


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


def _soup():
    """the soup of tests/test_gpu_restir_unbiased.py"""
    from cedec_2024_rt_amd.types import TRIANGLE

    rng = np.random.default_rng(15)
    n = 150
    t = np.zeros(n, TRIANGLE)
    c = rng.normal(size=(n, 1, 3)).astype(np.float32) * np.float32(3.0)
    size = np.float32(10.0) ** rng.uniform(-1.0, 0.6, size=(n, 1, 1)).astype(np.float32)
    t["v"] = (c + rng.normal(size=(n, 3, 3)).astype(np.float32) * size).astype(np.float32)
    t["color"] = rng.random((n, 3), dtype=np.float32)
    lights = rng.random(n) < 0.3
    lights[0] = True
    t["emissive"][lights] = (rng.random((int(lights.sum()), 3), dtype=np.float32) * np.float32(20.0)).astype(np.float32)
    return t


class _View:
    def __init__(self, oracle, world, W, H, eye, at):
        self.W, self.H, self.eye, self.at = W, H, np.asarray(eye, np.float32), at
        self.rg = oracle.raygen_lookat(eye, at, (0, 1, 0), FOVY, W, H)
        self.vis = world["scene"].raycast(W, H, self.rg)
        lit = (world["tris"]["emissive"] > 0).any(axis=1)
        self.shaded = (self.vis["index"] >= 0) & ~lit[np.maximum(self.vis["index"], 0)]


def _world(oracle, tris, eye, at):
    return dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True), eye=eye, at=at)


@pytest.fixture(scope="module")
def worlds(oracle):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    return {"field": _world(oracle, lg.make_lamp_field(), lg.FIELD_EYE, lg.FIELD_AT), "lamp": _world(oracle, ls.make_lamp_room(), ls.LAMP_EYE, ls.LAMP_AT),
            "soup": _world(oracle, _soup(), (1.0, 2.0, 9.0), (0.0, 0.0, 0.0))}


_grids = {}


def _grid(tris, cells, clusters):
    """the restatement's tables, built once per scene and setting"""
    key = (tris.tobytes(), cells, clusters)
    if key not in _grids:
        _grids[key] = lg.Grid(tris, cells, clusters)
    return _grids[key]


class _Cpu:
    """the frame of 10_restir_di.cpp:257-379 on the CPU with one scene and one camera per frame: the oracle's kernels, the candidates from
    the restatement (grid = (cells, clusters), "power", or None for the reference's), and the temporal merge of the frame's kind: the
    reference's own-pixel merge, the reprojection's restatement or the followed one's"""

    def __init__(self, oracle, W, H, opt, grid=(16, 64)):
        self.o, self.W, self.H, self.opt, self.grid = oracle, W, H, opt, grid
        self.st = oracle.new_state(W, H)
        self.prev = None

    def candidates(self, frame, world, view, opt=None):
        opt = self.opt if opt is None else opt
        if self.grid is None or self.grid == "power":
            return lg.generate_candidate(self.W, self.H, frame, world["tris"], view.vis, view.eye, opt, lg.UNIFORM if self.grid is None else lg.POWER, self.st["r0"])
        return lg.generate_candidate(self.W, self.H, frame, world["tris"], view.vis, view.eye, opt, lg.GRID, self.st["r0"], grid=_grid(world["tris"], *self.grid))

    def frame(self, frame, world, view, temporal="same"):
        sc, st, W, H, opt = world["scene"], self.st, self.W, self.H, self.opt
        st["vis"] = view.vis
        self.candidates(frame, world, view)
        if self.prev is None or temporal == "same":
            sc.temporal_resampling(W, H, frame, view.vis, view.eye, opt, st["temporal"], st["r0"])
        elif temporal == "motion":
            pw, pv = self.prev
            tm.temporal(W, H, frame, world["tris"], pw["tris"], view.vis, pv.vis, view.eye, pv.eye, pv.rg, view.rg, BOX_LO, BOX_HI, opt, st["temporal"], st["r0"])
        else:
            pw, pv = self.prev
            tr.temporal(W, H, frame, world["tris"], view.vis, pv.vis, view.eye, pv.rg, view.rg, opt, st["temporal"], st["r0"])
        self.o.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        self.prev = (world, view)
        src, dst = "r0", "r1"
        for k in range(int(opt["spatial_resampling_passes"][0])):
            if k:
                src, dst = dst, src
            st[dst] = sc.spatial_resampling(W, H, frame, k, view.vis, view.eye, opt, st[src])
        sc.resolve(st["accum"], W, H, view.vis, view.eye, opt, st[dst])
        st["pixels"] = self.o.tone_mapping(st["accum"], W, H)
        return st[dst]


def _renderer(api, world, W, H, opt, grid=(16, 64), **kw):
    r = api.Renderer(W, H, **kw)
    r.set_scene(world["tris"])
    if "eye" in world:
        r.lookat(world["eye"], world["at"], fovy=FOVY)
    r.set_options(opt)
    if grid is not None:
        got = r.light_grid(*grid)
        assert got == (grid[0], grid[1], min(grid[1], r.scene_info()["lights"]))
    return r


def _check_frame(api, r, out, cpu, last, view, what):
    W, H = cpu.W, cpu.H
    acc = r.download(api.RT_BUF_ACCUMULATION)
    assert _eq_bits(acc, cpu.st["accum"].reshape(acc.shape)), f"{what}: accumulation"
    assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), cpu.st["pixels"]), f"{what}: pixels"
    bad = _res_diff(r.download(api.RT_BUF_RES_0 + out), last, view.shaded)
    assert not bad, f"{what}: records after the frame {bad}"
    bad = _res_diff(r.download(api.RT_BUF_RES_TEMPORAL), cpu.st["temporal"], view.shaded)
    assert not bad, f"{what}: temporal history {bad}"


def _same_buffers(api, a, b, out, what):
    for buf in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0 + out):
        assert _eq_bits(a.download(buf), b.download(buf)), f"{what}: buffer {buf}"


def _epoch(r):
    e = C.c_uint64()
    assert r.L.rt_state_epoch(r.h, C.byref(e)) == 0
    return e.value


# ------------------------------------------------------------------------------------------------------------------ tables
def _check_table(r, tris, cells, clusters, what):
    t, g = r.light_grid_table(), _grid(tris, cells, clusters)
    assert (t["cells"], t["clusters"]) == (g.N, g.B), what
    for k, want in (("lo", g.lo), ("hi", g.hi), ("inv", g.inv), ("cluster_of", g.cluster_of), ("perm", g.perm), ("run_start", g.run_start),
                    ("run_thr", g.run_thr), ("run_alias", g.run_alias), ("run_K", g.run_K), ("cell_thr", g.cell_thr), ("cell_alias", g.cell_alias),
                    ("cell_K", g.cell_K), ("cell_prob", g.cell_prob)):
        assert t[k].shape == want.shape and _eq_bits(t[k], want), f"{what}: rt_light_grid_table {k}"
    assert (t["cell_K"].reshape(-1, g.B).astype(object).sum(axis=1) == g.B << 23).all()


@pytest.mark.parametrize("name", ["field", "lamp", "soup"])
def test_tables_equal_the_restatement(api, worlds, name):
    """after rt_scene_set with the grid on, after toggling with a scene present, and with other settings"""
    world = worlds[name]
    r = api.Renderer(8, 8)
    assert r.L.rt_light_grid_table(r.h, *[None] * 11, 0, 0) == RT_ERR_STATE  # no scene yet
    assert r.light_grid(16, 64) == (16, 64, 0)  # before the scene: nothing to build
    r.set_scene(world["tris"])
    _check_table(r, world["tris"], 16, 64, f"{name}: set before the scene")
    L = r.scene_info()["lights"]
    assert r.L.rt_light_grid_table(r.h, *[None] * 11, L + 1, 16 ** 3 * min(64, L)) == RT_ERR_ARG
    assert r.L.rt_light_grid_table(r.h, *[None] * 11, L, 5) == RT_ERR_ARG
    assert r.light_grid(0) == (0, 0, 0)
    assert r.L.rt_light_grid_table(r.h, *[None] * 11, L, 0) == RT_ERR_STATE  # off: no tables
    for cells, clusters in GRIDS:  # toggled with the scene present
        assert r.light_grid(cells, clusters) == (cells, clusters, min(clusters, L))
        _check_table(r, world["tris"], cells, clusters, f"{name}: toggled to {(cells, clusters)}")
    r.close()


def test_scene_update_equals_scene_set(api, oracle, worlds):
    """rt_scene_update that moves lamps (clusters and bounds change), changes an emission, turns a lamp off, and touches no light: the
    tables equal a fresh rt_scene_set of the new array, and so does a frame"""
    world, W, H = worlds["field"], 37, 29
    opt = oracle.bench_options()
    tris = world["tris"].copy()
    lit = np.flatnonzero((tris["emissive"] > 0).any(axis=1))
    r = _renderer(api, world, W, H, opt)
    r.frame(1)
    steps = []
    k = int(lit[0])
    t = tris[k:k + 64].copy()  # 32 lamps: up and past the edge of the floor, so that the bounds grow
    t["v"] += np.array([-3.0, 1.5, 0.5], np.float32)
    steps.append(("lamps moved", k, t))
    k = int(lit[100])
    t = tris[k:k + 2].copy()
    t["emissive"] = np.float32(900.0)
    steps.append(("an emission changed", k, t))
    k = int(lit[300])
    t = tris[k:k + 2].copy()
    t["emissive"] = np.float32(0.0)
    steps.append(("a lamp turned off", k, t))
    t = tris[0:2].copy()
    t["color"] = np.float32(0.25)
    steps.append(("no light in the span", 0, t))
    for frame, (what, first, t) in enumerate(steps, start=2):
        tris[first:first + len(t)] = t
        r.update_scene(t, first)
        _check_table(r, tris, 16, 64, what)
        fresh = _renderer(api, dict(world, tris=tris), W, H, opt)
        _check_table(fresh, tris, 16, 64, what + " (rt_scene_set)")
        fresh.raycast()  # an upload takes the records' shaded bits from the G-buffer
        fresh.upload(api.RT_BUF_RES_TEMPORAL, r.download(api.RT_BUF_RES_TEMPORAL))
        oa, ob_ = r.frame(frame, clear_first=True), fresh.frame(frame, clear_first=True)
        assert oa == ob_
        _same_buffers(api, r, fresh, oa, what)
        fresh.close()
    r.close()


# ------------------------------------------------------------------------------------------------------------ kernel forms
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["field", "lamp", "soup"])
def test_candidates_equal_the_restatement(api, oracle, worlds, name, W, H):
    """rt_generate_candidate with the grid on: every field of every record, for every setting of GRIDS, both target functions, 1 and
    32 candidates"""
    world = worlds[name]
    view = _View(oracle, world, W, H, world["eye"], world["at"])
    assert view.shaded.any()
    r = _renderer(api, world, W, H, oracle.default_options(), grid=None)
    assert _eq_bits(view.rg, r.raygen())
    r.raycast()
    assert _eq_bits(r.download(api.RT_BUF_VISIBILITY), view.vis)
    L = r.scene_info()["lights"]
    selected = 0
    for cells, clusters in GRIDS:
        assert r.light_grid(cells, clusters) == (cells, clusters, min(clusters, L))
        cpu = _Cpu(oracle, W, H, None, grid=(cells, clusters))
        for sh in (0, 1):
            for ris in (1, 32):
                opt = oracle.default_options(ris_sample_count=ris, use_shadowed_target_function=sh)
                r.set_options(opt)
                frame = 1 + ris % 3
                r.generate_candidate(frame, api.RT_RES_0)
                got = r.download(api.RT_BUF_RES_0)
                want = cpu.candidates(frame, world, view, opt)
                bad = _res_diff(got, want)
                assert not bad, f"grid {(cells, clusters)}, shadowed {sh}, {ris} candidates: {bad} of {int(view.shaded.sum())} shaded pixels"
                selected += int((want["w_sum"][view.shaded] > 0).sum())
    assert selected > 0
    # and the grid does something: the reference's selection gives other records
    opt = oracle.default_options()
    uniform = _Cpu(oracle, W, H, opt, grid=None).candidates(2, world, view).copy()
    assert _res_diff(uniform, _Cpu(oracle, W, H, opt, grid=(16, 64)).candidates(2, world, view), view.shaded)
    r.close()


FRAME_CASES = [
    # world, W, H, option overrides, (cells, clusters)
    ("field", 64, 48, dict(), (16, 64)),
    ("soup", 64, 48, dict(accumulate=1), (4, 256)),
    ("lamp", 37, 29, dict(accumulate=1), (32, 7)),
    ("field", 37, 29, dict(), (2, 3)),
    ("lamp", 8, 8, dict(), (16, 64)),
    ("field", 8, 8, dict(accumulate=1), (1, 1)),
    ("field", 37, 29, dict(use_shadowed_target_function=1), (16, 64)),
    ("soup", 37, 29, dict(use_shadowed_target_function=1), (2, 3)),
]


@pytest.mark.parametrize("name,W,H,kw,grid", FRAME_CASES)
def test_frames_equal_the_cpu_sequence(api, oracle, worlds, name, W, H, kw, grid):
    """four rt_frame frames with the benchmark options (temporal and spatial reuse on): stage 0 as one launch, the temporal merge in
    the kernel, the look-ahead"""
    world = worlds[name]
    opt = oracle.bench_options(**kw)
    view = _View(oracle, world, W, H, world["eye"], world["at"])
    assert view.shaded.any()
    cpu = _Cpu(oracle, W, H, opt, grid=grid)
    r = _renderer(api, world, W, H, opt, grid=grid)
    r.tuning(api.Tune.WS_PRIMARY, 0)  # the whole frame's form at the benchmark size, as tests/test_gpu_light_sampling.py
    for frame in (1, 2, 3, 4):
        out = r.frame(frame)
        if frame == 1 and not kw.get("use_shadowed_target_function"):
            assert r.stage0_one_launch(), "the frame did not take the product's one-launch stage 0: the case would not cover it"
        _check_frame(api, r, out, cpu, cpu.frame(frame, world, view), view, f"frame {frame}")
    r.close()


KNOBS = [
    (("tuning", 13, 0),), (("tuning", 13, -1),), (("tuning", 14, 0),), (("tuning", 14, 2),), (("tuning", 17, 0),), (("tuning", 17, 1),),
    (("tuning", 20, 0),), (("tuning", 25, 0),), (("tuning", 25, 1), ("tuning", 14, 0)),
    (("tuning", 0, 1), ("tuning", 1, 2), ("tuning", 2, 3), ("tuning", 3, 5)), (("tuning", 1, 0),), (("tuning", 1, 4),),
    (("tuning", 16, 0),), (("tuning", 16, 0), ("gbuffer_reuse", False)), (("tuning", 16, 0), ("tuning", 25, 0)), (("tuning", 16, 0), ("tuning", 14, 0), ("occluder_hints", False)),
    (("gbuffer_reuse", False),), (("occluder_hints", False),), (("gbuffer_reuse", False), ("occluder_hints", False), ("tuning", 13, 0)),
]


@pytest.fixture(scope="module")
def plain_frames(api, oracle, worlds):
    """the lamp field at 37 x 29 with the grid at (16, 64), three frames, no knob touched: checked against the CPU, computed once,
    shared and left unchanged"""
    world, W, H = worlds["field"], 37, 29
    opt = oracle.bench_options(accumulate=1)
    view = _View(oracle, world, W, H, world["eye"], world["at"])
    cpu = _Cpu(oracle, W, H, opt)
    r = _renderer(api, world, W, H, opt)
    frames = []
    for frame in (1, 2, 3):
        out = r.frame(frame)
        _check_frame(api, r, out, cpu, cpu.frame(frame, world, view), view, f"plain frame {frame}")
        frames.append((out, {b: r.download(b).copy() for b in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0 + out)}))
    r.close()
    return world, W, H, opt, frames


@pytest.mark.parametrize("knobs", KNOBS)
def test_knobs_leave_the_output_unchanged(api, plain_frames, knobs):
    """the rt_tuning keys that apply to stage 0 (the forms of the candidates' kernel: with and without the work-sharing walk, with and
    without primary rays, with and without the look-ahead) and the toggles around it"""
    world, W, H, opt, frames = plain_frames
    r = _renderer(api, world, W, H, opt)
    for k in knobs:
        getattr(r, k[0])(*k[1:])
    for frame, (out, bufs) in zip((1, 2, 3), frames):
        assert r.frame(frame) == out
        for b, want in bufs.items():
            assert _eq_bits(r.download(b), want), f"{knobs}: frame {frame}: buffer {b}"
    r.close()


def test_experiment_forms_refuse_the_grid(api, plain_frames):
    """[exp] rt_tuning 11 (deferred visibility rays through a queue) and 12 (software-pipelined RIS loop) are not built for the grid"""
    world, W, H, opt, _ = plain_frames
    for key in (11, 12):
        r = _renderer(api, world, W, H, opt, exp=True)
        r.tuning(key, 1)
        out = C.c_int(-1)
        assert r.L.rt_frame(r.h, 1, 0, C.byref(out)) == RT_ERR_UNSUPPORTED
        r.tuning(key, 0)
        r.frame(1)
        r.close()


# ------------------------------------------------------------------------------------------- beside the temporal toggles
@pytest.mark.parametrize("W,H,kw", [(37, 29, dict()), (64, 48, dict(use_shadowed_target_function=1))])
def test_frames_under_a_camera_step_equal_the_cpu_sequence(api, oracle, W, H, kw):
    """rt_temporal_reprojection: the camera orbits between the frames, every frame from the second on gathers its history by
    reprojection in the candidates' kernel (the REPROJECT forms with the grid)"""
    ws = Worlds(oracle)
    world = ws.of(ws.base)
    opt = oracle.bench_options(**kw)
    cpu = _Cpu(oracle, W, H, opt, grid=(16, 64))
    r = api.Renderer(W, H)
    r.set_scene(world["tris"])
    r.set_options(opt)
    assert r.temporal_reprojection(True) is True
    assert r.light_grid(16, 64) == (16, 64, 64)
    r.tuning(api.Tune.WS_PRIMARY, 0)
    r.walk_stats_enable(True)
    for k in range(4):
        view = ws.view(world, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, 0.1 * k))
        r.lookat(view.eye, view.at, fovy=FOVY)
        assert _eq_bits(r.raygen(), view.rg)
        out = r.frame(1 + k)
        _check_frame(api, r, out, cpu, cpu.frame(1 + k, world, view, temporal="reproject"), view, f"frame {1 + k}")
    assert r.temporal_reprojection_stats()["merged"] > 0, "no launch reprojected: the case covers nothing"
    r.close()


@pytest.mark.parametrize("W,H,one_launch,kw", [(37, 29, 1, dict()), (37, 29, 0, dict()), (64, 48, 1, dict(use_shadowed_target_function=1))])
def test_frames_with_a_moving_box_equal_the_cpu_sequence(api, oracle, W, H, one_launch, kw):
    """rt_temporal_motion: the lamp room's box moves by rt_scene_update between the frames (no light in the span, the bounds stay:
    the tables stay), every frame from the second on follows it in the candidates' kernel (the MOTION forms with the grid)"""
    ws = Worlds(oracle)
    opt = oracle.bench_options(**kw)
    cpu = _Cpu(oracle, W, H, opt, grid=(16, 64))
    t = move(ws.base, (0.0, 0.0, -2.0))
    r = api.Renderer(W, H)
    r.set_scene(t)
    r.set_options(opt)
    assert r.temporal_reprojection(True) is True and r.temporal_motion(True) is True
    assert r.light_grid(16, 64) == (16, 64, 64)
    r.tuning(api.Tune.WS_PRIMARY, 0)
    r.tuning(25, one_launch)
    r.walk_stats_enable(True)
    for k in range(4):
        if k:
            t = move(t, (0.0, 0.0, 1.0))
            r.update_scene(t[BOX_LO:BOX_HI], first=BOX_LO)
        world = ws.of(t)
        view = ws.view(world, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, 0.1 * k))
        r.lookat(view.eye, view.at, fovy=FOVY)
        out = r.frame(1 + k)
        _check_frame(api, r, out, cpu, cpu.frame(1 + k, world, view, temporal="motion"), view, f"frame {1 + k}")
    assert r.temporal_motion_stats()["valid"] > 0, "no launch followed the box: the case covers nothing"
    _check_table(r, t, 16, 64, "after the box moved")
    r.close()


# -------------------------------------------------------------------------------------------------------------- host rules
def test_on_then_off_equals_a_context_that_never_had_the_grid(api, oracle, worlds):
    world, W, H = worlds["lamp"], 64, 48
    opt = oracle.bench_options()
    view = _View(oracle, world, W, H, world["eye"], world["at"])
    a, b = _renderer(api, world, W, H, opt, grid=None), _renderer(api, world, W, H, opt, grid=None)
    assert a.light_grid() == (0, 0, 0)
    assert a.light_sampling("power") == api.RT_LIGHTS_POWER and b.light_sampling("power") == api.RT_LIGHTS_POWER
    e0 = _epoch(a)
    assert a.light_grid(16, 64) == (16, 64, 64) and _epoch(a) != e0
    assert a.light_sampling() == api.RT_LIGHTS_POWER, "rt_light_sampling's mode is kept while the grid is on"
    e1 = _epoch(a)
    assert a.light_grid(0) == (0, 0, 0) and _epoch(a) != e1
    # off again before anything ran: every byte of the frame equals the context that never called it, in the mode that was kept
    cpu = _Cpu(oracle, W, H, opt, grid="power")
    oa, ob_ = a.frame(1), b.frame(1)
    assert oa == ob_
    _same_buffers(api, a, b, oa, "grid off, frame 1")
    _check_frame(api, a, oa, cpu, cpu.frame(1, world, view), view, "grid off, frame 1")
    # switched on between frames 1 and 2 (the look-ahead of frame 1 drew frame 2's candidates from the alias table: it must be
    # dropped), no buffer touched: frame 2 continues the CPU sequence with the grid's candidates over the other history
    e2 = _epoch(a)
    a.light_grid(4, 256)
    assert _epoch(a) != e2
    cpu.grid = (4, 256)
    out = a.frame(2)
    _check_frame(api, a, out, cpu, cpu.frame(2, world, view), view, "switched on, frame 2")
    b.frame(2)
    assert not _eq_bits(a.download(api.RT_BUF_ACCUMULATION), b.download(api.RT_BUF_ACCUMULATION))
    # other settings without going through off, then off: power mode comes back
    a.light_grid(2, 3)
    cpu.grid = (2, 3)
    out = a.frame(3)
    _check_frame(api, a, out, cpu, cpu.frame(3, world, view), view, "other settings, frame 3")
    a.light_grid(0, 99)
    cpu.grid = "power"
    out = a.frame(4)
    _check_frame(api, a, out, cpu, cpu.frame(4, world, view), view, "switched off, frame 4")
    a.close(), b.close()


def test_error_codes(api, oracle, worlds):
    world, W, H = worlds["lamp"], 37, 29
    r = api.Renderer(W, H)
    assert r.light_grid(8, 16) == (8, 16, 0)
    e = _epoch(r)
    for cells, clusters in ((33, 64), (-1, 64), (16, 0), (16, 257), (4, 512), (16, -3)):
        assert r.L.rt_light_grid(r.h, cells, clusters) == RT_ERR_ARG
    assert r.light_grid() == (8, 16, 0) and _epoch(r) == e  # a refused call changes nothing
    assert r.L.rt_light_sampling(r.h, 2) == RT_ERR_ARG  # the grid is no third mode of rt_light_sampling
    assert r.light_grid(32, 256) == (32, 256, 0) and r.light_grid(1, 1) == (1, 1, 0)
    assert r.light_grid(None, 7) == (api.LIGHT_GRID_DEFAULT[0], 7, 0) and r.light_grid(5) == (5, api.LIGHT_GRID_DEFAULT[1], 0)
    # a scene whose only light has no area: the frame runs as before with the grid off, and the grid has nothing to select
    tris = world["tris"].copy()
    tris["emissive"] = 0.0
    k = len(tris) - 1
    tris["v"][k][2] = tris["v"][k][1]
    tris["emissive"][k] = 5.0
    r.set_scene(tris)
    r.lookat(world["eye"], world["at"], fovy=FOVY)
    opt = oracle.bench_options()
    r.set_options(opt)
    assert r.scene_info()["lights"] == 1 and r.light_grid() == (5, api.LIGHT_GRID_DEFAULT[1], 1) and not r.light_grid_table()["cell_K"].any()
    out = C.c_int(-1)
    assert r.L.rt_frame(r.h, 1, 0, C.byref(out)) == RT_ERR_STATE
    r.raycast()
    assert r.L.rt_generate_candidate(r.h, 1, api.RT_RES_0) == RT_ERR_STATE
    r.light_grid(0)
    plain = _renderer(api, dict(world, tris=tris), W, H, opt, grid=None)
    for frame in (1, 2):
        oa, ob_ = r.frame(frame), plain.frame(frame)
        assert oa == ob_
        _same_buffers(api, r, plain, oa, f"grid off, frame {frame}")
    # without candidates there is nothing to select either way
    r.light_grid(4, 4)
    r.set_options(oracle.bench_options(ris_sample_count=0))
    r.frame(3)
    r.close(), plain.close()
    # strip contexts: a follow-up
    s = api.Renderer(32, 64, rows=(0, 32), halo=8)
    assert s.L.rt_light_grid(s.h, 16, 64) == RT_ERR_UNSUPPORTED and s.light_grid() == (0, 0, 0)
    assert s.L.rt_light_grid(s.h, 0, 0) == 0
    s.close()


def test_restir_app_light_grid_equals_the_renderer(tmp_path, api, worlds):
    """restir_app --light-grid 16 64: the same RGBA8 bytes as the Renderer with the grid on; the option's refusals"""
    import os
    import subprocess

    from cedec_2024_rt_amd.types import bench_options

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    world = worlds["field"]
    path, out = os.path.join(str(tmp_path), "field.tris"), os.path.join(str(tmp_path), "out.raw")
    world["tris"].tofile(path)
    W, H = 96, 64
    head = [os.path.join(root, "app", "restir_app"), "--example", "10", "--tris", path, "--size", str(W), str(H), "--eye", *map(str, lg.FIELD_EYE),
            "--lookat", *map(str, lg.FIELD_AT), "--frames", "3"]
    p = subprocess.run(head + ["--light-grid", "16", "64", "--rgba", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    app_px = np.fromfile(out, np.uint8).reshape(H, W, 4)
    pixels = {}
    for grid in ((16, 64), None):
        r = api.Renderer(W, H)
        r.set_scene(world["tris"])
        r.lookat(lg.FIELD_EYE, lg.FIELD_AT)
        r.set_options(bench_options())
        if grid:
            r.light_grid(*grid)
        r.clear()
        for frame in (1, 2, 3):
            r.frame(frame)
        pixels[grid] = r.download(api.RT_BUF_PIXELS).reshape(H, W, 4).copy()
        r.close()
    assert np.array_equal(pixels[(16, 64)], app_px)
    assert not np.array_equal(pixels[None], app_px), "the option is what makes these bytes"
    for extra in (["--light-grid", "33", "64"], ["--light-grid", "16", "0"], ["--light-grid", "16"], ["--light-grid", "16", "64", "--example", "7"],
                  ["--light-grid", "16", "64", "--ranks", "2"]):
        p = subprocess.run(head + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (extra, p.stdout + p.stderr)
