"""rt_light_sampling on the device: every form of k_generate_candidate<.., POWER> against tests/light_sampling_ref.py (the restatement
compiled from the kernel's own headers, anchored to the oracle by tests/test_light_sampling_cpu.py), bit for bit. Everything around the
candidates (primary rays, temporal merge, spatial passes, resolve, tone mapping) is the oracle's, as in tests/test_gpu_parity.py; the
unbiased spatial pass is tests/restir_unbiased_ref.py's.

Sizes: 64 x 48 (whole tiles), 37 x 29 (partial tiles in both directions), 8 x 8 (one tile, one wavefront). Scenes: the lamp room
(light_sampling_ref.make_lamp_room: one bright panel, 40 dim tiles) and the soup of tests/test_gpu_restir_unbiased.py."""
import ctypes as C

import numpy as np
import pytest

import light_sampling_ref as ls
import restir_unbiased_ref as ru

pytestmark = pytest.mark.gpu

FOVY = np.float32(0.9)
RT_ERR_ARG, RT_ERR_STATE = 1, 3  # include/restir_rt.h
SIZES = [(64, 48), (37, 29), (8, 8)]


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


def _world(oracle, tris, eye, at):
    return dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True), eye=eye, at=at)


@pytest.fixture(scope="module")
def worlds(oracle):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    return {"lamp": _world(oracle, ls.make_lamp_room(), ls.LAMP_EYE, ls.LAMP_AT), "soup": _world(oracle, _soup(), (1.0, 2.0, 9.0), (0.0, 0.0, 0.0))}


class _Cpu:
    """the frame of 10_restir_di.cpp:257-379 on the CPU: the oracle's kernels, with the candidates from the restatement (and, for
    rt_spatial_unbiased, the spatial pass from its restatement); the shape of tests/test_gpu_restir_unbiased.py's _Cpu"""

    def __init__(self, oracle, world, W, H, opt, mode=ls.POWER, unbiased=False):
        self.o, self.w, self.W, self.H, self.opt, self.mode, self.unbiased = oracle, world, W, H, opt, mode, unbiased
        self.rg = oracle.raygen_lookat(world["eye"], world["at"], (0, 1, 0), FOVY, W, H)
        self.st = oracle.new_state(W, H)
        self.eye = np.asarray(world["eye"], np.float32)
        world["scene"].raycast(W, H, self.rg, self.st["vis"])
        e = world["tris"]["emissive"]
        vis = self.st["vis"]
        self.shaded = (vis["index"] >= 0) & ~(e > 0).any(axis=1)[np.maximum(vis["index"], 0)]

    def candidates(self, frame, opt=None):
        return ls.generate_candidate(self.W, self.H, frame, self.w["tris"], self.st["vis"], self.eye, self.opt if opt is None else opt,
                                     self.mode, self.st["r0"])

    def spatial(self, frame, pas, rin):
        if self.unbiased:
            return ru.spatial(self.W, self.H, frame, pas, self.w["tris"], self.st["vis"], self.eye, self.opt, rin)[0]
        return self.w["scene"].spatial_resampling(self.W, self.H, frame, pas, self.st["vis"], self.eye, self.opt, rin)

    def frame(self, frame):
        sc, st, W, H, opt = self.w["scene"], self.st, self.W, self.H, self.opt
        self.candidates(frame)
        sc.temporal_resampling(W, H, frame, st["vis"], self.eye, opt, st["temporal"], st["r0"])
        self.o.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        src, dst = "r0", "r1"
        for k in range(int(opt["spatial_resampling_passes"][0])):
            if k:
                src, dst = dst, src
            st[dst] = self.spatial(frame, k, st[src])
        sc.resolve(st["accum"], W, H, st["vis"], self.eye, opt, st[dst])
        st["pixels"] = self.o.tone_mapping(st["accum"], W, H)
        return st[dst]


def _renderer(api, world, W, H, opt, mode="power", **kw):
    r = api.Renderer(W, H, **kw)
    r.set_scene(world["tris"])
    r.lookat(world["eye"], world["at"], fovy=FOVY)
    r.set_options(opt)
    if mode is not None:
        assert r.light_sampling(mode) == api.LIGHT_SAMPLING[mode]
    return r


def _check_frame(api, r, out, cpu, last, what):
    W, H = cpu.W, cpu.H
    acc = r.download(api.RT_BUF_ACCUMULATION)
    assert _eq_bits(acc, cpu.st["accum"].reshape(acc.shape)), f"{what}: accumulation"
    assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), cpu.st["pixels"]), f"{what}: pixels"
    bad = _res_diff(r.download(api.RT_BUF_RES_0 + out), last, cpu.shaded)
    assert not bad, f"{what}: records after the frame {bad}"
    bad = _res_diff(r.download(api.RT_BUF_RES_TEMPORAL), cpu.st["temporal"], cpu.shaded)
    assert not bad, f"{what}: temporal history {bad}"


def _same_buffers(api, a, b, out, what):
    for buf in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0 + out):
        assert _eq_bits(a.download(buf), b.download(buf)), f"{what}: buffer {buf}"


def _epoch(r):
    e = C.c_uint64()
    assert r.L.rt_state_epoch(r.h, C.byref(e)) == 0
    return e.value


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["lamp", "soup"])
def test_candidates_equal_the_restatement(api, oracle, worlds, name, W, H):
    """rt_generate_candidate in power mode: every field of every record, for 0 / 1 / 32 candidates with and without visibility reuse"""
    world = worlds[name]
    cpu = _Cpu(oracle, world, W, H, None)
    assert cpu.shaded.any()
    r = _renderer(api, world, W, H, oracle.default_options())
    assert _eq_bits(cpu.rg, r.raygen())
    r.raycast()
    assert _eq_bits(r.download(api.RT_BUF_VISIBILITY), cpu.st["vis"])
    selected = 0
    for ris in (0, 1, 32):
        for vis_reuse in (0, 1):
            opt = oracle.default_options(ris_sample_count=ris, use_visibility_reuse=vis_reuse)
            r.set_options(opt)
            for frame in (1, 2):
                r.generate_candidate(frame, api.RT_RES_0)
                got = r.download(api.RT_BUF_RES_0)
                want = cpu.candidates(frame, opt)
                bad = _res_diff(got, want)
                assert not bad, f"{ris} candidates, visibility reuse {vis_reuse}, frame {frame}: {bad} of {int(cpu.shaded.sum())} shaded pixels"
                selected += int((want["w_sum"][cpu.shaded] > 0).sum())
    assert selected > 0
    # and the mode does something: the reference's selection gives other records
    uniform = _Cpu(oracle, world, W, H, oracle.default_options(), mode=ls.UNIFORM).candidates(2)
    assert _res_diff(uniform, cpu.candidates(2, oracle.default_options()), cpu.shaded)
    r.close()


FRAME_CASES = [
    # world, W, H, option overrides, rt_spatial_unbiased
    ("lamp", 64, 48, dict(), False),
    ("soup", 64, 48, dict(accumulate=1), False),
    ("lamp", 37, 29, dict(accumulate=1), False),
    ("soup", 37, 29, dict(), False),
    ("lamp", 8, 8, dict(), False),
    ("soup", 8, 8, dict(accumulate=1), False),
    ("lamp", 37, 29, dict(use_shadowed_target_function=1), False),
    ("soup", 37, 29, dict(), True),
]


@pytest.mark.parametrize("name,W,H,kw,unbiased", FRAME_CASES)
def test_frames_equal_the_cpu_sequence(api, oracle, worlds, name, W, H, kw, unbiased):
    """three rt_frame frames with the benchmark options: stage 0 as one launch, the temporal merge in the kernel, the look-ahead"""
    world = worlds[name]
    opt = oracle.bench_options(**kw)
    cpu = _Cpu(oracle, world, W, H, opt, unbiased=unbiased)
    assert cpu.shaded.any()
    r = _renderer(api, world, W, H, opt)
    # launches this small are "about one generation of wavefronts": auto would give their primary rays the strips' work-sharing walk and
    # stage 0 two launches (what the knob tests below and the strips run); this is the whole frame's form at the benchmark size
    r.tuning(api.Tune.WS_PRIMARY, 0)
    if unbiased:
        assert r.spatial_unbiased(True) is True
    for frame in (1, 2, 3):
        out = r.frame(frame)
        if frame == 1 and not kw.get("use_shadowed_target_function"):  # later frames reuse the G-buffer and take the look-ahead's candidates
            assert r.stage0_one_launch(), "the frame did not take the product's one-launch stage 0: the case would not cover it"
        _check_frame(api, r, out, cpu, cpu.frame(frame), f"frame {frame}")
    r.close()


def _run_three(api, r):
    outs = []
    for frame in (1, 2, 3):
        outs.append(r.frame(frame))
    return outs


KNOBS = [
    (("tuning", 13, 0),), (("tuning", 13, -1),), (("tuning", 14, 0),), (("tuning", 14, 2),), (("tuning", 17, 0),), (("tuning", 17, 1),),
    (("tuning", 20, 0),), (("tuning", 25, 0),), (("tuning", 25, 1), ("tuning", 14, 0)),
    (("tuning", 0, 1), ("tuning", 1, 2), ("tuning", 2, 3), ("tuning", 3, 5)), (("tuning", 1, 0),), (("tuning", 1, 1),), (("tuning", 1, 3),), (("tuning", 1, 4),),
    # the one-launch stage 0 at this size (rt_tuning 16 = 0, as in the frame cases above), in every frame and as two launches
    (("tuning", 16, 0),), (("tuning", 16, 0), ("gbuffer_reuse", False)), (("tuning", 16, 0), ("tuning", 25, 0)), (("tuning", 16, 0), ("tuning", 14, 0), ("occluder_hints", False)),
    (("gbuffer_reuse", False),), (("occluder_hints", False),), (("gbuffer_reuse", False), ("occluder_hints", False), ("tuning", 13, 0)),
]


@pytest.fixture(scope="module")
def plain_frames(api, oracle, worlds):
    """the lamp room at 37 x 29 in power mode, three frames, no knob touched: computed once, shared and left unchanged"""
    world, W, H = worlds["lamp"], 37, 29
    opt = oracle.bench_options(accumulate=1)
    cpu = _Cpu(oracle, world, W, H, opt)
    r = _renderer(api, world, W, H, opt)
    frames = []
    for frame in (1, 2, 3):
        out = r.frame(frame)
        _check_frame(api, r, out, cpu, cpu.frame(frame), f"plain frame {frame}")
        frames.append((out, {b: r.download(b).copy() for b in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0 + out)}))
    r.close()
    return world, W, H, opt, frames


def _check_against_plain(api, r, plain_frames, what):
    frames = plain_frames[4]
    for frame, (out, bufs) in zip((1, 2, 3), frames):
        assert r.frame(frame) == out
        for b, want in bufs.items():
            assert _eq_bits(r.download(b), want), f"{what}: frame {frame}: buffer {b}"


@pytest.mark.parametrize("knobs", KNOBS)
def test_knobs_leave_the_output_unchanged(api, plain_frames, knobs):
    world, W, H, opt, _ = plain_frames
    r = _renderer(api, world, W, H, opt)
    for k in knobs:
        getattr(r, k[0])(*k[1:])
    _check_against_plain(api, r, plain_frames, str(knobs))
    r.close()


@pytest.mark.parametrize("key", [11, 12])
def test_experiment_forms_leave_the_output_unchanged(api, plain_frames, key):
    """[exp] rt_tuning 11 (deferred visibility rays through a queue) and 12 (software-pipelined RIS loop), and both"""
    world, W, H, opt, _ = plain_frames
    for keys in ((key,), (11, 12)):
        r = _renderer(api, world, W, H, opt, exp=True)
        for k in keys:
            r.tuning(k, 1)
        _check_against_plain(api, r, plain_frames, f"[exp] keys {keys}")
        r.close()


def test_off_equals_a_context_that_never_had_the_mode_and_switching_follows_the_cpu(api, oracle, worlds):
    world, W, H = worlds["lamp"], 64, 48
    opt = oracle.bench_options()
    a, b = _renderer(api, world, W, H, opt, mode=None), _renderer(api, world, W, H, opt, mode=None)
    assert a.light_sampling() == api.RT_LIGHTS_UNIFORM
    e0 = _epoch(a)
    assert a.light_sampling("power") == api.RT_LIGHTS_POWER and _epoch(a) != e0
    e1 = _epoch(a)
    assert a.light_sampling("uniform") == api.RT_LIGHTS_UNIFORM and _epoch(a) != e1
    # off again before anything ran: every byte of every frame equals the context that never called it
    cpu = _Cpu(oracle, world, W, H, opt, mode=ls.UNIFORM)
    for frame in (1,):
        oa, ob_ = a.frame(frame), b.frame(frame)
        assert oa == ob_
        _same_buffers(api, a, b, oa, f"mode off, frame {frame}")
        _check_frame(api, a, oa, cpu, cpu.frame(frame), f"mode off, frame {frame}")
    # switched on between frames 1 and 2 (the look-ahead of frame 1 drew frame 2's candidates uniformly: it must be dropped), no
    # buffer touched: frame 2 continues the CPU sequence with power candidates over the uniform history
    e2 = _epoch(a)
    a.light_sampling(api.RT_LIGHTS_POWER)
    assert _epoch(a) != e2
    cpu.mode = ls.POWER
    out = a.frame(2)
    _check_frame(api, a, out, cpu, cpu.frame(2), "switched on, frame 2")
    b.frame(2)
    assert not _eq_bits(a.download(api.RT_BUF_ACCUMULATION), b.download(api.RT_BUF_ACCUMULATION))
    # and off again: frame 3 continues with uniform candidates
    a.light_sampling(api.RT_LIGHTS_UNIFORM)
    cpu.mode = ls.UNIFORM
    out = a.frame(3)
    _check_frame(api, a, out, cpu, cpu.frame(3), "switched off, frame 3")
    a.close(), b.close()


def _table_of(tris):
    return ls.table(ls.lights(tris)[1])


def _check_table(r, tris, what):
    thr, alias, K = r.light_table()
    t = _table_of(tris)
    assert np.array_equal(thr, t["thr"]) and np.array_equal(alias, t["alias"]) and np.array_equal(K, t["K"]), f"{what}: rt_light_table"
    assert int(K.sum()) == len(K) << 23


@pytest.mark.parametrize("name", ["lamp", "soup"])
def test_light_table_equals_the_host_builder(api, oracle, worlds, name):
    world = worlds[name]
    r = api.Renderer(8, 8)
    assert r.L.rt_light_table(r.h, None, None, None, 0) == RT_ERR_STATE  # no scene yet
    r.set_scene(world["tris"])
    _check_table(r, world["tris"], name)
    L = r.scene_info()["lights"]
    assert r.L.rt_light_table(r.h, None, None, None, L + 1) == RT_ERR_ARG
    r.close()


def test_scene_update_equals_scene_set(api, oracle, worlds):
    """rt_scene_update that scales a light, changes an emission, turns a triangle into a light and a light into a plain triangle, one
    after the other: table and frame equal rt_scene_set on the new array"""
    world, W, H = worlds["lamp"], 37, 29
    opt = oracle.bench_options()
    tris = world["tris"].copy()
    lit = np.flatnonzero((tris["emissive"] > 0).any(axis=1))
    dark = np.flatnonzero(~(tris["emissive"] > 0).any(axis=1))
    r = _renderer(api, world, W, H, opt)
    r.frame(1)
    steps = []
    k = int(lit[7])  # a tile: grown 30 times about its first vertex
    t = tris[k:k + 1].copy()
    t["v"][0] = t["v"][0][0] + (t["v"][0] - t["v"][0][0]) * np.float32(30.0)
    steps.append(("a light scaled", k, t))
    k = int(lit[20])
    t = tris[k:k + 2].copy()
    t["emissive"] = np.float32(900.0)
    steps.append(("an emission changed", k, t))
    k = int(dark[-1])  # a face of the box
    t = tris[k:k + 1].copy()
    t["emissive"] = np.float32(15.0)
    steps.append(("a triangle turned into a light", k, t))
    k = int(lit[0])  # half of the panel
    t = tris[k:k + 1].copy()
    t["emissive"] = np.float32(0.0)
    steps.append(("a light turned into a plain triangle", k, t))
    k = int(dark[3])
    t = tris[k:k + 2].copy()
    t["color"] = np.float32(0.25)
    steps.append(("no light in the span", k, t))
    for frame, (what, first, t) in enumerate(steps, start=2):
        tris[first:first + len(t)] = t
        r.update_scene(t, first)
        _check_table(r, tris, what)
        fresh = _renderer(api, dict(world, tris=tris), W, H, opt)
        _check_table(fresh, tris, what + " (rt_scene_set)")
        # the same temporal history on both (rt_scene_update keeps it, a new context has none), then the same frame: the same
        # candidates from the same table and light records
        fresh.raycast()  # an upload takes the records' shaded bits from the G-buffer
        fresh.upload(api.RT_BUF_RES_TEMPORAL, r.download(api.RT_BUF_RES_TEMPORAL))
        oa, ob_ = r.frame(frame, clear_first=True), fresh.frame(frame, clear_first=True)
        assert oa == ob_
        for buf in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0 + oa):
            assert _eq_bits(r.download(buf), fresh.download(buf)), f"{what}: buffer {buf}"
        cpu = _Cpu(oracle, _world(oracle, tris, world["eye"], world["at"]), W, H, oracle.bench_options(use_temporal_resampling=0))
        fresh.set_options(cpu.opt)
        out = fresh.frame(frame, clear_first=True)
        last = cpu.frame(frame)
        acc = fresh.download(api.RT_BUF_ACCUMULATION)
        assert _eq_bits(acc, cpu.st["accum"].reshape(acc.shape)), f"{what}: accumulation against the CPU"
        assert not _res_diff(fresh.download(api.RT_BUF_RES_0 + out), last, cpu.shaded), f"{what}: records against the CPU"
        fresh.close()
    r.close()


def test_strips_equal_the_whole_frame(api, oracle, worlds):
    """32 x 176 as two strips over the LOCAL transport (the rig of tests/test_mg_native.py), halo 87: the mode is a property of every
    context, and the strips' candidates (the work-sharing kernel without primary rays) equal the whole frame's"""
    world, W, H = worlds["lamp"], 32, 176
    bounds = [(0, 88), (88, 176)]
    opt = oracle.bench_options()

    def make(rows=None, halo=0):
        return _renderer(api, world, W, H, opt, rows=rows, halo=halo)

    full = make()
    ctxs = [make(rows=b, halo=87) for b in bounds]
    hub = api.MgHub(len(bounds), renderer=ctxs[0])
    mgs = [api.MultiGpu(c, k, bounds, transport=api.RT_MG_TRANSPORT_LOCAL, hub=hub) for k, c in enumerate(ctxs)]
    cpu = _Cpu(oracle, world, W, H, opt)
    for frame in (1, 2, 3):
        out = full.frame(frame)
        api.mg_frame_lockstep(mgs, frame, False)
        if frame == 1:
            _check_frame(api, full, out, cpu, cpu.frame(frame), "whole frame 1")
        ref = full.download(api.RT_BUF_ACCUMULATION).reshape(H, W, 4)
        refpx = full.download(api.RT_BUF_PIXELS).reshape(H, W, 4)
        hist = full.download(api.RT_BUF_RES_TEMPORAL).reshape(H, W)
        for c, (a, b) in zip(ctxs, bounds):
            rows = slice(a - c.local_row0, b - c.local_row0)
            acc = c.download(api.RT_BUF_ACCUMULATION).reshape(c.local_rows, W, 4)[rows]
            assert _eq_bits(acc, ref[a:b]), f"frame {frame}: rows {a}:{b}: {int((acc != ref[a:b]).any(axis=2).sum())} pixels differ"
            assert np.array_equal(c.download(api.RT_BUF_PIXELS).reshape(c.local_rows, W, 4)[rows], refpx[a:b]), f"frame {frame}: pixels of rows {a}:{b}"
            assert _eq_bits(c.download(api.RT_BUF_RES_TEMPORAL).reshape(c.local_rows, W)[rows], hist[a:b]), f"frame {frame}: history of rows {a}:{b}"
    for m in mgs:
        m.close()
    hub.close()
    for c in [full] + ctxs:
        c.close()


def test_error_codes(api, oracle, worlds):
    world, W, H = worlds["lamp"], 37, 29
    r = api.Renderer(W, H)
    for mode in (2, -1, 7):
        assert r.L.rt_light_sampling(r.h, mode) == RT_ERR_ARG
    with pytest.raises(api.RtError):
        r.light_sampling("brightest")
    assert r.light_sampling() == api.RT_LIGHTS_UNIFORM  # a refused mode changes nothing
    assert r.L.rt_light_sampling_get(r.h, None) == RT_ERR_ARG
    assert r.light_sampling("power") == api.RT_LIGHTS_POWER  # before the scene
    # a scene whose only light has no area: the frame runs as before in uniform mode, and power mode has nothing to select
    tris = world["tris"].copy()
    tris["emissive"] = 0.0
    k = len(tris) - 1
    tris["v"][k][2] = tris["v"][k][1]
    tris["emissive"][k] = 5.0
    r.set_scene(tris)
    r.lookat(world["eye"], world["at"], fovy=FOVY)
    opt = oracle.bench_options()
    r.set_options(opt)
    assert r.scene_info()["lights"] == 1 and not r.light_table()[2].any()
    out = C.c_int(-1)
    assert r.L.rt_frame(r.h, 1, 0, C.byref(out)) == RT_ERR_STATE
    r.raycast()
    assert r.L.rt_generate_candidate(r.h, 1, api.RT_RES_0) == RT_ERR_STATE
    r.light_sampling("uniform")
    plain = _renderer(api, dict(world, tris=tris), W, H, opt, mode=None)
    for frame in (1, 2):
        oa, ob_ = r.frame(frame), plain.frame(frame)
        assert oa == ob_
        _same_buffers(api, r, plain, oa, f"uniform mode, frame {frame}")
    # without candidates there is nothing to select either way
    r.light_sampling("power")
    r.set_options(oracle.bench_options(ris_sample_count=0))
    r.frame(3)
    r.close(), plain.close()
