"""rt_temporal_reprojection on the device: k_temporal<.., REPROJECT> and the fused k_generate_candidate<.., REPROJECT> forms against
tests/temporal_reproject_ref.py (the restatement compiled from the kernels' own headers, anchored to the oracle by
tests/test_temporal_reproject_cpu.py), bit for bit. Everything around the temporal merge (primary rays, candidates, spatial passes,
resolve, tone mapping) is the oracle's, as in tests/test_gpu_light_sampling.py; power-proportional candidates and the unbiased
spatial pass are their restatements'.

Sizes: 64 x 48 (whole tiles), 37 x 29 (partial tiles in both directions), 8 x 8 (one tile, one wavefront). Scene and cameras: the lamp
room and the camera pairs of tests/test_temporal_reproject_cpu.py. The off-screen, behind-the-camera and sky / emissive cases run
here only through code that the CPU run of the same header has shown to form no index from them."""
import ctypes as C

import numpy as np
import pytest

import light_sampling_ref as ls
import restir_unbiased_ref as ru
import temporal_reproject_ref as tr
from test_temporal_reproject_cpu import FOVY, View, _history, _orbit, _previous_view, _res_diff

pytestmark = pytest.mark.gpu

RT_ERR_ARG, RT_ERR_UNSUPPORTED = 1, 5  # include/restir_rt.h
SIZES = [(64, 48), (37, 29), (8, 8)]
OPTION_CASES = [dict(), dict(use_visibility_reuse=0), dict(use_shadowed_target_function=1), dict(use_shadowed_target_function=1, use_visibility_reuse=0)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _eq_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def world(oracle):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    tris = ls.make_lamp_room()
    return dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True))


def _epoch(r):
    e = C.c_uint64()
    assert r.L.rt_state_epoch(r.h, C.byref(e)) == 0
    return e.value


def _renderer(api, world, W, H, opt, on=True, **kw):
    r = api.Renderer(W, H, **kw)
    r.set_scene(world["tris"])
    r.set_options(opt)
    if on is not None:
        assert r.temporal_reprojection(on) is bool(on)
    return r


def _look(r, view):
    """the device camera = the view's: the same 36 bytes of RayGenerator, the same eye"""
    r.lookat(view.eye, view.at, fovy=FOVY)
    assert _eq_bits(r.raygen(), view.rg)


def _counts(cur, diag):
    q = np.arange(cur.W * cur.H)
    v = diag[:, 0] == 1
    return dict(merged=int(cur.shaded.sum()), valid=int(v.sum()), moved=int((v & ((diag[:, 1] != q % cur.W) | (diag[:, 2] != q // cur.W))).sum()))


def _kernel_path(api, oracle, world, W, H, kind, kw, frame=7):
    """(a): camera A, rt_raycast, upload a history; camera B, rt_raycast, rt_generate_candidate, rt_temporal_resampling"""
    opt = oracle.bench_options(**kw)
    cur, prev = View(oracle, world, W, H, ls.LAMP_EYE, ls.LAMP_AT), _previous_view(oracle, world, W, H, kind)
    hist = _history(oracle, world, prev, opt)
    r = _renderer(api, world, W, H, opt)
    _look(r, prev)
    r.raycast()
    assert _eq_bits(r.download(api.RT_BUF_VISIBILITY), prev.vis)
    r.upload(api.RT_BUF_RES_TEMPORAL, hist)
    assert _eq_bits(r.reservoir_camera(api.RT_RES_TEMPORAL), prev.rg)
    _look(r, cur)
    r.raycast()
    assert _eq_bits(r.download(api.RT_BUF_VISIBILITY), cur.vis)
    r.generate_candidate(frame, api.RT_RES_0)
    cand = r.download(api.RT_BUF_RES_0).copy()
    want_cand = world["scene"].generate_candidate(W, H, frame, cur.vis, cur.eye, opt)
    assert not _res_diff(cand, want_cand, cur.shaded)
    r.walk_stats_enable(True)
    r.temporal_resampling(frame, api.RT_RES_TEMPORAL, api.RT_RES_0)
    got = r.download(api.RT_BUF_RES_0)
    stats = r.temporal_reprojection_stats()
    r.walk_stats_enable(False)
    want, diag = tr.temporal(W, H, frame, world["tris"], cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, want_cand.copy())
    bad = _res_diff(got, want, cur.shaded)
    assert not bad, f"{kind} {W} x {H} {kw}: {bad} of {int(cur.shaded.sum())} shaded pixels"
    assert stats == _counts(cur, diag), f"{kind} {W} x {H}: counters {stats}, restatement {_counts(cur, diag)}"
    assert _eq_bits(r.reservoir_camera(api.RT_RES_0), cur.rg) and _eq_bits(r.reservoir_camera(api.RT_RES_TEMPORAL), prev.rg)
    # the same-pixel merge gives other records: the case shows the gather
    same = world["scene"].temporal_resampling(W, H, frame, cur.vis, cur.eye, opt, hist, want_cand.copy())
    r.close()
    return got, want, same, diag, cur


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kw", OPTION_CASES)
def test_kernel_path_equals_the_restatement(api, oracle, world, W, H, kw):
    got, want, same, diag, cur = _kernel_path(api, oracle, world, W, H, "orbit", kw)
    assert _res_diff(want, same, cur.shaded), "the orbit does not change the merge: the case covers nothing"
    assert diag[:, 0].sum() > cur.shaded.sum() // 2


# ------------------------------------------------------------------------------------------------------------------- (b)
class _Cpu:
    """the frame of 10_restir_di.cpp:257-379 on the CPU with one camera per frame: the oracle's kernels, the temporal merge from the
    restatement (history of the previous frame's camera), and where asked power candidates / the unbiased pass from theirs"""

    def __init__(self, oracle, world, W, H, opt, power=False, unbiased=False, reproject=True):
        self.o, self.w, self.W, self.H, self.opt, self.power, self.unbiased, self.reproject = oracle, world, W, H, opt, power, unbiased, reproject
        self.st = oracle.new_state(W, H)
        self.prev = None

    def frame(self, frame, view):
        sc, st, W, H, opt = self.w["scene"], self.st, self.W, self.H, self.opt
        st["vis"] = view.vis
        if self.power:
            ls.generate_candidate(W, H, frame, self.w["tris"], view.vis, view.eye, opt, ls.POWER, st["r0"])
        else:
            sc.generate_candidate(W, H, frame, view.vis, view.eye, opt, st["r0"])
        prev = view if self.prev is None else self.prev  # frame 1: zeros without a camera, the same-pixel merge
        if self.reproject:
            _, self.diag = tr.temporal(W, H, frame, self.w["tris"], view.vis, prev.vis, view.eye, prev.rg, view.rg, opt, st["temporal"], st["r0"])
        else:
            sc.temporal_resampling(W, H, frame, view.vis, view.eye, opt, st["temporal"], st["r0"])
        self.o.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        self.prev = view
        src, dst = "r0", "r1"
        for k in range(int(opt["spatial_resampling_passes"][0])):
            if k:
                src, dst = dst, src
            if self.unbiased:
                st[dst] = ru.spatial(W, H, frame, k, self.w["tris"], view.vis, view.eye, opt, st[src])[0]
            else:
                st[dst] = sc.spatial_resampling(W, H, frame, k, view.vis, view.eye, opt, st[src])
        sc.resolve(st["accum"], W, H, view.vis, view.eye, opt, st[dst])
        st["pixels"] = self.o.tone_mapping(st["accum"], W, H)
        return st[dst]


def _check_frame(api, r, out, cpu, last, view, what):
    W, H = cpu.W, cpu.H
    acc = r.download(api.RT_BUF_ACCUMULATION)
    assert _eq_bits(acc, cpu.st["accum"].reshape(acc.shape)), f"{what}: accumulation"
    assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), cpu.st["pixels"]), f"{what}: pixels"
    bad = _res_diff(r.download(api.RT_BUF_RES_0 + out), last, view.shaded)
    assert not bad, f"{what}: records after the frame {bad}"
    bad = _res_diff(r.download(api.RT_BUF_RES_TEMPORAL), cpu.st["temporal"], view.shaded)
    assert not bad, f"{what}: temporal history {bad}"
    assert _eq_bits(r.reservoir_camera(api.RT_RES_TEMPORAL), view.rg), f"{what}: the history's camera tag"


ORBIT_FRAMES, ORBIT_STEP = 6, 0.1

ORBIT_CASES = [
    # W, H, rt_tuning 25 (stage 0 as one launch), option overrides, power lights, unbiased passes, other knobs
    (64, 48, 1, dict(), False, False, ()),
    (64, 48, 0, dict(accumulate=1), False, False, ()),
    (37, 29, 1, dict(accumulate=1), False, False, ()),
    (37, 29, 0, dict(), False, False, ()),
    (8, 8, 1, dict(), False, False, ()),
    (8, 8, 0, dict(), False, False, ()),
    (37, 29, 1, dict(), False, True, ()),
    (37, 29, 1, dict(), True, False, ()),
    (37, 29, 0, dict(), True, False, ()),
    (37, 29, 1, dict(use_shadowed_target_function=1), False, False, ()),
    (37, 29, 1, dict(use_shadowed_target_function=1), True, False, ()),
    (37, 29, 0, dict(), False, False, ((13, 0),)),  # the fused kernel without the work-sharing walk
    (37, 29, 0, dict(), True, False, ((13, 0),)),
    (37, 29, 1, dict(), False, False, ((14, 0),)),  # no look-ahead
    (37, 29, 1, dict(spatial_resampling_passes=1), False, False, ()),  # the frame's end copies the history (and its tag)
]


@pytest.mark.parametrize("W,H,one_launch,kw,power,unbiased,knobs", ORBIT_CASES)
def test_frames_over_an_orbit_equal_the_cpu_sequence(api, oracle, world, W, H, one_launch, kw, power, unbiased, knobs):
    opt = oracle.bench_options(**kw)
    cpu = _Cpu(oracle, world, W, H, opt, power=power, unbiased=unbiased)
    r = _renderer(api, world, W, H, opt)
    r.tuning(api.Tune.WS_PRIMARY, 0)  # the whole frame's form at the benchmark size, as tests/test_gpu_light_sampling.py
    r.tuning(25, one_launch)
    for k, v in knobs:
        r.tuning(k, v)
    if power:
        r.light_sampling("power")
    if unbiased:
        assert r.spatial_unbiased(True) is True
    r.walk_stats_enable(True)
    gathered = 0
    for k in range(ORBIT_FRAMES):
        view = View(oracle, world, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT_STEP * k))
        _look(r, view)  # the camera call between the frames
        out = r.frame(1 + k)
        if k == 0 and one_launch and not kw.get("use_shadowed_target_function") and not knobs:
            assert r.stage0_one_launch(), "the frame did not take the one-launch stage 0: the case would not cover it"
        _check_frame(api, r, out, cpu, cpu.frame(1 + k, view), view, f"frame {1 + k}")
        gathered += int(cpu.diag[:, 0].sum())
    # frame 1 merges an untagged history (the launches of the mode off); the five others reproject every shaded pixel
    stats = r.temporal_reprojection_stats()
    assert stats["valid"] == gathered and stats["merged"] > 0 and gathered > 0, stats
    r.close()


# ------------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("W,H", [(64, 48), (37, 29)])
def test_static_camera_is_the_mode_off(api, oracle, world, W, H):
    """4 frames without a camera call: the mode on gives the bytes of the mode off, launches no primary rays the other does not, and
    takes the look-ahead's candidates as the other does"""
    opt = oracle.bench_options(accumulate=1)
    view = View(oracle, world, W, H, ls.LAMP_EYE, ls.LAMP_AT)
    a, b = _renderer(api, world, W, H, opt, on=True), _renderer(api, world, W, H, opt, on=None)
    cpu = _Cpu(oracle, world, W, H, opt, reproject=False)
    for r in (a, b):
        _look(r, view)
        r.tuning(api.Tune.WS_PRIMARY, 0)
    for frame in (1, 2, 3, 4):
        oa, ob_ = a.frame(frame), b.frame(frame)
        assert oa == ob_
        for buf in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0 + oa):
            assert _eq_bits(a.download(buf), b.download(buf)), f"frame {frame}: buffer {buf}"
        _check_frame(api, a, oa, cpu, cpu.frame(frame, view), view, f"frame {frame}")
        assert a.primary_launches() == b.primary_launches(), f"frame {frame}: primary launches"
        assert a.stage0_one_launch() == b.stage0_one_launch()
    assert a.primary_launches() < 4, "G-buffer reuse: a camera that stands still is not traced every frame"
    # and with the counters on, no launch of these frames was a reprojecting one
    a.walk_stats_enable(True)
    a.frame(5)
    assert a.temporal_reprojection_stats() == dict(merged=0, valid=0, moved=0)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("W,H", [(37, 29), (8, 8)])
@pytest.mark.parametrize("kind", ["pan_right", "pan_left", "pan_up", "pan_down", "away", "above", "zoom_out"])
def test_histories_off_the_image_behind_the_camera_and_on_sky_or_lamps(api, oracle, world, W, H, kind):
    got, want, same, diag, cur = _kernel_path(api, oracle, world, W, H, kind, dict())
    if kind == "away":
        assert not diag.any()
    else:
        assert (cur.shaded & (diag[:, 0] == 0)).any(), f"{kind}: every pixel found a history, the case covers nothing"


def test_shadowed_target_with_the_previous_camera_facing_away(api, oracle, world):
    _kernel_path(api, oracle, world, 37, 29, "away", dict(use_shadowed_target_function=1))


# ------------------------------------------------------------------------------------------------------------------- (e)
def test_errors_getters_tags_and_epoch(api, oracle, world):
    W, H = 37, 29
    opt = oracle.bench_options()
    a, b = View(oracle, world, W, H, ls.LAMP_EYE, ls.LAMP_AT), _previous_view(oracle, world, W, H, "orbit")
    r = _renderer(api, world, W, H, opt, on=None)
    assert r.temporal_reprojection() is False
    e0 = _epoch(r)
    assert r.temporal_reprojection(True) is True and _epoch(r) != e0
    e1 = _epoch(r)
    assert r.temporal_reprojection(False) is False and _epoch(r) != e1
    assert r.temporal_reprojection(True) is True
    # no buffer carries a camera before anything was written
    for res in (api.RT_RES_0, api.RT_RES_1, api.RT_RES_TEMPORAL):
        assert r.reservoir_camera(res) is None
    assert r.L.rt_reservoir_camera(r.h, 3, None, None) == RT_ERR_ARG
    _look(r, a)
    r.raycast()
    r.generate_candidate(1, api.RT_RES_0)
    assert _eq_bits(r.reservoir_camera(api.RT_RES_0), a.rg) and r.reservoir_camera(api.RT_RES_TEMPORAL) is None
    r.save_temporal_reservoir(api.RT_RES_0, api.RT_RES_TEMPORAL)
    assert _eq_bits(r.reservoir_camera(api.RT_RES_TEMPORAL), a.rg)
    assert r.L.rt_temporal_resampling(r.h, 2, api.RT_RES_0, api.RT_RES_0) == RT_ERR_ARG  # prev == inout: with a gather, a race
    _look(r, b)
    r.raycast()
    r.upload(api.RT_BUF_RES_1, np.zeros(W * H, dtype=oracle.RESERVOIR))
    assert _eq_bits(r.reservoir_camera(api.RT_RES_1), b.rg) and _eq_bits(r.reservoir_camera(api.RT_RES_TEMPORAL), a.rg)
    # rt_frame: the history it leaves carries the frame's camera, whichever physical buffer now has the name
    r.frame(2)
    assert _eq_bits(r.reservoir_camera(api.RT_RES_TEMPORAL), b.rg)
    _look(r, a)
    r.frame(3)
    assert _eq_bits(r.reservoir_camera(api.RT_RES_TEMPORAL), a.rg)
    r.set_scene(world["tris"])
    for res in (api.RT_RES_0, api.RT_RES_1, api.RT_RES_TEMPORAL):
        assert r.reservoir_camera(res) is None, "rt_scene_set clears the tags"
    r.close()
    # a strip context holds only its own rows of the history
    s = api.Renderer(W, H, rows=(8, 20), halo=4)
    assert s.L.rt_temporal_reprojection(s.h, 1) == RT_ERR_UNSUPPORTED
    assert s.L.rt_temporal_reprojection(s.h, 0) == RT_ERR_UNSUPPORTED
    assert s.temporal_reprojection() is False
    s.close()


@pytest.mark.parametrize("key", [11, 12])
def test_experiment_stage0_forms_refuse_a_moved_camera(api, oracle, world, key):
    """[exp] rt_tuning 11 / 12 gather their history from the own pixel only: fine while the camera stands still, RT_ERR_UNSUPPORTED from
    the frame after it moved"""
    W, H = 37, 29
    r = _renderer(api, world, W, H, oracle.bench_options(), exp=True)
    r.tuning(key, 1)
    _look(r, View(oracle, world, W, H, ls.LAMP_EYE, ls.LAMP_AT))
    r.frame(1)
    r.frame(2)
    _look(r, _previous_view(oracle, world, W, H, "orbit"))
    out = C.c_int(-1)
    assert r.L.rt_frame(r.h, 3, 0, C.byref(out)) == RT_ERR_UNSUPPORTED
    r.close()
