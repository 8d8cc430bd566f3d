"""rt_temporal_unbiased on the device: k_temporal_unbiased through rt_temporal_resampling and as the second launch of a staged frame's
stage 0, against tests/temporal_unbiased_ref.py (the restatement compiled from the kernel's own headers, anchored by
tests/test_temporal_unbiased_cpu.py), bit for bit. Everything around the temporal merge (primary rays, candidates, spatial passes,
resolve, tone mapping) is the oracle's, as in tests/test_gpu_temporal_reproject.py; power-proportional candidates and the unbiased
spatial pass are their restatements'.

Sizes: 64 x 48 (whole tiles), 37 x 29 (partial tiles in both directions), 17 x 9 (three tile columns, the last with one pixel; two
tile rows, the second with one row), 8 x 8 (one tile). Scenes: the quad room of the bias study and the lamp room of
tests/light_sampling_ref.py. The off-image, behind-the-camera and sky / emissive cases run here only through code that the CPU run of
the same headers has shown to form no index from them."""
import ctypes as C

import numpy as np
import pytest

import light_sampling_ref as ls
import restir_unbiased_ref as ru
import temporal_reproject_ref as tr
import temporal_unbiased_ref as tu
from test_temporal_reproject_cpu import FOVY, View, _history, _orbit, _pan, _res_diff, _zoom
from test_temporal_unbiased_cpu import EDGE_PANS, beyond_edge, edge_pan_view

pytestmark = pytest.mark.gpu

RT_ERR_ARG, RT_ERR_UNSUPPORTED = 1, 5  # include/restir_rt.h
QUAD_EYE, QUAD_AT = (0.5, 3.0, 6.0), (0.0, 1.0, -1.5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _eq_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def worlds(oracle):
    from cedec_2024_rt_amd import scenes

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    out = {}
    for name, tris, eye, at in (("quad", scenes.make_quad_room(), QUAD_EYE, QUAD_AT), ("lamp", ls.make_lamp_room(), ls.LAMP_EYE, ls.LAMP_AT)):
        out[name] = dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True), eye=eye, at=at)
    return out


def _epoch(r):
    e = C.c_uint64()
    assert r.L.rt_state_epoch(r.h, C.byref(e)) == 0
    return e.value


def _renderer(api, world, W, H, opt, on=True, **kw):
    r = api.Renderer(W, H, **kw)
    r.set_scene(world["tris"])
    r.set_options(opt)
    assert r.temporal_reprojection(True) is True
    if on is not None:
        assert r.temporal_unbiased(on) is bool(on)
    return r


def _look(r, view):
    """the device camera = the view's: the same 36 bytes of RayGenerator, the same eye"""
    r.lookat(view.eye, view.at, fovy=FOVY)
    assert _eq_bits(r.raygen(), view.rg)


def _previous_view(oracle, world, W, H, kind):
    """the camera the history was written under, for the world's current camera"""
    eye, at = world["eye"], world["at"]
    if kind == "orbit":
        eye, at = _orbit(eye, at, 0.3)
    elif kind == "zoom":  # the previous camera was farther away
        eye, at = _zoom(eye, at, 1.25)
    elif kind == "pan":  # the previous camera stood 1.2 units to the left: part of the current image lies off its edge
        eye, at = _pan(oracle, eye, at, W, H, -1.2, 0.0)
    elif kind == "away":  # looking the other way from the same place
        e, a = np.asarray(eye, np.float32), np.asarray(at, np.float32)
        eye, at = e, np.asarray(e + (e - a), np.float32)
    else:
        raise KeyError(kind)
    return View(oracle, world, W, H, eye, at)


def _counts(cur, diag):
    return dict(merged=int(cur.shaded.sum()), valid=int((diag[:, 4] > 0).sum()), excluded=int(((diag[:, 4] > 0) & (diag[:, 2] == 0)).sum()),
                history_rays=int(diag[:, 3].sum()))


# ------------------------------------------------------------------------------------------------------------------- (a)
KERNEL_CASES = [("lamp", W, H, kind, vr) for (W, H) in ((64, 48), (37, 29), (17, 9), (8, 8)) for kind in ("orbit", "zoom", "pan", "away") for vr in (1, 0)]
KERNEL_CASES += [("quad", W, H, kind, vr) for (W, H) in ((64, 48), (37, 29), (17, 9), (8, 8)) for kind in ("orbit", "zoom") for vr in (1, 0)]


def _reproject_counts(world, cur, prev, diag, merged):
    """rt_temporal_reprojection_stats of unbiased launches: an unbiased launch is a reprojecting one and counts each pixel once"""
    pts, _ = tr.surface_points(world["tris"], cur.vis, cur.eye)
    pix, _ = tr.project(pts, prev.rg, cur.W, cur.H)
    q = np.arange(cur.W * cur.H)
    v = diag[:, 0] == 1
    return dict(merged=merged, valid=int(v.sum()), moved=int((v & ((pix[:, 1] != q % cur.W) | (pix[:, 2] != q // cur.W))).sum()))


def _kernel_path(api, oracle, world, W, H, cur, prev, vis_reuse, what, frame=7):
    """camera A, rt_raycast, upload a history; camera B, rt_raycast, rt_generate_candidate, rt_temporal_resampling"""
    opt = oracle.bench_options(use_visibility_reuse=vis_reuse)
    hist = _history(oracle, world, prev, opt)
    r = _renderer(api, world, W, H, opt)
    _look(r, prev)
    r.raycast()
    r.upload(api.RT_BUF_RES_TEMPORAL, hist)
    _look(r, cur)
    r.raycast()
    assert _eq_bits(r.download(api.RT_BUF_VISIBILITY), cur.vis)
    r.generate_candidate(frame, api.RT_RES_0)
    want_cand = world["scene"].generate_candidate(W, H, frame, cur.vis, cur.eye, opt)
    assert not _res_diff(r.download(api.RT_BUF_RES_0), want_cand, cur.shaded)
    r.walk_stats_enable(True)
    r.temporal_resampling(frame, api.RT_RES_TEMPORAL, api.RT_RES_0)
    got = r.download(api.RT_BUF_RES_0)
    stats, rstats = r.temporal_unbiased_stats(), r.temporal_reprojection_stats()
    r.walk_stats_enable(False)
    want, diag = tu.temporal(W, H, frame, world["tris"], cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, want_cand.copy())
    bad = _res_diff(got, want, cur.shaded)
    assert not bad, f"{what} {W} x {H} vis_reuse {vis_reuse}: {bad} of {int(cur.shaded.sum())} shaded pixels"
    assert stats == _counts(cur, diag), f"{what} {W} x {H}: counters {stats}, restatement {_counts(cur, diag)}"
    want_r = _reproject_counts(world, cur, prev, diag, int(cur.shaded.sum()))
    assert rstats == want_r, f"{what} {W} x {H}: reprojection counters {rstats}, restatement {want_r}"
    assert _eq_bits(r.reservoir_camera(api.RT_RES_0), cur.rg) and _eq_bits(r.reservoir_camera(api.RT_RES_TEMPORAL), prev.rg)
    r.close()
    return got, want, want_cand, diag, opt, hist


@pytest.mark.parametrize("room,W,H,kind,vis_reuse", KERNEL_CASES)
def test_kernel_path_equals_the_restatement(api, oracle, worlds, room, W, H, kind, vis_reuse, frame=7):
    world = worlds[room]
    cur, prev = View(oracle, world, W, H, world["eye"], world["at"]), _previous_view(oracle, world, W, H, kind)
    got, want, want_cand, diag, opt, hist = _kernel_path(api, oracle, world, W, H, cur, prev, vis_reuse, f"{room} {kind}", frame)
    if kind == "away":
        assert not diag[:, :5].any()
    elif (W, H) == (64, 48):
        # the case shows the estimator: histories merged, some kept out of Z, and the 1/M merge gives other records
        biased, _ = tu.temporal(W, H, frame, world["tris"], cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, want_cand.copy(), mode=tu.REPROJECT)
        assert diag[:, 0].sum() > cur.shaded.sum() // 2 and _res_diff(want, biased, cur.shaded)
        # without visibility reuse only a geometry term of exactly zero keeps a history out, and no light of these rooms lies in a surface's plane
        assert not vis_reuse or (diag[:, 3].any() and _counts(cur, diag)["excluded"] > 0)


@pytest.mark.parametrize("W,H", [(37, 29), (17, 9)])
@pytest.mark.parametrize("edge", list(EDGE_PANS))
def test_histories_off_each_edge(api, oracle, worlds, W, H, edge):
    """the four pans of tests/test_temporal_unbiased_cpu.py on the quad room: pixels that project past the left, right, low-row and
    high-row edge of the previous image keep their candidates' records, the kernel equals the restatement everywhere"""
    world = worlds["quad"]
    cur, prev = edge_pan_view(oracle, world, W, H, edge)
    out = beyond_edge(world["tris"], cur, prev, edge)
    assert out.sum() >= 6
    got, want, want_cand, diag, opt, hist = _kernel_path(api, oracle, world, W, H, cur, prev, 1, f"quad pan {edge}")
    assert not diag[out, :5].any() and not _res_diff(got, want_cand, out)


# ------------------------------------------------------------------------------------------------------------------- (b)
class _Cpu:
    """the frame of 10_restir_di.cpp:257-379 on the CPU with one camera per frame: the oracle's kernels, the temporal merge from the
    restatement (history of the previous frame's camera), and where asked power candidates / the unbiased passes from theirs"""

    def __init__(self, oracle, world, W, H, opt, power=False, spatial_unbiased=False, mode=tu.UNBIASED):
        self.o, self.w, self.W, self.H, self.opt, self.power, self.su, self.mode = oracle, world, W, H, opt, power, spatial_unbiased, mode
        self.st = oracle.new_state(W, H)
        self.prev = None
        self.counts = dict(merged=0, valid=0, excluded=0, history_rays=0)
        self.from_hist = 0
        self.gathered = 0  # valid histories of the unbiased launches

    def frame(self, frame, view):
        sc, st, W, H, opt = self.w["scene"], self.st, self.W, self.H, self.opt
        st["vis"] = view.vis
        if self.power:
            ls.generate_candidate(W, H, frame, self.w["tris"], view.vis, view.eye, opt, ls.POWER, st["r0"])
        else:
            sc.generate_candidate(W, H, frame, view.vis, view.eye, opt, st["r0"])
        prev = view if self.prev is None else self.prev  # frame 1: zeros without a camera, the same-pixel merge
        _, self.diag = tu.temporal(W, H, frame, self.w["tris"], view.vis, prev.vis, view.eye, prev.rg, view.rg, opt, st["temporal"], st["r0"], mode=self.mode)
        if self.mode == tu.UNBIASED and not _eq_bits(prev.rg, view.rg):
            for k, v in _counts(view, self.diag).items():
                self.counts[k] += v
            self.gathered += int(self.diag[:, 0].sum())
        self.from_hist = int(self.diag[:, 1].sum())
        self.o.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        self.prev = view
        src, dst = "r0", "r1"
        if not int(opt["use_spatial_resampling"][0]):
            dst = "r0"
        else:
            for k in range(int(opt["spatial_resampling_passes"][0])):
                if k:
                    src, dst = dst, src
                if self.su:
                    st[dst] = ru.spatial(W, H, frame, k, self.w["tris"], view.vis, view.eye, opt, st[src])[0]
                else:
                    st[dst] = sc.spatial_resampling(W, H, frame, k, view.vis, view.eye, opt, st[src])
        sc.resolve(st["accum"], W, H, view.vis, view.eye, opt, st[dst])
        st["pixels"] = self.o.tone_mapping(st["accum"], W, H)
        return st[dst]


def _check_frame(api, r, out, cpu, last, view, what):
    W, H = cpu.W, cpu.H
    bad = _res_diff(r.download(api.RT_BUF_RES_TEMPORAL), cpu.st["temporal"], view.shaded)
    assert not bad, f"{what}: temporal history {bad}"
    bad = _res_diff(r.download(api.RT_BUF_RES_0 + out), last, view.shaded)
    assert not bad, f"{what}: records after the frame {bad}"
    acc = r.download(api.RT_BUF_ACCUMULATION)
    assert _eq_bits(acc, cpu.st["accum"].reshape(acc.shape)), f"{what}: accumulation"
    assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), cpu.st["pixels"]), f"{what}: pixels"
    assert _eq_bits(r.reservoir_camera(api.RT_RES_TEMPORAL), view.rg), f"{what}: the history's camera tag"


ORBIT_STEPS, ORBIT_STEP = 4, 0.15

ORBIT_CASES = [
    # room, W, H, rt_tuning 25 (stage 0 as one launch), option overrides, power lights, unbiased passes, occluder hints, other knobs
    ("quad", 64, 48, 1, dict(), False, False, True, ()),
    ("quad", 64, 48, 0, dict(accumulate=1), False, False, True, ()),
    ("lamp", 37, 29, 1, dict(accumulate=1), False, False, True, ()),
    ("lamp", 37, 29, 0, dict(), False, False, True, ()),
    ("lamp", 17, 9, 1, dict(), False, False, True, ()),
    ("lamp", 8, 8, 0, dict(), False, False, True, ()),
    ("quad", 37, 29, 1, dict(), False, True, True, ()),   # both unbiased toggles
    ("quad", 37, 29, 0, dict(), False, True, True, ()),
    ("lamp", 37, 29, 1, dict(), True, False, True, ()),   # power light sampling
    ("lamp", 37, 29, 0, dict(), True, False, True, ()),
    ("quad", 37, 29, 1, dict(), False, False, False, ()),  # no occluder hints
    ("quad", 37, 29, 0, dict(), False, False, False, ()),
    ("quad", 37, 29, 0, dict(), False, False, True, ((13, 0),)),  # the candidates' kernel without the work-sharing walk
    ("quad", 37, 29, 1, dict(), False, False, True, ((14, 0),)),  # no look-ahead
    ("quad", 37, 29, 1, dict(), False, False, True, ((17, 0),)),  # no pipelined tail
    ("quad", 37, 29, 1, dict(), False, False, True, ((20, 0),)),  # tone mapping as a launch of its own
    ("quad", 37, 29, 1, dict(use_visibility_reuse=0), False, False, True, ()),
    ("quad", 37, 29, 1, dict(use_spatial_resampling=0), False, False, True, ()),  # resolve reads what stage 0 wrote
]


@pytest.mark.parametrize("room,W,H,one_launch,kw,power,spatial_unbiased,hints,knobs", ORBIT_CASES)
def test_frames_over_an_orbit_equal_the_cpu_sequence(api, oracle, worlds, room, W, H, one_launch, kw, power, spatial_unbiased, hints, knobs):
    world = worlds[room]
    opt = oracle.bench_options(**kw)
    cpu = _Cpu(oracle, world, W, H, opt, power=power, spatial_unbiased=spatial_unbiased)
    r = _renderer(api, world, W, H, opt)
    r.tuning(api.Tune.WS_PRIMARY, 0)  # the whole frame's form at the benchmark size, as tests/test_gpu_light_sampling.py
    r.tuning(25, one_launch)
    for k, v in knobs:
        r.tuning(k, v)
    if power:
        r.light_sampling("power")
    if spatial_unbiased:
        assert r.spatial_unbiased(True) is True
    r.occluder_hints(hints)
    r.walk_stats_enable(True)
    for k in range(ORBIT_STEPS + 1):
        view = View(oracle, world, W, H, *_orbit(world["eye"], world["at"], -ORBIT_STEP * (ORBIT_STEPS - k)))
        _look(r, view)  # the camera call between the frames
        out = r.frame(1 + k)
        if k == 0 and one_launch and not knobs:
            assert r.stage0_one_launch(), "the frame did not take the one-launch stage 0: the case would not cover it"
        _check_frame(api, r, out, cpu, cpu.frame(1 + k, view), view, f"frame {1 + k}")
    # frame 1 merges an untagged history (the launches of the toggle off); the four others are unbiased launches
    stats = r.temporal_unbiased_stats()
    assert stats == cpu.counts and stats["valid"] > 0, (stats, cpu.counts)
    # an unbiased stage 0 is two launches and still counts every shaded pixel once as merged by a reprojecting launch
    rstats = r.temporal_reprojection_stats()
    assert (rstats["merged"], rstats["valid"]) == (cpu.counts["merged"], cpu.gathered), (rstats, cpu.counts, cpu.gathered)
    r.close()


def test_resolve_does_not_walk_the_own_rays_again(api, oracle, worlds):
    """no spatial passes, so resolve reads stage 0's records: with the toggle on every own ray is known (the candidates' launch walked
    the surviving candidates', k_temporal_unbiased the ones of the pixels whose history won); with it off the latter are walked"""
    world, W, H = worlds["quad"], 64, 48
    opt = oracle.bench_options(use_spatial_resampling=0)
    views = [View(oracle, world, W, H, *_orbit(world["eye"], world["at"], -ORBIT_STEP * (1 - k))) for k in range(2)]
    seen = {}
    for on in (True, False):
        cpu = _Cpu(oracle, world, W, H, opt, mode=tu.UNBIASED if on else tu.REPROJECT)
        r = _renderer(api, world, W, H, opt, on=on)
        _look(r, views[0])
        _check_frame(api, r, r.frame(1), cpu, cpu.frame(1, views[0]), views[0], "frame 1")
        _look(r, views[1])
        r.walk_stats_enable(True)
        _check_frame(api, r, r.frame(2), cpu, cpu.frame(2, views[1]), views[1], "frame 2")
        seen[on] = (r.walk_stats()["resolve"], cpu.from_hist, int(views[1].shaded.sum()))
        r.close()
    res, from_hist, shaded = seen[True]
    assert from_hist > 0 and res["walked"] + res["self_test"] == 0 and res["not_evaluated"] == shaded == res["reference_rays"], seen
    res, from_hist, shaded = seen[False]
    assert from_hist > 0 and res["walked"] + res["self_test"] == from_hist and res["not_evaluated"] == shaded - from_hist, seen


# ------------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("W,H", [(64, 48), (37, 29)])
def test_static_camera_is_the_toggle_off(api, oracle, worlds, W, H):
    """4 frames without a camera call: the toggle on gives the bytes of the toggle off, launches no primary rays the other does not,
    takes the look-ahead's candidates as the other does, and counts no unbiased launch"""
    world = worlds["quad"]
    opt = oracle.bench_options(accumulate=1)
    view = View(oracle, world, W, H, world["eye"], world["at"])
    a, b = _renderer(api, world, W, H, opt, on=True), _renderer(api, world, W, H, opt, on=None)
    for r in (a, b):
        _look(r, view)
        r.tuning(api.Tune.WS_PRIMARY, 0)
    for frame in (1, 2, 3, 4):
        oa, ob_ = a.frame(frame), b.frame(frame)
        assert oa == ob_
        for buf in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0 + oa):
            assert _eq_bits(a.download(buf), b.download(buf)), f"frame {frame}: buffer {buf}"
        assert a.primary_launches() == b.primary_launches(), f"frame {frame}: primary launches"
        assert a.stage0_one_launch() == b.stage0_one_launch()
    assert a.primary_launches() < 4, "G-buffer reuse: a camera that stands still is not traced every frame"
    a.walk_stats_enable(True)
    b.walk_stats_enable(True)
    a.frame(5)
    b.frame(5)
    assert a.temporal_unbiased_stats() == dict(merged=0, valid=0, excluded=0, history_rays=0)
    assert a.walk_stats() == b.walk_stats(), "the same launches walk the same rays"
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------- (d)
def test_errors_getter_and_epoch(api, oracle, worlds):
    world, W, H = worlds["quad"], 37, 29
    a, b = View(oracle, world, W, H, world["eye"], world["at"]), _previous_view(oracle, world, W, H, "orbit")
    r = _renderer(api, world, W, H, oracle.bench_options(), on=None)
    assert r.temporal_unbiased() is False
    e0 = _epoch(r)
    assert r.temporal_unbiased(True) is True and _epoch(r) != e0
    e1 = _epoch(r)
    assert r.temporal_unbiased(False) is False and _epoch(r) != e1
    assert r.L.rt_temporal_unbiased_get(r.h, None) == RT_ERR_ARG
    # rt_temporal_motion and this toggle: the second call refuses, whichever it is
    assert r.temporal_unbiased(True) is True
    assert r.L.rt_temporal_motion(r.h, 1) == RT_ERR_UNSUPPORTED and r.temporal_motion() is False
    assert r.temporal_unbiased(False) is False and r.temporal_motion(True) is True
    assert r.L.rt_temporal_unbiased(r.h, 1) == RT_ERR_UNSUPPORTED and r.temporal_unbiased() is False
    assert r.temporal_motion(False) is False and r.temporal_unbiased(True) is True
    # prev == inout stays refused
    _look(r, a)
    r.raycast()
    r.generate_candidate(1, api.RT_RES_0)
    assert r.L.rt_temporal_resampling(r.h, 2, api.RT_RES_0, api.RT_RES_0) == RT_ERR_ARG
    r.close()
    # the shadowed target function: fine while the camera stands still, refused at an unbiased launch
    r = _renderer(api, world, W, H, oracle.bench_options(use_shadowed_target_function=1))
    _look(r, a)
    r.frame(1)
    r.frame(2)
    _look(r, b)
    out = C.c_int(-1)
    assert r.L.rt_frame(r.h, 3, 0, C.byref(out)) == RT_ERR_UNSUPPORTED
    r.close()
    r = _renderer(api, world, W, H, oracle.bench_options(use_shadowed_target_function=1))
    _look(r, b)
    r.raycast()
    r.generate_candidate(4, api.RT_RES_0)
    _look(r, a)
    r.raycast()
    r.generate_candidate(4, api.RT_RES_1)
    assert r.L.rt_temporal_resampling(r.h, 4, api.RT_RES_0, api.RT_RES_1) == RT_ERR_UNSUPPORTED
    r.close()
    # a strip context holds only its own rows of the history
    s = api.Renderer(W, H, rows=(8, 20), halo=4)
    assert s.L.rt_temporal_unbiased(s.h, 1) == RT_ERR_UNSUPPORTED
    assert s.L.rt_temporal_unbiased(s.h, 0) == RT_ERR_UNSUPPORTED
    assert s.temporal_unbiased() is False
    s.close()


@pytest.mark.parametrize("key", [11, 12])
def test_experiment_stage0_forms_refuse_an_unbiased_launch(api, oracle, worlds, key):
    world, W, H = worlds["quad"], 37, 29
    r = _renderer(api, world, W, H, oracle.bench_options(), exp=True)
    r.tuning(key, 1)
    _look(r, View(oracle, world, W, H, world["eye"], world["at"]))
    r.frame(1)
    r.frame(2)
    _look(r, _previous_view(oracle, world, W, H, "orbit"))
    out = C.c_int(-1)
    assert r.L.rt_frame(r.h, 3, 0, C.byref(out)) == RT_ERR_UNSUPPORTED
    r.close()
