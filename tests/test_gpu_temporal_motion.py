"""rt_temporal_motion on the device: k_temporal<.., MOTION> and the fused k_generate_candidate<.., MOTION> forms against
tests/temporal_motion_ref.py (the restatement compiled from the kernels' own headers, anchored by tests/test_temporal_motion_cpu.py),
bit for bit, and the host's bookkeeping of generations, moved range and previous vertices. Everything around the temporal merge is the
oracle's, as in tests/test_gpu_temporal_reproject.py.

Sizes: 64 x 48 (whole tiles), 37 x 29 (partial tiles in both directions), 8 x 8 (one tile, one wavefront). Scene: the lamp room; its box
(triangles 64-75) moves. The NaN / infinite / degenerate previous vertices run on the CPU only, through the same header."""
import ctypes as C

import numpy as np
import pytest

import light_sampling_ref as ls
import restir_unbiased_ref as ru
import temporal_motion_ref as tm
import temporal_reproject_ref as tr
from test_temporal_motion_cpu import BOX_HI, BOX_LO, MOVES, Worlds, move, on_box, other_pixel
from test_temporal_reproject_cpu import FOVY, _history, _orbit, _res_diff

pytestmark = pytest.mark.gpu

RT_ERR_ARG, RT_ERR_UNSUPPORTED = 1, 5  # include/restir_rt.h
SIZES = [(64, 48), (37, 29), (8, 8)]
OPTION_CASES = [dict(), dict(use_visibility_reuse=0), dict(use_shadowed_target_function=1), dict(use_shadowed_target_function=1, use_visibility_reuse=0)]
ORBIT = 0.3


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
    return Worlds(oracle)


def _epoch(r):
    e = C.c_uint64()
    assert r.L.rt_state_epoch(r.h, C.byref(e)) == 0
    return e.value


def _renderer(api, tris, W, H, opt, reproject=True, motion=True, **kw):
    r = api.Renderer(W, H, **kw)
    r.set_scene(tris)
    r.set_options(opt)
    if reproject:
        assert r.temporal_reprojection(True) is True
    if motion is not None:
        assert r.temporal_motion(motion) is bool(motion)
    return r


def _look(r, view):
    r.lookat(view.eye, view.at, fovy=FOVY)
    assert _eq_bits(r.raygen(), view.rg)


def _update_box(r, world, first=BOX_LO, count=BOX_HI - BOX_LO):
    r.update_scene(world["tris"][first:first + count], first=first)


def _counts(cur, diag):
    return dict(merged=int(cur.shaded.sum()), in_range=int((diag[:, 3] == 1).sum()), valid=int(((diag[:, 3] == 1) & (diag[:, 0] == 1)).sum()))


def _prev_view(worlds, world, W, H, orbit):
    return worlds.view(world, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT)) if orbit else worlds.view(world, W, H)


# ------------------------------------------------------------------------------------------------------------- kernel path
def _kernel_path(api, oracle, worlds, W, H, kw, orbit, offset=MOVES[0], frame=7):
    """scene A and camera A, rt_raycast, upload a history (it is tagged); rt_scene_update with the moved box; the same camera or
    another; rt_raycast, rt_generate_candidate, rt_temporal_resampling"""
    opt = oracle.bench_options(**kw)
    wa, wb = worlds.of(worlds.base), worlds.moved(offset)
    prev, cur = _prev_view(worlds, wa, W, H, orbit), worlds.view(wb, W, H)
    hist = _history(oracle, wa, prev, opt)
    r = _renderer(api, wa["tris"], W, H, opt)
    _look(r, prev)
    r.raycast()
    assert _eq_bits(r.download(api.RT_BUF_VISIBILITY), prev.vis)
    r.upload(api.RT_BUF_RES_TEMPORAL, hist)
    gen, eye = r.reservoir_scene(api.RT_RES_TEMPORAL)
    assert gen == 0 and _eq_bits(eye, prev.eye)
    _update_box(r, wb)
    assert r.temporal_motion_range() == dict(lo=BOX_LO, hi=BOX_HI, generation=0)
    _look(r, cur)
    r.raycast()
    assert _eq_bits(r.download(api.RT_BUF_VISIBILITY), cur.vis)
    r.generate_candidate(frame, api.RT_RES_0)
    want_cand = wb["scene"].generate_candidate(W, H, frame, cur.vis, cur.eye, opt)
    assert not _res_diff(r.download(api.RT_BUF_RES_0), want_cand, cur.shaded)
    r.walk_stats_enable(True)
    r.temporal_resampling(frame, api.RT_RES_TEMPORAL, api.RT_RES_0)
    got = r.download(api.RT_BUF_RES_0)
    stats = r.temporal_motion_stats()
    r.walk_stats_enable(False)
    want, diag = tm.temporal(W, H, frame, wb["tris"], wa["tris"], cur.vis, prev.vis, cur.eye, prev.eye, prev.rg, cur.rg, BOX_LO, BOX_HI, opt, hist, want_cand.copy())
    bad = _res_diff(got, want, cur.shaded)
    assert not bad, f"{W} x {H} {kw} orbit={orbit}: {bad} of {int(cur.shaded.sum())} shaded pixels"
    assert stats == _counts(cur, diag), f"{W} x {H}: counters {stats}, restatement {_counts(cur, diag)}"
    assert r.reservoir_scene(api.RT_RES_0)[0] == 1 and r.reservoir_scene(api.RT_RES_TEMPORAL)[0] == 0
    # the launch of the toggle off gives other records on the box: the case shows the lookup
    r23, _ = tr.temporal(W, H, frame, wb["tris"], cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, want_cand.copy())
    assert _res_diff(want, r23, on_box(cur)) and not _res_diff(want, r23, cur.shaded & ~on_box(cur))
    assert other_pixel(diag, W)[on_box(cur)].any(), "no pixel of the box gathers from another pixel: the case covers nothing"
    r.close()


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kw", OPTION_CASES)
@pytest.mark.parametrize("orbit", [False, True])
def test_kernel_path_equals_the_restatement(api, oracle, worlds, W, H, kw, orbit):
    _kernel_path(api, oracle, worlds, W, H, kw, orbit)


def test_kernel_path_with_a_sideways_move_at_8_x_8(api, oracle, worlds):
    _kernel_path(api, oracle, worlds, 8, 8, dict(), False, offset=MOVES[1])


# -------------------------------------------------------------------------------------------------------------- frame path
class _Cpu:
    """the frame of 10_restir_di.cpp:257-379 on the CPU with one scene and one camera per frame: the oracle's kernels, the temporal merge
    from the restatement (follow) or from the reprojection's (not follow: the toggle off), and where asked power candidates / the
    unbiased pass from theirs"""

    def __init__(self, oracle, W, H, opt, power=False, unbiased=False, follow=True):
        self.o, self.W, self.H, self.opt, self.power, self.unbiased, self.follow = oracle, W, H, opt, power, unbiased, follow
        self.st = oracle.new_state(W, H)
        self.prev = None
        self.diag = np.zeros((W * H, 4), np.int32)

    def frame(self, frame, world, view):
        sc, st, W, H, opt = world["scene"], self.st, self.W, self.H, self.opt
        st["vis"] = view.vis
        if self.power:
            ls.generate_candidate(W, H, frame, world["tris"], view.vis, view.eye, opt, ls.POWER, st["r0"])
        else:
            sc.generate_candidate(W, H, frame, view.vis, view.eye, opt, st["r0"])
        if self.prev is None:  # frame 1: a history of zeros without a tag, the same-pixel merge
            sc.temporal_resampling(W, H, frame, view.vis, view.eye, opt, st["temporal"], st["r0"])
        elif self.follow:
            pw, pv = self.prev
            _, self.diag = tm.temporal(W, H, frame, world["tris"], pw["tris"], view.vis, pv.vis, view.eye, pv.eye, pv.rg, view.rg, BOX_LO, BOX_HI, opt, st["temporal"], st["r0"])
        else:
            pw, pv = self.prev
            tr.temporal(W, H, frame, world["tris"], view.vis, pv.vis, view.eye, pv.rg, view.rg, opt, st["temporal"], st["r0"])
        self.o.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        self.prev = (world, view)
        src, dst = "r0", "r1"
        for k in range(int(opt["spatial_resampling_passes"][0])):
            if k:
                src, dst = dst, src
            if self.unbiased:
                st[dst] = ru.spatial(W, H, frame, k, world["tris"], view.vis, view.eye, opt, st[src])[0]
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


# the box starts 2 units back and comes forward by 1 unit per frame: at 8 x 8 its 6 and 9 pixels of frames 4 and 5 gather 2 and 9
# histories from other pixels with the camera standing still (6 and 8 under the orbit); smaller steps leave 8 x 8 without one
FRAMES, FRAME_START, FRAME_STEP, FRAME_ORBIT = 5, (0.0, 0.0, -2.0), (0.0, 0.0, 1.0), 0.1


def _frame_worlds(worlds):
    t = move(worlds.base, FRAME_START)
    out = [worlds.of(t)]
    for _ in range(1, FRAMES):
        t = move(t, FRAME_STEP)
        out.append(worlds.of(t))
    return out


def _run_frames(api, oracle, worlds, W, H, one_launch, kw, power, unbiased, knobs, orbit, follow=True):
    opt = oracle.bench_options(**kw)
    ws = _frame_worlds(worlds)
    cpu = _Cpu(oracle, W, H, opt, power=power, unbiased=unbiased, follow=follow)
    r = _renderer(api, ws[0]["tris"], W, H, opt, motion=follow)
    r.tuning(api.Tune.WS_PRIMARY, 0)  # the whole frame's form at the benchmark size, as tests/test_gpu_light_sampling.py
    r.tuning(25, one_launch)
    for k, v in knobs:
        r.tuning(k, v)
    if power:
        r.light_sampling("power")
    if unbiased:
        assert r.spatial_unbiased(True) is True
    r.walk_stats_enable(True)
    want = dict(merged=0, in_range=0, valid=0)
    gathered_elsewhere = 0
    for k, w in enumerate(ws):
        view = worlds.view(w, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, FRAME_ORBIT * k if orbit else 0.0))
        if k:
            _update_box(r, w)
            assert r.temporal_motion_range() == (dict(lo=BOX_LO, hi=BOX_HI, generation=k - 1) if follow else dict(lo=0, hi=0, generation=0))
        _look(r, view)  # the camera call between the frames
        out = r.frame(1 + k)
        if k == 0 and one_launch and not kw.get("use_shadowed_target_function") and not knobs:
            assert r.stage0_one_launch(), "the frame did not take the one-launch stage 0: the case would not cover it"
        _check_frame(api, r, out, cpu, cpu.frame(1 + k, w, view), view, f"frame {1 + k}")
        gen, eye = r.reservoir_scene(api.RT_RES_TEMPORAL)
        assert gen == k and _eq_bits(eye, view.eye), f"frame {1 + k}: the history's scene tag"
        if k and follow:
            for key, v in _counts(view, cpu.diag).items():
                want[key] += v
            gathered_elsewhere += int(other_pixel(cpu.diag, W)[on_box(view)].sum())
    stats = r.temporal_motion_stats()
    r.close()
    return stats, want, gathered_elsewhere


FRAME_CASES = [
    # W, H, rt_tuning 25 (stage 0 as one launch), option overrides, power lights, unbiased passes, other knobs, orbit
    (64, 48, 1, dict(), False, False, (), False),
    (64, 48, 1, dict(), False, False, (), True),
    (37, 29, 1, dict(), False, False, (), False),
    (37, 29, 1, dict(), False, False, (), True),
    (8, 8, 1, dict(), False, False, (), False),
    (8, 8, 0, dict(), False, False, (), True),
    (37, 29, 0, dict(), False, False, (), False),  # rt_tuning 25 = 0: raycast, then candidates + temporal with the work-sharing walk
    (37, 29, 0, dict(), False, False, (), True),
    (37, 29, 0, dict(), False, False, ((13, 0),), True),  # the fused kernel without the work-sharing walk
    (37, 29, 1, dict(use_shadowed_target_function=1), False, False, (), False),
    (37, 29, 1, dict(use_shadowed_target_function=1), False, False, (), True),
    (37, 29, 1, dict(), True, False, (), True),  # power light sampling: one-launch stage 0 ...
    (37, 29, 0, dict(), True, False, (), False),  # ... candidates + temporal
    (37, 29, 0, dict(), True, False, ((13, 0),), False),
    (37, 29, 1, dict(use_shadowed_target_function=1), True, False, (), True),
    (37, 29, 1, dict(), False, True, (), True),  # rt_spatial_unbiased
]


@pytest.mark.parametrize("W,H,one_launch,kw,power,unbiased,knobs,orbit", FRAME_CASES)
def test_frames_with_a_moving_box_equal_the_cpu_sequence(api, oracle, worlds, W, H, one_launch, kw, power, unbiased, knobs, orbit):
    stats, want, elsewhere = _run_frames(api, oracle, worlds, W, H, one_launch, kw, power, unbiased, knobs, orbit)
    # frame 1 merges an untagged history; the four others are motion launches
    assert stats == want and want["valid"] > 0 and elsewhere > 0, (stats, want, elsewhere)


# -------------------------------------------------------------------------------------------------------------- host rules
@pytest.mark.parametrize("orbit", [False, True])
def test_toggle_off_is_the_reprojection_alone(api, oracle, worlds, orbit):
    stats, _, _ = _run_frames(api, oracle, worlds, 37, 29, 1, dict(), False, False, (), orbit, follow=False)
    assert stats == dict(merged=0, in_range=0, valid=0)


def test_toggle_without_reprojection_changes_nothing(api, oracle, worlds):
    """rt_temporal_motion on, rt_temporal_reprojection off: the same-pixel merge of the reference, no motion launch"""
    W, H = 37, 29
    opt = oracle.bench_options()
    ws = _frame_worlds(worlds)
    r = _renderer(api, ws[0]["tris"], W, H, opt, reproject=False, motion=True)
    view = worlds.view(ws[0], W, H)
    _look(r, view)
    r.walk_stats_enable(True)
    st = oracle.new_state(W, H)
    for k, w in enumerate(ws[:3]):
        if k:
            _update_box(r, w)
        view = worlds.view(w, W, H)
        out = r.frame(1 + k)
        w["scene"].frame(W, H, 1 + k, view.rg, view.eye, opt, st)
        acc = r.download(api.RT_BUF_ACCUMULATION)
        assert _eq_bits(acc, st["accum"].reshape(acc.shape)), f"frame {1 + k}"
    assert r.temporal_motion_stats() == dict(merged=0, in_range=0, valid=0)
    r.close()


def test_getters_epoch_tags_and_scene_set(api, oracle, worlds):
    W, H = 37, 29
    opt = oracle.bench_options()
    wa, wb = worlds.of(worlds.base), worlds.moved(MOVES[0])
    r = _renderer(api, wa["tris"], W, H, opt, motion=None)
    assert r.temporal_motion() is False
    e0 = _epoch(r)
    assert r.temporal_motion(True) is True and _epoch(r) != e0
    e1 = _epoch(r)
    assert r.temporal_motion(False) is False and _epoch(r) != e1
    assert r.temporal_motion(True) is True
    for res in (api.RT_RES_0, api.RT_RES_1, api.RT_RES_TEMPORAL):
        assert r.reservoir_scene(res) is None
    assert r.L.rt_reservoir_scene(r.h, api.RT_RES_0, None, None, None) == RT_ERR_ARG
    assert r.L.rt_temporal_motion_range(r.h, None, None, None) == RT_ERR_ARG
    assert r.temporal_motion_range() == dict(lo=0, hi=0, generation=0)
    a = worlds.view(wa, W, H)
    _look(r, a)
    r.raycast()
    r.generate_candidate(1, api.RT_RES_0)
    r.save_temporal_reservoir(api.RT_RES_0, api.RT_RES_TEMPORAL)
    assert r.reservoir_scene(api.RT_RES_TEMPORAL)[0] == 0 and _eq_bits(r.reservoir_scene(api.RT_RES_TEMPORAL)[1], a.eye)
    _update_box(r, wb)
    assert r.temporal_motion_range() == dict(lo=BOX_LO, hi=BOX_HI, generation=0)
    r.raycast()
    r.generate_candidate(2, api.RT_RES_1)
    assert r.reservoir_scene(api.RT_RES_1)[0] == 1 and r.reservoir_scene(api.RT_RES_TEMPORAL)[0] == 0
    # the toggle touches no reservoir buffer and no tag; off and on again, no earlier update is followed
    before = r.download(api.RT_BUF_RES_TEMPORAL).copy()
    r.temporal_motion(False)
    r.temporal_motion(True)
    assert _eq_bits(r.download(api.RT_BUF_RES_TEMPORAL), before) and r.reservoir_scene(api.RT_RES_TEMPORAL)[0] == 0
    assert r.temporal_motion_range() == dict(lo=0, hi=0, generation=1)
    r.set_scene(wa["tris"])
    for res in (api.RT_RES_0, api.RT_RES_1, api.RT_RES_TEMPORAL):
        assert r.reservoir_scene(res) is None, "rt_scene_set clears the tags"
    assert r.temporal_motion_range() == dict(lo=0, hi=0, generation=0), "... and the range"
    r.close()
    # a strip context holds only its own rows of the history
    s = api.Renderer(W, H, rows=(8, 20), halo=4)
    assert s.L.rt_temporal_motion(s.h, 1) == RT_ERR_UNSUPPORTED
    assert s.L.rt_temporal_motion(s.h, 0) == RT_ERR_UNSUPPORTED
    assert s.temporal_motion() is False
    s.close()


def _two_step(api, oracle, worlds, W, H, write_between):
    """a history of generation 0, then two updates of the box's halves (each by MOVES[0]); with write_between a reservoir buffer is
    written between them, which makes the history one generation too old"""
    opt = oracle.bench_options()
    wa = worlds.of(worlds.base)
    half = worlds.of(move(worlds.base, MOVES[0], first=BOX_LO, count=6))
    wb = worlds.moved(MOVES[0])
    prev, cur = worlds.view(wa, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT)), worlds.view(wb, W, H)
    hist = _history(oracle, wa, prev, opt)
    r = _renderer(api, wa["tris"], W, H, opt)
    _look(r, prev)
    r.raycast()
    r.upload(api.RT_BUF_RES_TEMPORAL, hist)
    _update_box(r, half, BOX_LO, 6)
    if write_between:
        r.raycast()
        r.generate_candidate(3, api.RT_RES_1)
    _update_box(r, wb, BOX_LO + 6, 6)
    rng = r.temporal_motion_range()
    _look(r, cur)
    r.raycast()
    assert _eq_bits(r.download(api.RT_BUF_VISIBILITY), cur.vis)
    r.generate_candidate(7, api.RT_RES_0)
    cand = wb["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
    r.walk_stats_enable(True)
    r.temporal_resampling(7, api.RT_RES_TEMPORAL, api.RT_RES_0)
    got, stats = r.download(api.RT_BUF_RES_0), r.temporal_motion_stats()
    r.close()
    return wa, wb, prev, cur, opt, hist, cand, got, stats, rng


@pytest.mark.parametrize("W,H", [(37, 29), (8, 8)])
def test_two_updates_between_two_frames_are_both_followed(api, oracle, worlds, W, H):
    wa, wb, prev, cur, opt, hist, cand, got, stats, rng = _two_step(api, oracle, worlds, W, H, False)
    assert rng == dict(lo=BOX_LO, hi=BOX_HI, generation=0)
    want, diag = tm.temporal(W, H, 7, wb["tris"], wa["tris"], cur.vis, prev.vis, cur.eye, prev.eye, prev.rg, cur.rg, BOX_LO, BOX_HI, opt, hist, cand.copy())
    assert not _res_diff(got, want, cur.shaded) and stats == _counts(cur, diag) and stats["valid"] > 0


@pytest.mark.parametrize("W,H", [(37, 29), (8, 8)])
def test_a_history_one_generation_too_old_gets_the_cameras_only(api, oracle, worlds, W, H):
    wa, wb, prev, cur, opt, hist, cand, got, stats, rng = _two_step(api, oracle, worlds, W, H, True)
    assert rng == dict(lo=BOX_LO + 6, hi=BOX_HI, generation=1)
    want, _ = tr.temporal(W, H, 7, wb["tris"], cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, cand.copy())
    assert not _res_diff(got, want, cur.shaded) and stats == dict(merged=0, in_range=0, valid=0)


def test_trace_closest_after_updates_equals_a_fresh_scene(api, oracle, worlds):
    W, H = 37, 29
    ws = _frame_worlds(worlds)
    r = _renderer(api, ws[0]["tris"], W, H, oracle.bench_options())
    _look(r, worlds.view(ws[0], W, H))
    for k, w in enumerate(ws):
        if k:
            _update_box(r, w)
        r.frame(1 + k)
    rng = np.random.default_rng(24)
    rays = np.zeros((4096, 8), np.float32)
    rays[:, 0:3] = rng.random((4096, 3), dtype=np.float32) * np.float32(8.0) - np.float32(4.0)
    rays[:, 3:6] = rng.random((4096, 3), dtype=np.float32) * 2 - 1
    rays[:, 7] = 3.402823466e38
    fresh = api.Renderer(W, H)
    fresh.set_scene(ws[-1]["tris"])
    a, b = r.trace_closest(rays), fresh.trace_closest(rays)
    assert (a[:, 3].view(np.int32) >= 0).sum() > 1000
    assert _eq_bits(a, b)
    r.close()
    fresh.close()


@pytest.mark.parametrize("key", [11, 12])
def test_experiment_stage0_forms_refuse_a_motion_launch(api, oracle, worlds, key):
    """[exp] rt_tuning 11 / 12 gather their history from the own pixel only: fine until the scene moves, RT_ERR_UNSUPPORTED from the frame
    after the update (the camera stands still: it is the motion launch that is refused)"""
    W, H = 37, 29
    ws = _frame_worlds(worlds)
    r = _renderer(api, ws[0]["tris"], W, H, oracle.bench_options(), exp=True)
    r.tuning(key, 1)
    _look(r, worlds.view(ws[0], W, H))
    r.frame(1)
    r.frame(2)
    _update_box(r, ws[1])
    out = C.c_int(-1)
    assert r.L.rt_frame(r.h, 3, 0, C.byref(out)) == RT_ERR_UNSUPPORTED
    r.close()


def test_restir_app_move_tris_follow_motion_equals_the_renderer(tmp_path, api, worlds):
    """restir_app --move-tris --reproject --follow-motion: the same RGBA8 bytes as the Renderer with both toggles on, driven through
    update_scene with scenes.move_triangles (the same float32 add on both sides)"""
    import os
    import subprocess

    from cedec_2024_rt_amd.types import bench_options

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    A = worlds.base
    path, out = os.path.join(str(tmp_path), "room.tris"), os.path.join(str(tmp_path), "out.raw")
    A.tofile(path)
    W, H, d = 96, 64, (0.0, 0.0, 0.5)
    cmd = [os.path.join(root, "app", "restir_app"), "--example", "10", "--tris", path, "--size", str(W), str(H), "--eye", *map(str, ls.LAMP_EYE),
           "--lookat", *map(str, ls.LAMP_AT), "--frames", "4", "--move-tris", str(BOX_LO), str(BOX_HI - BOX_LO), *map(str, d), "--reproject",
           "--follow-motion", "--rgba", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("scene update:") == 3, p.stdout
    app_px = np.fromfile(out, np.uint8).reshape(H, W, 4)
    r = _renderer(api, A, W, H, bench_options())
    r.lookat(ls.LAMP_EYE, ls.LAMP_AT)
    r.clear()
    r.walk_stats_enable(True)
    cur = A
    for frame in range(1, 5):
        if frame >= 2:
            cur = move(cur, d)
            r.update_scene(cur[BOX_LO:BOX_HI], BOX_LO)
        r.frame(frame)
    assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), app_px)
    assert r.temporal_motion_stats()["valid"] > 0
    # and the toggle is what makes these bytes
    off = _renderer(api, A, W, H, bench_options(), motion=False)
    off.lookat(ls.LAMP_EYE, ls.LAMP_AT)
    off.clear()
    cur = A
    for frame in range(1, 5):
        if frame >= 2:
            cur = move(cur, d)
            off.update_scene(cur[BOX_LO:BOX_HI], BOX_LO)
        off.frame(frame)
    assert not np.array_equal(off.download(api.RT_BUF_PIXELS).reshape(H, W, 4), app_px)
    r.close()
    off.close()
