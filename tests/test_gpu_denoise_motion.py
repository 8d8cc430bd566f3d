"""rt_denoise_temporal_motion on the device: k_denoise_temporal_motion and the host's bookkeeping against tests/denoise_motion_ref.py
(the restatement compiled from the kernels' own headers, anchored by tests/test_denoise_motion_cpu.py), bit for bit.

Sizes: 8 x 8 (one wavefront), 19 x 7, 37 x 29 and 40 x 33 (partial tiles, more than one block). Scene: the lamp room of
tests/light_sampling_ref.py; its box (triangles 64-75) moves before every call. The input of every call is a ReSTIR frame rendered on
the device at accumulate = 0; the restatement gets the accumulation, the guide hits and the camera the call saw."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_motion_ref as dm
import denoise_temporal_ref as dtr
import light_sampling_ref as ls
from test_temporal_motion_cpu import BOX_HI, BOX_LO, MOVES, move
from test_temporal_reproject_cpu import FOVY, _orbit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "app", "restir_app")
RT_OK, RT_ERR_UNSUPPORTED = 0, 5
SIZES = [(8, 8), (19, 7), (37, 29), (40, 33)]
ORBIT = 0.1
STEP = (0.0, 0.0, 0.25)  # per call: the box comes forward


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def base():
    return ls.make_lamp_room()


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _ndiff(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1, 4).view(np.uint32), np.ascontiguousarray(b).reshape(-1, 4).view(np.uint32)
    return int((a != b).any(axis=1).sum())


def _renderer(api, tris, W, H, on=None, layout=None, **kw):
    from cedec_2024_rt_amd.types import bench_options

    r = api.Renderer(W, H, **kw)
    r.set_scene(tris)
    r.lookat(ls.LAMP_EYE, ls.LAMP_AT, fovy=FOVY)
    r.set_options(bench_options(accumulate=0))
    if layout is not None:
        r.tuning(api.Tune.DN_LAYOUT, layout)
    if on is not None:
        assert r.denoise_temporal_motion(on)["on"] is bool(on)
    return r


def _box(r, tris, first=BOX_LO, count=BOX_HI - BOX_LO):
    r.update_scene(tris[first:first + count], first=first)


def _call(api, r, ref, params, what=""):
    """one rt_denoise_temporal call and the restatement's on the same input; DENOISED, DENOISE_HISTORY and PIXELS bit for bit"""
    r.sync()
    acc = r.download(api.RT_BUF_ACCUMULATION)
    hdr = r.denoise_temporal(hdr=True, **params).reshape(-1, 4).copy()
    mom, px = r.download(api.RT_BUF_DENOISE_HISTORY), r.download(api.RT_BUF_PIXELS)
    vis, eye, rg = r.download(api.RT_BUF_DENOISE_GUIDE), r.camera_pose()[0], r.raygen()
    want = ref(vis, eye, rg, acc) if callable(ref) else ref
    assert _eq_bits(hdr, want[0]), f"{what}: {_ndiff(hdr, want[0])} pixels differ from the restatement"
    assert _eq_bits(mom, want[1]), f"{what}: {_ndiff(mom, want[1])} history records differ from the restatement"
    r.upload(api.RT_BUF_ACCUMULATION, want[0])
    r.tone_mapping()
    assert _eq_bits(r.download(api.RT_BUF_PIXELS), px), f"{what}: the pixels are not the tone-mapped image"
    r.upload(api.RT_BUF_ACCUMULATION, acc)
    return want, mom


def _moving_box(api, base, W, H, calls, orbit, on, iterations, layouts=(0, 1), step=STEP, ref_cls=None):
    """`calls` calls, the box moved by `step` (and the camera turned) before each from the second on, one context per layout and one
    restatement for both; returns the history lengths per call and the restatement"""
    params = dict(iterations=iterations)
    rs = [_renderer(api, base, W, H, on=on, layout=lay) for lay in layouts]
    ref = dm.MotionRef(W, H, base, on=on, **params) if ref_cls is None else ref_cls(W, H, base, **params)
    t = base
    hs = []
    for j in range(1, calls + 1):
        if j >= 2:
            t = move(t, step)
            if ref_cls is None:
                ref.update(t[BOX_LO:BOX_HI], BOX_LO)
            else:
                ref.tris = dm._bytes(t)
        want = None
        for lay, r in zip(layouts, rs):
            if j >= 2:
                _box(r, t)
                if orbit:
                    r.lookat(*_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT * (j - 1)), fovy=FOVY)
            r.frame(j)
            want, mom = _call(api, r, ref if want is None else want, params, f"{W} x {H} call {j} layout {lay} {iterations} iterations")
            if ref_cls is None:
                assert r.denoise_temporal_motion()["followed"] == ref.followed == (on and j >= 2)
        hs.append(mom[:, 2].copy())
    for r in rs:
        r.close()
    return hs, ref


# ------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("orbit", [False, True])
def test_moving_box_equals_the_restatement(api, base, W, H, orbit):
    for iterations in (0, 1, 2):
        hs, ref = _moving_box(api, base, W, H, 5 if iterations else 4, orbit, True, iterations)
        on_range = ref.diag[:, 0] == 1
        assert on_range.any(), "no participating box pixel"
        assert hs[-1][on_range].max() == len(hs), "no box pixel kept its history through every call"


def test_history_length_reaches_the_cap(api, base):
    """36 calls with the box moving every call (there and back, so that it stays in view): h passes 4, where the temporal variance
    takes over, and stops at 32 on followed pixels"""
    W, H, calls = 19, 7, 36
    params = dict(iterations=1)
    r = _renderer(api, base, W, H, on=True)
    ref = dm.MotionRef(W, H, base, on=True, **params)
    t = base
    for j in range(1, calls + 1):
        if j >= 2:
            t = move(t, (0.0, 0.0, 0.125 if (j // 4) % 2 == 0 else -0.125))
            ref.update(t[BOX_LO:BOX_HI], BOX_LO)
            _box(r, t)
        r.frame(j)
        _, mom = _call(api, r, ref, params, f"call {j}")
        assert r.denoise_temporal_motion()["followed"] == (j >= 2)
        on_range = ref.diag[:, 0] == 1
        if j >= 2:
            assert on_range.any() and mom[on_range, 2].max() == min(j, 32)
    r.close()


@pytest.mark.parametrize("W,H", [(37, 29), (8, 8)])
def test_toggle_off_is_the_parents_call(api, base, W, H):
    hs, _ = _moving_box(api, base, W, H, 4, True, False, 2, ref_cls=dtr.TemporalRef)
    assert hs[-1].max() == 4.0


def _epoch(r):
    e = C.c_uint64()
    assert r.L.rt_state_epoch(r.h, C.byref(e)) == RT_OK
    return e.value


def test_toggling_changes_no_frame_state(api, base):
    """neither rt_state_epoch nor any reservoir or accumulation byte of the following frame"""
    W, H = 37, 29
    bufs = (api.RT_BUF_ACCUMULATION, api.RT_BUF_RES_0, api.RT_BUF_RES_1, api.RT_BUF_RES_TEMPORAL)
    a, b = _renderer(api, base, W, H), _renderer(api, base, W, H)
    t = base
    for f in range(1, 5):
        if f >= 2:
            t = move(t, STEP)
            _box(a, t), _box(b, t)
        e = _epoch(b)
        b.denoise_temporal_motion(f % 2 == 0)
        assert _epoch(b) == e
        a.frame(f), b.frame(f)
        a.sync(), b.sync()
        assert _epoch(a) == _epoch(b)
        for k in bufs:
            assert _eq_bits(a.download(k), b.download(k)), (f, k)
        a.denoise_temporal(), b.denoise_temporal()
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------ host rules
def test_host_rules(api, base):
    W, H = 19, 7
    n = len(base)
    r = _renderer(api, base, W, H, on=True)
    ref = dm.MotionRef(W, H, base, on=True, iterations=1)
    p = dict(iterations=1)
    ts = [base]
    for _ in range(8):
        ts.append(move(ts[-1], STEP))

    def check(followed, what, **rng):
        assert r.denoise_temporal_motion() == dict(on=True, followed=followed) and ref.followed == followed, what
        if rng:
            assert r.temporal_motion_range() == ref.range() == rng, what

    assert r.temporal_motion_range() == dict(lo=0, hi=0, generation=0)
    # the first call after a reset, and after an update with no history
    _box(r, ts[1]), ref.update(ts[1][BOX_LO:BOX_HI], BOX_LO)
    r.frame(1)
    _call(api, r, ref, p, "first call")
    check(False, "first call", lo=BOX_LO, hi=BOX_HI, generation=0)
    # re-basing after a denoise call; a frame in between changes nothing (only this toggle is on)
    _box(r, ts[2]), ref.update(ts[2][BOX_LO:BOX_HI], BOX_LO)
    check(False, "re-based", lo=BOX_LO, hi=BOX_HI, generation=1)
    r.frame(2), ref.frame()
    _call(api, r, ref, p, "second call")
    check(True, "second call")
    # the range growing over two updates of two spans, with a frame between them
    half = ts[2].copy()
    half[64:70] = ts[3][64:70]
    r.update_scene(half[64:70], first=64), ref.update(half[64:70], 64)
    check(True, "first span", lo=64, hi=70, generation=2)
    r.frame(3), ref.frame()
    r.update_scene(ts[3][70:76], first=70), ref.update(ts[3][70:76], 70)
    check(True, "second span", lo=64, hi=76, generation=2)
    r.frame(4)
    _call(api, r, ref, p, "two spans")
    check(True, "two spans")
    # rt_denoise_temporal_reset: the next call has no history to follow
    _box(r, ts[4]), ref.update(ts[4][BOX_LO:BOX_HI], BOX_LO)
    r.denoise_temporal_reset(), ref.reset()
    r.frame(5)
    _call(api, r, ref, p, "after a reset")
    check(False, "after a reset")
    # toggle off then on: an empty range of the current generation, and updates from here on are followed
    r.denoise_temporal_motion(False), ref.toggle(False)
    assert r.temporal_motion_range() == ref.range() == dict(lo=0, hi=0, generation=5)
    _box(r, ts[5]), ref.update(ts[5][BOX_LO:BOX_HI], BOX_LO)
    assert r.temporal_motion_range() == dict(lo=0, hi=0, generation=5)  # no kept vertices: nothing is tracked
    r.denoise_temporal_motion(True), ref.toggle(True)
    check(False, "on again", lo=0, hi=0, generation=6)
    r.frame(6)
    _call(api, r, ref, p, "not followed: the update came before the toggle")
    check(False, "update before the toggle")
    _box(r, ts[6]), ref.update(ts[6][BOX_LO:BOX_HI], BOX_LO)
    r.frame(7)
    _call(api, r, ref, p, "followed again")
    check(True, "followed again", lo=BOX_LO, hi=BOX_HI, generation=6)
    # rt_scene_set: generations from 0, no history
    r.set_scene(ts[6]), ref.set_scene(ts[6])
    assert r.temporal_motion_range() == ref.range() == dict(lo=0, hi=0, generation=0)
    _box(r, ts[7]), ref.update(ts[7][BOX_LO:BOX_HI], BOX_LO)
    r.frame(8)
    _call(api, r, ref, p, "first call after rt_scene_set")
    check(False, "first call after rt_scene_set")
    _box(r, ts[8]), ref.update(ts[8][BOX_LO:BOX_HI], BOX_LO)
    r.frame(9)
    _call(api, r, ref, p, "second call after rt_scene_set")
    check(True, "second call after rt_scene_set", lo=BOX_LO, hi=BOX_HI, generation=1)
    assert n == len(ts[8])
    r.close()


def test_both_toggles_share_the_kept_vertices(api, base):
    """frame / update / denoise / update / frame / update / denoise with rt_temporal_motion on as well: the consumer whose history is
    not of the kept generation gets the camera only; and the buffer survives this toggle going off while the other stays on"""
    W, H = 37, 29
    p = dict(iterations=1)
    r = _renderer(api, base, W, H, on=True)
    assert r.temporal_reprojection(True) is True and r.temporal_motion(True) is True
    ref = dm.MotionRef(W, H, base, on=True, motion=True, **p)
    ts = [base]
    for _ in range(5):
        ts.append(move(ts[-1], STEP))

    def upd(k):
        _box(r, ts[k]), ref.update(ts[k][BOX_LO:BOX_HI], BOX_LO)
        assert r.temporal_motion_range() == ref.range(), k

    r.frame(1), ref.frame()
    _call(api, r, ref, p, "call 1")
    upd(1)
    _call(api, r, ref, p, "call 2")  # no new frame: the same accumulation, a moved guide
    assert r.denoise_temporal_motion()["followed"] and ref.followed
    upd(2)
    assert ref.range()["generation"] == 1
    r.walk_stats_enable(True)
    r.frame(2), ref.frame()
    # the reservoir history is of generation 0, the kept vertices of generation 1: no motion launch
    assert r.temporal_motion_stats()["merged"] == 0
    r.walk_stats_enable(False)
    upd(3)
    assert ref.range()["generation"] == 2
    _call(api, r, ref, p, "call 3")
    assert not r.denoise_temporal_motion()["followed"] and not ref.followed
    # off while rt_temporal_motion stays on: the range is kept and keeps growing by r24's rule
    before = r.temporal_motion_range()
    r.denoise_temporal_motion(False), ref.toggle(False)
    assert r.temporal_motion_range() == before == ref.range()
    upd(4)
    r.denoise_temporal_motion(True), ref.toggle(True)
    assert r.temporal_motion_range() == ref.range()
    r.frame(3), ref.frame()
    _call(api, r, ref, p, "call 4")
    upd(5)
    r.frame(4), ref.frame()
    _call(api, r, ref, p, "call 5")
    assert r.denoise_temporal_motion()["followed"] and ref.followed
    # rt_temporal_motion off while this toggle stays on: likewise
    before = r.temporal_motion_range()
    r.temporal_motion(False), ref.toggle_motion(False)
    assert r.temporal_motion_range() == before == ref.range()
    r.denoise_temporal_motion(False), ref.toggle(False)
    assert r.temporal_motion_range()["lo"] == r.temporal_motion_range()["hi"] == 0
    r.close()


def test_a_strip_context_refuses_the_toggle(api, base):
    W, H = 37, 29
    s = api.Renderer(W, H, rows=(0, H // 2), halo=8)
    s.set_scene(base)
    assert s.L.rt_denoise_temporal_motion(s.h, 1) == RT_ERR_UNSUPPORTED
    on = C.c_int(7)
    assert s.L.rt_denoise_temporal_motion_get(s.h, C.byref(on), None) == RT_OK and on.value == 0
    s.close()


# ------------------------------------------------------------------------------------------------------------ restir_app
def test_restir_app_denoise_follow_motion_equals_the_renderer(tmp_path, api, base):
    from cedec_2024_rt_amd.types import bench_options

    W, H, frames = 40, 33, 4
    path, out = os.path.join(str(tmp_path), "lamp.tris"), os.path.join(str(tmp_path), "out.raw")
    base.tofile(path)
    cmd = [APP, "--tris", path, "--size", str(W), str(H), "--eye", *map(str, ls.LAMP_EYE), "--lookat", *map(str, ls.LAMP_AT), "--accumulate", "0",
           "--frames", str(frames), "--denoise", "2", "--denoise-temporal", "--move-tris", str(BOX_LO), str(BOX_HI - BOX_LO), *map(str, STEP),
           "--denoise-follow-motion", "--rgba", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("followed moved geometry") == frames - 1 and p.stdout.count("camera only") == 1, p.stdout
    app_px = np.fromfile(out, np.uint8).reshape(H, W, 4)
    r = api.Renderer(W, H)
    r.set_scene(base)
    r.lookat(ls.LAMP_EYE, ls.LAMP_AT)
    r.set_options(bench_options(accumulate=0))
    r.denoise_temporal_motion(True)
    r.clear()
    t = base
    for f in range(1, frames + 1):
        if f >= 2:
            t = move(t, STEP)
            _box(r, t)
        r.frame(f)
        px = r.denoise_temporal(iterations=2)
    assert r.denoise_temporal_motion()["followed"]
    r.close()
    assert np.array_equal(app_px, px), f"{int((app_px != px).any(axis=2).sum())} pixels differ"
    p = subprocess.run([APP, "--tris", path, "--denoise", "2", "--denoise-follow-motion"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--denoise-follow-motion needs" in p.stderr, p.stdout + p.stderr
