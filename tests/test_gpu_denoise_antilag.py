"""rt_denoise_temporal_antilag on the device: k_denoise_antilag_gather and k_denoise_antilag and the host's rules against
tests/denoise_antilag_ref.py (the restatement compiled from the kernels' own headers, anchored by tests/test_denoise_antilag_cpu.py),
bit for bit after every call: RT_BUF_DENOISED, all four components of RT_BUF_DENOISE_HISTORY, RT_BUF_PIXELS.

Sizes: 1 x 1, 8 x 8, 19 x 7, 3 x 70 (thinner than the window), 37 x 29 and 40 x 33 (no multiples of the tile: the LDS halo crosses tile
seams and image edges), and 70 x 19: the tile is 32 x 8, so the issue's two sizes have four and five tiles down and two across, and
this one three each way. Scene: the lamp room of tests/light_sampling_ref.py; its box (triangles 64-75)
moves before every call. The input of every call is a ReSTIR frame rendered on the device at accumulate = 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_antilag_ref as da
import denoise_motion_ref as dm
import light_sampling_ref as ls
from test_gpu_denoise_motion import APP, ORBIT, STEP, _box, _call, _eq_bits, _epoch, _renderer
from test_temporal_motion_cpu import BOX_HI, BOX_LO, move
from test_temporal_reproject_cpu import FOVY, _orbit

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_ARG, RT_ERR_STATE, RT_ERR_UNSUPPORTED = 0, 1, 3, 5
SIZES = [(1, 1), (8, 8), (19, 7), (3, 70), (37, 29), (40, 33), (70, 19)]
# (iterations, radius, follow-motion): every radius, 0 / 1 / 2 iterations, follow-motion off and on (the orbit cases swap the last)
COMBOS = [(0, 1, True), (1, 2, False), (2, 3, True), (1, 4, True), (0, 4, False)]


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def base():
    return ls.make_lamp_room()


def _antilag(r, on=True, **al):
    s = r.denoise_temporal_antilag(on, **al)
    assert s["on"] is bool(on) and all(s[k] == np.float32(v) for k, v in al.items())
    return s


def _sequence(api, base, W, H, calls, orbit, follow, iterations, al, layouts=(0, 1), step=STEP):
    """`calls` calls, the box moved by `step` (and the camera turned) before each from the second on; one context per a-trous layout and
    one restatement for both. Returns the moments of the last call and the restatement."""
    params = dict(iterations=iterations)
    rs = [_renderer(api, base, W, H, on=follow, layout=lay) for lay in layouts]
    for r in rs:
        _antilag(r, True, **al)
    ref = da.AntilagRef(W, H, base, on=follow, antilag=True, al=al, **params)
    t = base
    for j in range(1, calls + 1):
        if j >= 2:
            t = move(t, step)
            ref.update(t[BOX_LO:BOX_HI], BOX_LO)
        want = None
        for lay, r in zip(layouts, rs):
            if j >= 2:
                _box(r, t)
                if orbit:
                    r.lookat(*_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT * (j - 1)), fovy=FOVY)
            r.frame(j)
            want, mom = _call(api, r, ref if want is None else want, params, f"{W} x {H} call {j} layout {lay} {iterations} iterations {al}")
            s = r.denoise_temporal_antilag()
            assert s["adapted"] == ref.adapted == (j >= 2) and r.denoise_temporal_motion()["followed"] == ref.followed == (follow and j >= 2)
    for r in rs:
        r.close()
    return mom, ref


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("orbit", [False, True])
def test_moving_box_equals_the_restatement(api, base, W, H, orbit):
    """This test fails without the feature: the parent has no toggle."""
    responded = 0
    for iterations, radius, follow in COMBOS:
        mom, ref = _sequence(api, base, W, H, 4, orbit, follow != orbit, iterations, dict(radius=radius))
        assert (mom[:, 3] >= 0.0).all() and (mom[:, 3] <= 1.0).all() and (mom[mom[:, 2] <= 1.0, 3] == 0.0).all()
        responded += int((mom[:, 3] > 0.0).sum())
    if W * H >= 64:
        assert responded > 0, "no pixel of any case responded: the comparison shows nothing about lambda'"


def test_static_run_to_the_cap(api, base):
    """36 calls of a static scene: h passes 4, where the temporal variance takes over, and stops at 32; every call from the second on
    is an adapted call"""
    W, H, calls = 19, 7, 36
    params = dict(iterations=1)
    r = _renderer(api, base, W, H)
    _antilag(r, True)
    ref = da.AntilagRef(W, H, base, antilag=True, **params)
    for j in range(1, calls + 1):
        r.frame(j)
        _, mom = _call(api, r, ref, params, f"call {j}")
        assert r.denoise_temporal_antilag()["adapted"] == (j >= 2)
        assert mom[:, 2].max() == min(j, 32)
    r.close()


# ------------------------------------------------------------------------------------------------------------ host rules
def test_toggle_off_and_the_first_call_after_a_reset_are_the_parents_call(api, base):
    """not adapted, and the bytes of tests/denoise_motion_ref.py, which knows no anti-lag"""
    W, H = 37, 29
    p = dict(iterations=2)
    r = _renderer(api, base, W, H)
    ref = dm.MotionRef(W, H, base, **p)
    assert r.denoise_temporal_antilag() == dict(on=False, adapted=False, radius=4, gradient_lo=float(np.float32(0.2)),
                                                gradient_hi=float(np.float32(0.8)), floor=float(np.float32(0.05)))
    for j in (1, 2, 3):
        r.frame(j)
        _, mom = _call(api, r, ref, p, f"toggle off, call {j}")
        assert not r.denoise_temporal_antilag()["adapted"] and (mom[:, 3] == 0.0).all()
    # on: no reset needed, the next call reads the history the calls above wrote (a ramp steep enough that this static scene's noise
    # makes pixels respond: the comparison is then about lambda' too)
    al = dict(gradient_lo=0.02, gradient_hi=0.3, floor=0.0)
    _antilag(r, True, **al)
    aref = da.AntilagRef(W, H, base, antilag=True, al=al, **p)
    aref.gx, aref.gn, aref.hcol, aref.hmom, aref.rg, aref.has = ref.gx, ref.gn, ref.hcol, ref.hmom, ref.rg, ref.has
    r.frame(4)
    _, mom = _call(api, r, aref, p, "toggle on, call 4")
    assert r.denoise_temporal_antilag()["adapted"] and aref.adapted and (mom[:, 3] > 0.0).any()
    # the first call after a reset has no history: the parent's kernels, not adapted
    r.denoise_temporal_reset(), ref.reset()
    r.frame(5)
    _, mom = _call(api, r, ref, p, "first call after a reset")
    s = r.denoise_temporal_antilag()
    assert s["on"] and not s["adapted"] and (mom[:, 3] == 0.0).all()
    r.close()


def test_toggling_changes_no_frame_state(api, base):
    """neither rt_state_epoch nor any reservoir or accumulation byte of the following frame"""
    W, H = 37, 29
    bufs = (api.RT_BUF_ACCUMULATION, api.RT_BUF_RES_0, api.RT_BUF_RES_1, api.RT_BUF_RES_TEMPORAL)
    a, b = _renderer(api, base, W, H), _renderer(api, base, W, H)
    for f in range(1, 5):
        e = _epoch(b)
        b.denoise_temporal_antilag(f % 2 == 0, radius=1 + f % 4)
        assert _epoch(b) == e
        a.frame(f), b.frame(f)
        a.sync(), b.sync()
        assert _epoch(a) == _epoch(b)
        for k in bufs:
            assert _eq_bits(a.download(k), b.download(k)), (f, k)
        a.denoise_temporal(), b.denoise_temporal()
        assert b.denoise_temporal_antilag()["adapted"] == (f % 2 == 0 and f >= 2)
    a.close(), b.close()


def test_error_codes(api, base):
    W, H = 19, 7
    r = _renderer(api, base, W, H)
    L, P = r.L, api._AntilagParams
    before = _antilag(r, True, radius=2, gradient_lo=0.25, gradient_hi=0.75, floor=0.05)
    nan, inf = float("nan"), float("inf")
    bad = [(0, 0.2, 0.8, 0.1), (5, 0.2, 0.8, 0.1), (-1, 0.2, 0.8, 0.1), (3, -0.1, 0.8, 0.1), (3, 0.8, 0.8, 0.1), (3, 0.9, 0.8, 0.1),
           (3, nan, 0.8, 0.1), (3, 0.2, nan, 0.1), (3, 0.2, inf, 0.1), (3, inf, inf, 0.1), (3, 0.2, 0.8, -0.1), (3, 0.2, 0.8, nan), (3, 0.2, 0.8, inf)]
    for q in bad:
        p = P(*q)
        assert L.rt_denoise_temporal_antilag(r.h, 0, C.byref(p)) == RT_ERR_ARG, q
        assert L.rt_last_error(r.h)
        assert r.denoise_temporal_antilag() == before, q  # a refused call changes nothing, the toggle included
    for q in ((1, 0.0, 1e-30, 0.0), (4, 0.0, 3e38, 3e38)):  # the borders that are allowed
        assert L.rt_denoise_temporal_antilag(r.h, 1, C.byref(P(*q))) == RT_OK, q
    assert L.rt_denoise_temporal_antilag(r.h, 1, None) == RT_OK  # NULL = defaults
    assert r.denoise_temporal_antilag()["radius"] == 4
    assert L.rt_denoise_temporal_antilag_get(r.h, None, None, None) == RT_ERR_ARG
    ms = C.c_float()
    assert L.rt_denoise_temporal_antilag_timing(r.h, None) == RT_ERR_ARG
    assert L.rt_denoise_temporal_antilag_timing(r.h, C.byref(ms)) == RT_ERR_STATE  # no timed call yet
    # timing: the first call is not adapted (RT_ERR_STATE), the second is, and ms[1] of rt_denoise_temporal_timing covers it
    assert L.rt_timing_enable(r.h, 1) == RT_OK
    r.frame(1)
    r.denoise_temporal(iterations=1)
    assert L.rt_denoise_temporal_antilag_timing(r.h, C.byref(ms)) == RT_ERR_STATE
    r.frame(2)
    r.denoise_temporal(iterations=1)
    assert L.rt_denoise_temporal_antilag_timing(r.h, C.byref(ms)) == RT_OK
    six = (C.c_float * 6)()
    assert L.rt_denoise_temporal_timing(r.h, six) == RT_OK
    assert 0.0 <= ms.value <= six[1] and abs(sum(six[:5]) - six[5]) <= 0.05 * six[5] + 0.01
    with pytest.raises(api.RtError):
        r.denoise_temporal_antilag(True, sigma=1.0)
    r.close()
    s = api.Renderer(W, H * 4, rows=(0, H * 2), halo=8)
    s.set_scene(base)
    assert s.L.rt_denoise_temporal_antilag(s.h, 1, None) == RT_ERR_UNSUPPORTED
    on = C.c_int(7)
    assert s.L.rt_denoise_temporal_antilag_get(s.h, C.byref(on), None, None) == RT_OK and on.value == 0
    s.close()


# ------------------------------------------------------------------------------------------------------------ stream ordering
def test_stream_ordering_of_an_adapted_call(api, monkeypatch):
    """frames 1-3, rt_denoise_temporal, frames 4-6, rt_denoise_temporal (an adapted call), frames 7-8, the downloads: under every plan
    of tests/stream_delay.py (each stream of the context parked in turn, both, at random) on the context's own stream and on a
    caller's, the downloads are the synchronised run's"""
    import stream_delay as sd
    from test_gpu_stream_order import check, reference_of

    setup = sd._setup

    def with_antilag(e, op, args):
        if op == "denoise_antilag":
            e.r.denoise_temporal_antilag(*args)
        else:
            setup(e, op, args)

    monkeypatch.setattr(sd, "_setup", with_antilag)
    script = sd.foreign_script("denoise_temporal")._replace(name="foreign_denoise_temporal_antilag", setup=(("denoise_antilag", (True,)),))
    hist = [a for n, a in reference_of(script) if n.endswith("denoise history")]
    assert hist and (np.asarray(hist[-1]).reshape(-1, 4)[:, 3] > 0.0).any(), "the synchronised run's last call was not an adapted call that responded"
    for mode in ("own", "caller"):
        check(script, mode)


# ------------------------------------------------------------------------------------------------------------ restir_app
def test_restir_app_denoise_antilag_equals_the_renderer(tmp_path, api, base):
    from cedec_2024_rt_amd.types import bench_options

    W, H, frames = 40, 33, 4
    path, out = os.path.join(str(tmp_path), "lamp.tris"), os.path.join(str(tmp_path), "out.raw")
    base.tofile(path)
    head = [APP, "--tris", path, "--size", str(W), str(H), "--eye", *map(str, ls.LAMP_EYE), "--lookat", *map(str, ls.LAMP_AT), "--accumulate", "0",
            "--frames", str(frames), "--denoise", "2", "--denoise-temporal", "--move-tris", str(BOX_LO), str(BOX_HI - BOX_LO), *map(str, STEP)]
    for flag, al in ((["--denoise-antilag"], {}), (["--denoise-antilag", "2", "0.25", "0.75", "0.05", "--denoise-follow-motion"], dict(radius=2, gradient_lo=0.25, gradient_hi=0.75, floor=0.05))):
        p = subprocess.run(head + flag + ["--rgba", out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert p.stdout.count("anti-lag adapted") == frames - 1 and p.stdout.count("anti-lag not adapted") == 1, p.stdout
        app_px = np.fromfile(out, np.uint8).reshape(H, W, 4)
        r = api.Renderer(W, H)
        r.set_scene(base)
        r.lookat(ls.LAMP_EYE, ls.LAMP_AT)
        r.set_options(bench_options(accumulate=0))
        r.denoise_temporal_motion(len(flag) > 1)
        r.denoise_temporal_antilag(True, **al)
        r.clear()
        t = base
        for f in range(1, frames + 1):
            if f >= 2:
                t = move(t, STEP)
                _box(r, t)
            r.frame(f)
            px = r.denoise_temporal(iterations=2)
        assert r.denoise_temporal_antilag()["adapted"]
        r.close()
        assert np.array_equal(app_px, px), f"{flag}: {int((app_px != px).any(axis=2).sum())} pixels differ"
    p = subprocess.run([APP, "--tris", path, "--denoise", "2", "--denoise-antilag"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--denoise-antilag needs" in p.stderr, p.stdout + p.stderr
    p = subprocess.run(head + ["--denoise-antilag", "7", "0.2", "0.8", "0.1"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "radius" in p.stdout + p.stderr, p.stdout + p.stderr
