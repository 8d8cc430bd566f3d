"""rt_denoise_temporal (include/restir_rt_internal.h, csrc/denoise_kernels.h) on the GPU.

* RT_BUF_DENOISED and RT_BUF_DENOISE_HISTORY == the CPU restatement (tests/denoise_temporal_ref.py) bit for bit after every call of
  a 6-frame orbit: the bench stand-in at 1920 x 1080 and 333 x 187 (partial tiles), 0, 1 and 5 iterations, both layouts of
  rt_tuning key 28, ReSTIR and 07_pt input;
* the first call after a reset equals rt_denoise; rt_scene_update between calls keeps the history (still the restatement);
  rt_scene_set and rt_denoise_temporal_reset empty it; rt_denoise calls in between change nothing;
* no side effects on an unsynchronised frame sequence; error codes; timing; restir_app --denoise-temporal --orbit == the Renderer.
"""
import os
import subprocess

import numpy as np
import pytest

import denoise_temporal_ref as dtr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "app", "restir_app")
RT_OK, RT_ERR_ARG, RT_ERR_STATE, RT_ERR_UNSUPPORTED = 0, 1, 3, 5
ROOM_EYE, ROOM_AT = (0.5, 2.5, 6.0), (0.0, 1.5, -1.0)
ORBIT = (12.0, 0.0)


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def blocks():
    from cedec_2024_rt_amd import scenes
    return scenes.make_blocks_restir(), scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT


@pytest.fixture(scope="module")
def room():
    from cedec_2024_rt_amd import scenes
    return scenes.make_quad_room(), ROOM_EYE, ROOM_AT


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _ndiff(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1, 4).view(np.uint32), np.ascontiguousarray(b).reshape(-1, 4).view(np.uint32)
    return int((a != b).any(axis=1).sum())


def _renderer(api, scene, W, H, layout=None, **opt):
    from cedec_2024_rt_amd.types import bench_options

    tris, eye, at = scene
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(eye, at)
    r.set_options(bench_options(**opt))
    if layout is not None:
        r.tuning(api.Tune.DN_LAYOUT, layout)
    return r


def _render(r, example, f):
    if example == 10:
        r.frame(f)
    else:
        r.path_trace(example, f)


def _call(api, r, params):
    """one temporal call: (HDR, history, guide hits, eye, raygen, accumulation as the call saw it)"""
    acc = r.download(api.RT_BUF_ACCUMULATION)
    hdr = r.denoise_temporal(hdr=True, **params).reshape(-1, 4)
    return hdr, r.download(api.RT_BUF_DENOISE_HISTORY), r.download(api.RT_BUF_DENOISE_GUIDE), r.camera_pose()[0], r.raygen(), acc


def _orbit_sequence(api, scene, W, H, example=10, frames=6, layouts=(0, 1), **params):
    """frames of an orbit, one temporal call after each, on one context per layout: every call == the restatement"""
    rs = [_renderer(api, scene, W, H, layout=lay, accumulate=0) for lay in layouts]
    T = dtr.TemporalRef(W, H, scene[0], **params)
    hist = []
    for f in range(1, frames + 1):
        ref = None
        for lay, r in zip(layouts, rs):
            if f >= 2:
                r.orbit(*ORBIT)
            _render(r, example, f)
            r.sync()
            hdr, mom, vis, eye, rg, acc = _call(api, r, params)
            if ref is None:
                ref = T(vis, eye, rg, acc)
            assert _eq_bits(hdr, ref[0]), f"frame {f} layout {lay} {params}: {_ndiff(hdr, ref[0])} pixels differ from the restatement"
            assert _eq_bits(mom, ref[1]), f"frame {f} layout {lay} {params}: {_ndiff(mom, ref[1])} history records differ"
            assert _eq_bits(r.download(api.RT_BUF_ACCUMULATION), acc), "rt_denoise_temporal changed the accumulation buffer"
        hist.append(ref[1][:, 2].copy())
    for r in rs:
        r.close()
    return hist


def test_orbit_1080p_equals_cpu(api, blocks):
    hist = _orbit_sequence(api, blocks, 1920, 1080)
    # the history grows where the orbit keeps surfaces in view
    assert float(np.mean(hist[-1] == 6.0)) > 0.5, np.unique(hist[-1], return_counts=True)


@pytest.mark.parametrize("iterations", [0, 1, 5])
def test_orbit_partial_tiles_equals_cpu(api, blocks, iterations):
    _orbit_sequence(api, blocks, 333, 187, iterations=iterations)


def test_orbit_other_parameters_equals_cpu(api, blocks):
    _orbit_sequence(api, blocks, 333, 187, frames=5, layouts=(1,), iterations=3, sigma_luminance=2.5, sigma_plane=0.5,
                    normal_power_log2=3, variance_radius=1, alpha_color=0.05, alpha_moments=0.5)


def test_path_trace_orbit_equals_cpu(api, room):
    _orbit_sequence(api, room, 96, 64, example=7)


def test_first_call_after_reset_equals_rt_denoise(api, blocks):
    r = _renderer(api, blocks, 333, 187, accumulate=0)
    for f in range(1, 4):
        if f >= 2:
            r.orbit(*ORBIT)
        r.frame(f)
        first = r.denoise_temporal(hdr=True).copy()
        if f == 1:
            assert _eq_bits(first, r.denoise(hdr=True)), "the first call != rt_denoise"
    r.denoise_temporal_reset()
    buf = np.zeros(333 * 187 * 4, np.float32)
    assert r.L.rt_download(r.h, api.RT_BUF_DENOISE_HISTORY, buf.ctypes.data, buf.nbytes) == RT_ERR_STATE
    for it in (0, 1, 5):
        r.denoise_temporal_reset()
        t = r.denoise_temporal(hdr=True, iterations=it).copy()
        assert _eq_bits(t, r.denoise(hdr=True, iterations=it)), f"{it} iterations: the first call after a reset != rt_denoise"
    r.close()


def test_scene_update_keeps_the_history(api, blocks):
    from cedec_2024_rt_amd import scenes

    tris, eye, at = blocks
    W, H = 333, 187
    r = _renderer(api, blocks, W, H, accumulate=0)
    T = dtr.TemporalRef(W, H, tris)
    lights = np.flatnonzero((tris["emissive"] > 0).any(axis=1))
    lo, hi = int(lights.min()), int(lights.max()) + 1
    cur = tris.copy()
    for f in range(1, 5):
        if f >= 2:
            r.orbit(*ORBIT)
        if f >= 3:  # the lights and the triangles between them move: a refit, not a rebuild
            mask = np.zeros(len(cur), bool)
            mask[lo:hi] = True
            cur = scenes.move_triangles(cur, mask, (0.05, 0.0, 0.0))
            r.update_scene(cur[lo:hi], first=lo)
            T.tris = np.ascontiguousarray(cur).view(np.uint8)
        r.frame(f)
        r.sync()
        hdr, mom, vis, e, rg, acc = _call(api, r, {})
        want = T(vis, e, rg, acc)
        assert _eq_bits(hdr, want[0]) and _eq_bits(mom, want[1]), f"frame {f}: {_ndiff(hdr, want[0])} pixels differ"
        if f >= 3:
            assert float(np.max(mom[:, 2])) == f  # kept across the update
    r.close()


def test_scene_set_and_reset_empty_the_history(api, blocks):
    W, H = 333, 187
    buf = np.zeros(W * H * 4, np.float32)
    r = _renderer(api, blocks, W, H, accumulate=0)
    for f in range(1, 4):
        r.frame(f)
        r.denoise_temporal()
    assert float(r.download(api.RT_BUF_DENOISE_HISTORY)[:, 2].max()) == 3.0
    r.set_scene(blocks[0])
    assert r.L.rt_download(r.h, api.RT_BUF_DENOISE_HISTORY, buf.ctypes.data, buf.nbytes) == RT_ERR_STATE
    r.frame(4)
    t = r.denoise_temporal(hdr=True).copy()
    assert float(r.download(api.RT_BUF_DENOISE_HISTORY)[:, 2].max()) == 1.0
    assert _eq_bits(t, r.denoise(hdr=True))
    r.frame(5)
    r.denoise_temporal()
    assert float(r.download(api.RT_BUF_DENOISE_HISTORY)[:, 2].max()) == 2.0
    r.denoise_temporal_reset()
    assert r.L.rt_download(r.h, api.RT_BUF_DENOISE_HISTORY, buf.ctypes.data, buf.nbytes) == RT_ERR_STATE
    r.denoise_temporal()
    assert float(r.download(api.RT_BUF_DENOISE_HISTORY)[:, 2].max()) == 1.0
    r.close()


def test_rt_denoise_in_between_changes_nothing(api, blocks):
    W, H = 333, 187
    a = _renderer(api, blocks, W, H, accumulate=0)
    b = _renderer(api, blocks, W, H, accumulate=0)
    for f in range(1, 6):
        for r in (a, b):
            if f >= 2:
                r.orbit(*ORBIT)
            r.frame(f)
        b.denoise(iterations=2, variance_radius=1)  # between the frame and the temporal call, and after it
        ta, tb = a.denoise_temporal(hdr=True).copy(), b.denoise_temporal(hdr=True).copy()
        ha, hb = a.download(api.RT_BUF_DENOISE_HISTORY), b.download(api.RT_BUF_DENOISE_HISTORY)
        b.denoise(iterations=8)
        assert _eq_bits(ta, tb) and _eq_bits(ha, hb), f"frame {f}"
    a.close()
    b.close()


def _state(api, r):
    import ctypes as C

    r.sync()
    e = C.c_uint64()
    assert r.L.rt_state_epoch(r.h, C.byref(e)) == RT_OK
    return [r.download(b) for b in (api.RT_BUF_ACCUMULATION, api.RT_BUF_RES_0, api.RT_BUF_RES_1, api.RT_BUF_RES_TEMPORAL)] + [e.value]


def test_no_side_effects_on_the_frame_sequence(api, blocks):
    """rt_denoise_temporal between rt_frame calls, nothing synchronised: the frames' own state is what it is without the calls,
    and the last result is a synchronised run's."""
    W, H, frames = 333, 187, 6
    plain = _renderer(api, blocks, W, H, accumulate=1)
    for f in range(1, frames + 1):
        if f >= 2:
            plain.orbit(*ORBIT)
        plain.frame(f, clear_first=f >= 2)
    want = _state(api, plain)
    plain.close()

    r = _renderer(api, blocks, W, H, accumulate=1)
    for f in range(1, frames + 1):
        if f >= 2:
            r.orbit(*ORBIT)
        r.frame(f, clear_first=f >= 2)
        assert r.L.rt_denoise_temporal(r.h, None, None) == RT_OK, r.L.rt_last_error(r.h)
    got = _state(api, r)
    hdr, mom, px = r.download(api.RT_BUF_DENOISED), r.download(api.RT_BUF_DENOISE_HISTORY), r.download(api.RT_BUF_PIXELS)
    r.close()
    for name, x, y in zip(("accumulation", "RES_0", "RES_1", "RES_TEMPORAL", "epoch"), got, want):
        assert (x == y) if name == "epoch" else _eq_bits(x, y), name

    s = _renderer(api, blocks, W, H, accumulate=1)
    for f in range(1, frames + 1):
        if f >= 2:
            s.orbit(*ORBIT)
        s.frame(f, clear_first=f >= 2)
        s.sync()
        h = s.denoise_temporal(hdr=True)
        s.sync()
    assert _eq_bits(h.reshape(-1, 4), hdr) and _eq_bits(s.download(api.RT_BUF_DENOISE_HISTORY), mom)
    assert _eq_bits(s.download(api.RT_BUF_PIXELS), px)
    s.close()


def test_error_codes_and_timing(api, room):
    W, H = 64, 36
    r = api.Renderer(W, H)
    buf = np.zeros(W * H * 4, np.float32)
    ms = np.zeros(6, np.float32)
    assert r.L.rt_download(r.h, api.RT_BUF_DENOISE_HISTORY, buf.ctypes.data, buf.nbytes) == RT_ERR_STATE
    assert r.L.rt_denoise_temporal_timing(r.h, ms.ctypes.data) == RT_ERR_STATE
    assert r.L.rt_denoise_temporal(r.h, None, None) == RT_ERR_STATE  # no scene
    r.set_scene(room[0])
    assert r.L.rt_denoise_temporal(r.h, None, None) == RT_ERR_STATE  # no camera
    r.lookat(room[1], room[2])
    for a, m in ((0.0, 0.2), (0.2, 0.0), (1.5, 0.2), (0.2, -1.0), (float("nan"), 0.2), (0.2, float("inf"))):
        t = np.zeros(1, dtype=api.DENOISE_TEMPORAL_PARAMS)
        t[0] = (a, m)
        assert r.L.rt_denoise_temporal(r.h, None, t.ctypes.data) == RT_ERR_ARG, (a, m)
    for b in (dict(iterations=9), dict(sigma_luminance=0.0), dict(variance_radius=4)):
        p = np.zeros(1, dtype=api.DENOISE_PARAMS)
        p[0] = (5, 4.0, 1.0, 7, 3)
        for k, v in b.items():
            p[k] = v
        assert r.L.rt_denoise_temporal(r.h, p.ctypes.data, None) == RT_ERR_ARG, b
    assert r.L.rt_download(r.h, api.RT_BUF_DENOISE_HISTORY, buf.ctypes.data, buf.nbytes) == RT_ERR_STATE
    t = np.zeros(1, dtype=api.DENOISE_TEMPORAL_PARAMS)
    t[0] = (1.0, 1.0)
    assert r.L.rt_denoise_temporal(r.h, None, t.ctypes.data) == RT_OK
    assert r.L.rt_download(r.h, api.RT_BUF_DENOISE_HISTORY, buf.ctypes.data, buf.nbytes) == RT_OK
    assert r.L.rt_download(r.h, api.RT_BUF_DENOISE_HISTORY, buf.ctypes.data, buf.nbytes - 16) == RT_ERR_ARG
    assert r.L.rt_upload(r.h, api.RT_BUF_DENOISE_HISTORY, buf.ctypes.data, buf.nbytes) == RT_ERR_ARG  # download only
    r.timing_enable(True)
    r.denoise_temporal()
    tm = r.denoise_temporal_timing()
    assert all(v > 0.0 for v in tm.values()), tm
    assert tm["total"] >= max(v for k, v in tm.items() if k != "total")
    assert r.L.rt_denoise_temporal_reset(r.h) == RT_OK
    assert r.L.rt_download(r.h, api.RT_BUF_DENOISE_HISTORY, buf.ctypes.data, buf.nbytes) == RT_ERR_STATE
    r.close()
    s = api.Renderer(W, H, rows=(0, H // 2), halo=8)
    s.set_scene(room[0])
    s.lookat(room[1], room[2])
    assert s.L.rt_denoise_temporal(s.h, None, None) == RT_ERR_UNSUPPORTED
    s.close()


@pytest.mark.parametrize("example,accumulate", [(10, 0), (10, 1), (7, 1)])
def test_restir_app_denoise_temporal_equals_the_renderer(tmp_path, api, room, example, accumulate):
    from cedec_2024_rt_amd.types import bench_options

    tris, eye, at = room
    path = os.path.join(str(tmp_path), "room.tris")
    tris.tofile(path)
    out, pfm = os.path.join(str(tmp_path), "out.raw"), os.path.join(str(tmp_path), "out.pfm")
    W, H, frames = 96, 64, 4
    cmd = [APP, "--example", str(example), "--tris", path, "--size", str(W), str(H), "--eye", *map(str, eye), "--lookat", *map(str, at),
           "--accumulate", str(accumulate), "--frames", str(frames), "--denoise", "5", "--denoise-temporal", "--orbit", *map(str, ORBIT),
           "--rgba", out, "--pfm", pfm]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("denoise:") == frames and "reprojection" in p.stdout, p.stdout
    app_px = np.fromfile(out, np.uint8).reshape(H, W, 4)

    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(eye, at)
    r.set_options(bench_options(accumulate=accumulate))
    r.clear()
    for f in range(1, frames + 1):
        if f >= 2:
            r.orbit(*ORBIT)
        moved = f >= 2 and accumulate == 1
        if example == 10:
            r.frame(f, clear_first=moved)
        else:
            if moved:
                r.clear()
            r.path_trace(example, f)
            r.tone_mapping()
        px = r.denoise_temporal(iterations=5)
        hdr = r.download(api.RT_BUF_DENOISED)
    r.close()
    assert np.array_equal(app_px, px), f"{int((app_px != px).any(axis=2).sum())} pixels differ"
    with open(pfm, "rb") as f:
        body = f.read().split(b"\n", 3)[3]
    want = (hdr[:, :3] / hdr[:, 3:4]).astype(np.float32)
    assert _eq_bits(np.frombuffer(body, np.float32).reshape(-1, 3), want)


def test_restir_app_denoise_temporal_refusals(tmp_path, room):
    path = os.path.join(str(tmp_path), "room.tris")
    room[0].tofile(path)
    for extra, word in ((["--denoise-temporal"], "--denoise-temporal"), (["--orbit", "1", "0", "--ranks", "2"], "--orbit"),
                        (["--orbit", "1", "0", "--example", "6"], "--orbit")):
        p = subprocess.run([APP, "--tris", path, "--size", "64", "36", *extra], capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and word in p.stderr, (extra, p.stdout + p.stderr)
