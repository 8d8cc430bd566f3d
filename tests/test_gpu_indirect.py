"""rt_indirect on the device: k_indirect against tests/indirect_ref.py with
its GBUFFER start (the restatement compiled from the kernels' own header, anchored to the oracle by tests/test_indirect_cpu.py), bit
for bit. The restatement is applied to the accumulation buffer as downloaded after resolve, so everything before the pass is the
device's own frame (held to the oracle by tests/test_gpu_parity.py); tone mapping after it is the oracle's.

Sizes: 64 x 48 (whole tiles), 9 x 7 (partial tiles in both directions), 67 x 5 (thin), 8 x 8 (one tile, one wavefront)."""
import ctypes as C

import numpy as np
import pytest

import indirect_ref as ir
from restir_unbiased_ref import LEDGE_AT, LEDGE_EYE, make_ledge

pytestmark = pytest.mark.gpu

EYE, AT, FOVY = (0.5, 3.0, 6.0), (0.0, 1.0, -1.5), np.float32(0.9)
RT_ERR_ARG, RT_ERR_STATE, RT_ERR_UNSUPPORTED = 1, 3, 5  # include/restir_rt.h


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _eq_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _differing(a, b, W):
    a, b = np.ascontiguousarray(a).reshape(-1, 4).view(np.uint32), np.ascontiguousarray(b).reshape(-1, 4).view(np.uint32)
    i = np.flatnonzero((a != b).any(axis=1))
    return f"{len(i)} pixels differ, first (x, row): {[(int(k % W), int(k // W)) for k in i[:8]]}"


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def worlds(oracle):
    from cedec_2024_rt_amd import scenes

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    room = scenes.make_quad_room()
    one = room.copy()
    lights = np.flatnonzero((one["emissive"] > 0).any(axis=1))
    one["emissive"][lights[1:]] = 0.0  # the other lamps become plain surfaces
    return dict(room=dict(tris=room, eye=EYE, at=AT), one_light=dict(tris=one, eye=EYE, at=AT),
                ledge=dict(tris=make_ledge(oracle.TRIANGLE), eye=LEDGE_EYE, at=LEDGE_AT),
                blocks=dict(tris=scenes.make_blocks_restir(detail=0.02), eye=scenes.BLOCKS_RESTIR_EYE, at=scenes.BLOCKS_RESTIR_LOOKAT))


def _renderer(api, world, W, H, opt=None, **kw):
    from cedec_2024_rt_amd.types import bench_options

    r = api.Renderer(W, H, **kw)
    r.set_scene(world["tris"])
    r.lookat(world["eye"], world["at"], fovy=FOVY)
    r.set_options(bench_options() if opt is None else opt)
    return r


def _until_resolve(api, r, frame):
    """frame_by_kernels up to and including resolve"""
    r.raycast()
    r.generate_candidate(frame, api.RT_RES_0)
    r.temporal_resampling(frame, api.RT_RES_TEMPORAL, api.RT_RES_0)
    r.save_temporal_reservoir(api.RT_RES_0, api.RT_RES_TEMPORAL)
    src, dst = api.RT_RES_0, api.RT_RES_1
    for k in range(int(r.options()["spatial_resampling_passes"][0])):
        if k:
            src, dst = dst, src
        r.spatial_resampling(frame, k, src, dst)
    r.resolve(dst)


def _check_pass(api, oracle, r, world, W, H, frame, cases, name):
    """the accumulation buffer stands after resolve: every bounce count of `cases` on a fresh copy of it against the restatement.
    Leaves the first case's result in the buffer and returns it."""
    direct = r.download(api.RT_BUF_ACCUMULATION)
    vis, eye, rg = r.download(api.RT_BUF_VISIBILITY), r.camera_pose()[0], r.raygen()
    want, first = {}, None
    for bounces in cases:
        if bounces not in want:
            acc = direct.copy()
            want[bounces] = (acc, ir.add(acc, W, H, frame, world["tris"], vis, eye, rg, bounces))
        r.upload(api.RT_BUF_ACCUMULATION, direct)
        r.indirect_pass(frame, bounces)
        got = r.download(api.RT_BUF_ACCUMULATION)
        acc, st = want[bounces]
        assert _eq_bits(got, acc), f"{name} frame {frame} bounces {bounces}: {_differing(got, acc, W)}"
        assert r.indirect_stats() == st, f"{name} frame {frame} bounces {bounces}"
        first = got if first is None else first
    r.upload(api.RT_BUF_ACCUMULATION, first)
    return first, want[cases[0]][1]


@pytest.mark.parametrize("W,H", [(64, 48), (9, 7), (67, 5), (8, 8)])
def test_pass_after_a_kernel_sequence_equals_the_restatement(api, oracle, worlds, W, H):
    world = worlds["room"]
    added = 0
    for accumulate in (0, 1):
        r = _renderer(api, world, W, H, oracle.bench_options(accumulate=accumulate))
        for frame in (1, 2, 3):
            _until_resolve(api, r, frame)
            before = r.download(api.RT_BUF_ACCUMULATION)
            acc, st = _check_pass(api, oracle, r, world, W, H, frame, [2, 1, 6], f"{W} x {H} accumulate {accumulate}")
            vis = r.download(api.RT_BUF_VISIBILITY)
            shaded = (vis["index"] >= 0) & ~(world["tris"]["emissive"] > 0).any(axis=1)[np.maximum(vis["index"], 0)]
            assert st["paths"] == int(shaded.sum())
            # the sample count is resolve's: the pass leaves it
            assert _eq_bits(acc[:, 3], before[:, 3]) and (acc[shaded, 3] == (frame if accumulate else 1)).all()
            assert _eq_bits(acc[~shaded], before[~shaded])
            added += int((acc[:, :3] != before[:, :3]).any(axis=1).sum())
            r.tone_mapping()
            assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), oracle.tone_mapping(acc, W, H))
        r.close()
    assert added > 0, "the pass added nothing anywhere: the comparison would show nothing"


@pytest.mark.parametrize("name,W,H,bounces", [("ledge", 64, 48, 6), ("one_light", 37, 29, 3), ("blocks", 32, 24, 2)])
def test_other_scenes(api, oracle, worlds, name, W, H, bounces):
    """open sky (paths leave without a contribution, sky pixels start none), one light, the pre-split stand-in at its smallest size"""
    world = worlds[name]
    r = _renderer(api, world, W, H)
    _until_resolve(api, r, 2)
    before = r.download(api.RT_BUF_ACCUMULATION)
    acc, st = _check_pass(api, oracle, r, world, W, H, 2, [bounces], name)
    vis = r.download(api.RT_BUF_VISIBILITY)
    lit = (world["tris"]["emissive"] > 0).any(axis=1)
    unshaded = (vis["index"] < 0) | lit[np.maximum(vis["index"], 0)]
    assert st["paths"] == int((~unshaded).sum()) > 0
    assert _eq_bits(acc[unshaded], before[unshaded])
    if name == "ledge":
        assert (vis["index"] < 0).any() and st["alive_last"] < st["paths"] // 4
    assert (acc[:, :3] != before[:, :3]).any()
    r.close()


@pytest.mark.parametrize("keys", [((0, 0),), ((0, 1),), ((0, 2),), ((0, 3),), ((0, 4),), ((0, 5),), ((0, 6),), ((0, 7),), ((13, 0), (16, 1))])
def test_tuning_keys_leave_the_output_unchanged(api, oracle, worlds, keys):
    """the tile orders of the tracing kernels (key 0: the raycast's, which the pass takes) and the walks' keys"""
    world, W, H = worlds["room"], 100, 76
    plain, tuned = _renderer(api, world, W, H), _renderer(api, world, W, H)
    for k, v in keys:
        tuned.tuning(k, v)
    for r in (plain, tuned):
        _until_resolve(api, r, 1)
    out = []
    for r in (plain, tuned):
        r.indirect_pass(1, 3)
        out.append((r.download(api.RT_BUF_ACCUMULATION), r.indirect_stats()))
    assert _eq_bits(out[0][0], out[1][0]) and out[0][1] == out[1][1], f"keys {keys}"
    plain.close(), tuned.close()


@pytest.mark.parametrize("reuse", [True, False])
def test_frame_equals_the_kernel_sequence(api, oracle, worlds, reuse):
    """rt_frame with the toggle against resolve -> rt_indirect_pass -> tone mapping by kernels, six frames, a camera orbit at frame 3 and
    an rt_scene_update at frame 5: the look-ahead stage 0 of the next frame writes the other G-buffer set while the pass reads its own"""
    from cedec_2024_rt_amd import scenes

    world, W, H = worlds["room"], 64, 48
    opt = oracle.bench_options(accumulate=1)
    rf, rk = _renderer(api, world, W, H, opt), _renderer(api, world, W, H, opt)
    rf.gbuffer_reuse(reuse)
    assert rf.indirect() == 0 and rf.indirect(2) == 2
    moved = scenes.move_triangles(world["tris"], np.arange(len(world["tris"])) >= len(world["tris"]) - 12, (0.25, 0.0, -0.125))
    tris = world["tris"]
    for frame in range(1, 7):
        if frame == 3:
            rf.orbit(12.0, -5.0), rk.orbit(12.0, -5.0)
        if frame == 5:
            rf.update_scene(moved), rk.update_scene(moved)
            tris = moved
        clear = frame in (3, 5)
        out_f = rf.frame(frame, clear_first=clear)
        out_k = rk.frame_by_kernels(frame, clear_first=clear, indirect=2)
        assert out_f == out_k
        acc_f, acc_k = rf.download(api.RT_BUF_ACCUMULATION), rk.download(api.RT_BUF_ACCUMULATION)
        assert _eq_bits(acc_f, acc_k), f"frame {frame}: accumulation: {_differing(acc_f, acc_k, W)}"
        assert _eq_bits(rf.download(api.RT_BUF_PIXELS), rk.download(api.RT_BUF_PIXELS)), f"frame {frame}: pixels"
        assert rf.indirect_stats() == rk.indirect_stats()
    # and the kernel sequence's last pass is the restatement's (the moved scene, the orbited camera)
    _until_resolve(api, rk, 7)
    _check_pass(api, oracle, rk, dict(tris=tris), W, H, 7, [2], "after the sequence")
    rf.close(), rk.close()


def _epoch(r):
    e = C.c_uint64()
    assert r.L.rt_state_epoch(r.h, C.byref(e)) == 0
    return e.value


def test_on_then_off_equals_a_context_that_never_had_it(api, oracle, worlds):
    world, W, H = worlds["room"], 64, 48
    a, b = _renderer(api, world, W, H), _renderer(api, world, W, H)
    e0 = _epoch(a)
    assert a.indirect(5) == 5 and _epoch(a) != e0
    a.frame(1), b.frame(1)
    assert not _eq_bits(a.download(api.RT_BUF_ACCUMULATION), b.download(api.RT_BUF_ACCUMULATION))
    e1 = _epoch(a)
    assert a.indirect(0) == 0 and _epoch(a) != e1
    for frame in (2, 3):
        oa, ob_ = a.frame(frame), b.frame(frame)
        assert oa == ob_
        for buf in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0 + oa):
            assert _eq_bits(a.download(buf), b.download(buf)), f"frame {frame}: buffer {buf}"
    a.close(), b.close()


def test_staged_frame_runs_the_pass_in_the_resolve_stage(api, oracle, worlds):
    """rt_frame_stage* with the toggle on: the resolve stage runs the pass over all owned rows; a partial run of that stage is refused"""
    world, W, H = worlds["room"], 64, 48
    a, b = _renderer(api, world, W, H), _renderer(api, world, W, H)
    a.indirect(3), b.indirect(3)
    passes = int(a.options()["spatial_resampling_passes"][0])
    b.frame(1)
    for st in range(passes + 2):
        assert a.L.rt_frame_stage(a.h, 1, st, 0) == 0
    assert _eq_bits(a.download(api.RT_BUF_ACCUMULATION), b.download(api.RT_BUF_ACCUMULATION))
    assert _eq_bits(a.download(api.RT_BUF_PIXELS), b.download(api.RT_BUF_PIXELS))
    for st in range(passes + 1):
        assert a.L.rt_frame_stage(a.h, 2, st, 0) == 0
    assert a.L.rt_frame_stage_begin(a.h, 2, passes + 1, 0) == 0
    assert a.L.rt_frame_stage_run(a.h, 2, passes + 1, 0, H // 2) == RT_ERR_UNSUPPORTED
    assert a.L.rt_frame_stage_run(a.h, 2, passes + 1, 0, H) == 0 and a.L.rt_frame_stage_end(a.h, passes + 1) == 0
    b.frame(2)
    assert _eq_bits(a.download(api.RT_BUF_ACCUMULATION), b.download(api.RT_BUF_ACCUMULATION))
    a.close(), b.close()


def test_denoiser_takes_the_summed_image(api, oracle, worlds):
    import denoise_ref

    world, W, H = worlds["room"], 64, 48
    r = _renderer(api, world, W, H)
    r.indirect(3)
    r.frame(1)
    acc = r.download(api.RT_BUF_ACCUMULATION)
    hdr = r.denoise(hdr=True).reshape(-1, 4)
    eye, rg = r.camera_pose()[0], r.raygen()
    ref = denoise_ref.denoise(W, H, world["tris"], r.download(api.RT_BUF_VISIBILITY), eye, rg["up"][0], acc)
    assert _eq_bits(hdr, ref), _differing(hdr, ref, W)
    assert _eq_bits(r.download(api.RT_BUF_ACCUMULATION), acc)
    r.close()


def test_refusals(api, oracle, worlds):
    world, W, H = worlds["room"], 64, 48
    strip = _renderer(api, world, W, H, rows=(0, 24), halo=8)
    strip.raycast()
    assert strip.L.rt_indirect(strip.h, 2) == RT_ERR_UNSUPPORTED and strip.L.rt_indirect_pass(strip.h, 1, 2) == RT_ERR_UNSUPPORTED
    strip.close()
    r = _renderer(api, world, W, H)
    for bad in (33, -1):
        assert r.L.rt_indirect(r.h, bad) == RT_ERR_ARG and r.indirect() == 0
    assert r.L.rt_indirect_pass(r.h, 1, 33) == RT_ERR_ARG and r.L.rt_indirect_pass(r.h, 1, 0) == RT_ERR_ARG
    out = np.zeros(3, np.uint64)
    assert r.L.rt_indirect_stats(r.h, out.ctypes.data_as(C.c_void_p)) == RT_ERR_STATE
    # no traced G-buffer: none yet, then one of another camera
    assert r.L.rt_indirect_pass(r.h, 1, 2) == RT_ERR_STATE
    r.raycast()
    assert r.L.rt_indirect_pass(r.h, 1, 2) == 0
    r.orbit(3.0, 0.0)
    assert r.L.rt_indirect_pass(r.h, 1, 2) == RT_ERR_STATE
    ms = C.c_float()
    assert r.L.rt_indirect_timing(r.h, C.byref(ms)) == RT_ERR_STATE
    r.timing_enable(True)
    r.raycast()
    r.indirect_pass(1, 2)
    assert r.indirect_timing() > 0.0
    r.close()
    # no lights: the pass and the frame with the toggle, with rt_path_trace's message for 08_nee
    dark = dict(world, tris=world["tris"].copy())
    dark["tris"]["emissive"] = 0.0
    r = _renderer(api, dark, W, H)
    r.raycast()
    assert r.L.rt_path_trace(r.h, 8, 1) == RT_ERR_STATE
    msg = r.L.rt_last_error(r.h)
    assert r.L.rt_indirect_pass(r.h, 1, 2) == RT_ERR_STATE and r.L.rt_last_error(r.h) == msg
    r.indirect(2)
    assert r.L.rt_frame(r.h, 1, 0, None) == RT_ERR_STATE and r.L.rt_last_error(r.h) == msg
    r.close()
