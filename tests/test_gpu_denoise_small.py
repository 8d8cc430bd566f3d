"""rt_denoise and rt_denoise_temporal on the GPU at the shapes and history lengths the larger tests leave out, against both the
C++ restatements (bit for bit) and the independent float64 reference of tests/denoise_spec.py (within the tolerance that
tests/denoise_spec_cases.py derives from the reference's own float32 run). Scene and inputs: tests/denoise_spec_cases.py.

* rt_denoise at 8 x 8, 19 x 7, 7 x 19 (narrower than one 16 x 16 block of k_denoise_iter_lds), 16 x 16, 17 x 17 (a second block of
  one row and column), 40 x 33, 257 x 20 and 20 x 257 (257 = 16 * 16 + 1: at step 16 one residue has 17 lattice points, at step 1
  the last block is one pixel wide); 0, 1, 5 and 8 iterations (step 128: larger than every image here); both layouts of rt_tuning
  key 28; an uploaded accumulation with w == 0 records. RT_BUF_PIXELS == rt_tone_mapping of the result; the accumulation stays.
* rt_denoise_temporal over the five camera sequences at 40 x 33 on both layouts, the 36 static calls included (h passes 4, 1 / alpha
  and the cap of 32 on the device), plus one sequence at 8 x 8 and one at 19 x 7: after every call RT_BUF_DENOISED and
  RT_BUF_DENOISE_HISTORY == the restatement, then the moments and the image against the teacher-forced reference.
"""
import numpy as np
import pytest

import denoise_ref
import denoise_spec_cases as cs
import denoise_temporal_ref as dtr

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (19, 7), (7, 19), (16, 16), (17, 17), (40, 33), (257, 20), (20, 257)]


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def tris():
    return cs.scene()


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _differing(a, b, W):
    """the differing pixels as (x, row) pairs, for the message: they name the residue, block and apron cell involved"""
    a, b = np.ascontiguousarray(a).reshape(-1, 4).view(np.uint32), np.ascontiguousarray(b).reshape(-1, 4).view(np.uint32)
    i = np.flatnonzero((a != b).any(axis=1))
    return f"{len(i)} pixels differ, first (x, row): {[(int(k % W), int(k // W)) for k in i[:12]]}"


def _renderer(api, tris, W, H, layout=None):
    from cedec_2024_rt_amd.types import bench_options

    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(cs.EYE, cs.AT)
    r.set_options(bench_options())
    if layout is not None:
        r.tuning(api.Tune.DN_LAYOUT, layout)
    return r


@pytest.mark.parametrize("W,H", SIZES)
def test_small_images_equal_restatement_and_reference(api, tris, W, H):
    r = _renderer(api, tris, W, H)
    acc = cs.accumulation(W, H, 100 + W)
    r.upload(api.RT_BUF_ACCUMULATION, acc)
    eye, rg = r.camera_pose()[0], r.raygen()
    case = None
    for params in [dict(iterations=it) for it in (0, 1, 5, 8)] + [dict(iterations=5, **cs.OTHER)]:
        ref = None
        for lay in (0, 1):
            name = f"{W} x {H}, layout {lay}, {params}"
            r.tuning(api.Tune.DN_LAYOUT, lay)
            hdr = r.denoise(hdr=True, **params).reshape(-1, 4)
            px = r.download(api.RT_BUF_PIXELS)
            if case is None:
                case = cs.SpatialCase(W, H, tris, r.download(api.RT_BUF_DENOISE_GUIDE), eye, rg, acc)
            if ref is None:
                ref = denoise_ref.denoise(W, H, tris, case.vis, eye, rg["up"][0], acc, **params)
            assert _eq_bits(hdr, ref), f"{name}: {_differing(hdr, ref, W)}"
            case.compare(name, hdr, **params)
            assert _eq_bits(r.download(api.RT_BUF_ACCUMULATION), acc), f"{name}: rt_denoise changed the accumulation buffer"
            r.upload(api.RT_BUF_ACCUMULATION, hdr)
            r.tone_mapping()
            assert _eq_bits(r.download(api.RT_BUF_PIXELS), px), f"{name}: rt_tone_mapping(RT_BUF_DENOISED) != rt_denoise's pixels"
            r.upload(api.RT_BUF_ACCUMULATION, acc)
    assert (acc[:, 3] == 0).any() and case.reference(iterations=0)["part"].any()
    r.close()


def _temporal_sequence(api, tris, W, H, name, alphas=(0.2, 0.2), layouts=(0, 1), iterations=5):
    ap = dict(alpha_color=alphas[0], alpha_moments=alphas[1])
    rs = [_renderer(api, tris, W, H, layout=lay) for lay in layouts]
    T = dtr.TemporalRef(W, H, tris, **ap)
    static = name == "static"
    pose_set = None
    for k, pose in enumerate(cs.sequence(name, W, H), start=1):
        acc = cs.accumulation(W, H, 1000 * W + k, empty_seed=7 if static else None)
        prev, ref = cs.prev_state(T), None
        for lay, r in zip(layouts, rs):
            what = f"{name} {W} x {H} {alphas} call {k} layout {lay}"
            if pose != pose_set:
                r.lookat(pose[0], pose[1])
            r.upload(api.RT_BUF_ACCUMULATION, acc)
            hdr = r.denoise_temporal(hdr=True, iterations=iterations, **ap).reshape(-1, 4)
            mom = r.download(api.RT_BUF_DENOISE_HISTORY)
            if ref is None:
                vis, eye, rg = r.download(api.RT_BUF_DENOISE_GUIDE), r.camera_pose()[0], r.raygen()
                ref = T(vis, eye, rg, acc, iterations=iterations)
                call = cs.TemporalCall(W, H, tris, vis, eye, rg, acc, prev, iterations=iterations, **ap)
            assert _eq_bits(hdr, ref[0]), f"{what}: image: {_differing(hdr, ref[0], W)}"
            assert _eq_bits(mom, ref[1]), f"{what}: history: {_differing(mom, ref[1], W)}"
            assert _eq_bits(r.download(api.RT_BUF_ACCUMULATION), acc), f"{what}: rt_denoise_temporal changed the accumulation buffer"
            call.compare(what, hdr, mom)
            if static:
                assert call.part.sum() > W * H // 2 and (mom[call.part, 2] == min(k, 32)).all(), (what, np.unique(mom[:, 2]))
        pose_set = pose
    for r in rs:
        r.close()


@pytest.mark.parametrize("name", ["sideways", "dolly", "turn", "half_turn"])
def test_temporal_camera_sequences(api, tris, name):
    _temporal_sequence(api, tris, 40, 33, name)


@pytest.mark.parametrize("alphas", [(0.2, 0.2), (0.05, 0.5)])
def test_temporal_static_36_calls(api, tris, alphas):
    _temporal_sequence(api, tris, 40, 33, "static", alphas=alphas)


@pytest.mark.parametrize("W,H,name", [(8, 8, "sideways"), (19, 7, "dolly")])
def test_temporal_tiny_images(api, tris, W, H, name):
    _temporal_sequence(api, tris, W, H, name)
