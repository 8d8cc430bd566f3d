"""Ambient occlusion on the GPU: rt_path_trace example 6 (examples/06_ao_hiprt/06_ao_hiprt.cu:35-91) and 4
(examples/04_ao/04_ao.cu:31-88), frame_kernels.h k_ao.

* cornellbox1 at 256x256 with the default camera: every byte of the reference's own kernel output (tests/golden/ref_ao04_256.npz);
* blocks_ao.obj at 1920x1080 (BASELINE.md §1's 06_ao_hiprt row): the oracle's o_ao_04 (portable math, BVH) bit for bit, and the
  reference's ray count (2 073 600 primary rays + 64 per hit pixel);
* both layouts of rt_tuning key 27 give the same image (whole tiles and partial ones);
* random triangle soups with degenerate triangles: the any-hit walk with tmax = FLT_MAX == the brute-force closest-hit loop;
* row strips, example 4 == example 6, the accumulation buffer untouched, the error codes;
* restir_app --example 6 end to end.
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "app", "restir_app")
FOVY = np.float32(np.pi) / np.float32(4)
RT_ERR_ARG, RT_ERR_STATE = 1, 3
BLOCKS_AO_RAYS_1080P = 99_726_016  # 2 073 600 primary rays + 64 x 1 525 819 hit pixels


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def scenes():
    from cedec_2024_rt_amd import scenes as s

    return s


def _asset(golden_dir, name):
    return os.path.join(golden_dir, "assets", name)


def _renderer(api, tris, W, H, eye, at, rows=None, layout=None):
    r = api.Renderer(W, H, rows=rows)
    r.set_scene(tris)
    r.lookat(eye, at)
    if layout is not None:
        r.tuning(api.Tune.AO_LAYOUT, layout)
    return r


def _oracle_ao(oracle, tris, W, H, eye, at, use_bvh=True):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    sc = oracle.Scene(tris, use_bvh=use_bvh)
    rg = oracle.raygen_lookat(eye, at, (0, 1, 0), FOVY, W, H)
    return np.asarray(sc.ao_04(W, H, rg)).reshape(H, W, 4)


def _diff(a, b):
    return int((a != b).any(axis=-1).sum())


def _ray_count(px):
    H, W = px.shape[:2]
    return W * H + 64 * int((px[..., 0] != 32).sum())  # 32 is no hit value: 0/64 -> 0, 1/64 -> 38


@pytest.fixture(scope="module")
def blocks_ao(scenes, oracle, golden_dir):
    W, H = 1920, 1080
    tris = scenes.load_obj(_asset(golden_dir, "blocks_ao.obj"))
    ref = _oracle_ao(oracle, tris, W, H, scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT, use_bvh=True)
    return tris, W, H, ref


def test_cornellbox1_256_is_the_reference_kernel(api, oracle, scenes, golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_ao04_256.npz"))
    W, H = int(g["W"]), int(g["H"])
    tris = scenes.load_obj(_asset(golden_dir, "cornellbox1.obj"))
    r = _renderer(api, tris, W, H, scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT)
    assert r.raygen().tobytes() == g["raygen"].tobytes()
    px = r.ambient_occlusion()
    assert px.shape == (H, W, 4) and px.dtype == np.uint8
    assert np.array_equal(px, g["pixels"]), f"{_diff(px, g['pixels'])} pixels differ from the reference's kernel"
    assert np.array_equal(px, _oracle_ao(oracle, tris, W, H, scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT))
    assert r.path_trace_rays() == _ray_count(px)
    assert (px[..., 0] != 32).mean() > 0.1 and (px[..., 3] == 255).all()
    r.close()


def test_blocks_ao_1080p_equals_the_oracle(api, scenes, blocks_ao):
    tris, W, H, ref = blocks_ao
    r = _renderer(api, tris, W, H, scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT)
    assert r.scene_info()["lights"] == 0  # AO needs no emissive triangle
    px = r.ambient_occlusion(6)
    assert np.array_equal(px, ref), f"{_diff(px, ref)} pixels differ from o_ao_04"
    assert int((ref[..., 0] != 32).sum()) == 1_525_819
    assert r.path_trace_rays() == _ray_count(px) == BLOCKS_AO_RAYS_1080P
    r.close()


def test_both_layouts_give_the_same_image(api, oracle, scenes, golden_dir, blocks_ao):
    tris, W, H, ref = blocks_ao
    for layout in (0, 1):
        r = _renderer(api, tris, W, H, scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT, layout=layout)
        assert r.tuning_get(api.Tune.AO_LAYOUT) == layout
        px = r.ambient_occlusion()
        assert np.array_equal(px, ref), f"layout {layout}: {_diff(px, ref)} pixels differ"
        assert r.path_trace_rays() == BLOCKS_AO_RAYS_1080P
        r.close()
    # an odd size: partial tiles at the right and bottom edges
    W, H = 333, 197
    ref = _oracle_ao(oracle, tris, W, H, scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT)
    for layout in (0, 1):
        r = _renderer(api, tris, W, H, scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT, layout=layout)
        px = r.ambient_occlusion()
        assert np.array_equal(px, ref), f"{W}x{H} layout {layout}: {_diff(px, ref)} pixels differ"
        assert r.path_trace_rays() == _ray_count(ref)
        r.close()
    r = api.Renderer(64, 48)
    for bad in (-1, 2):
        with pytest.raises(api.RtError):
            r.tuning(api.Tune.AO_LAYOUT, bad)
    r.close()


@pytest.mark.parametrize("seed", range(6))
def test_random_triangle_soups_equal_brute_force(api, oracle, seed):
    from cedec_2024_rt_amd.types import TRIANGLE

    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(8, 500))
    tris = np.zeros(n, TRIANGLE)
    c = rng.normal(size=(n, 1, 3)).astype(np.float32) * np.float32(3.0)
    size = np.float32(10.0) ** rng.uniform(-2.0, 0.7, size=(n, 1, 1)).astype(np.float32)
    tris["v"] = (c + rng.normal(size=(n, 3, 3)).astype(np.float32) * size).astype(np.float32)
    k = n // 8
    tris["v"][:k, 1] = tris["v"][:k, 0]  # degenerate: two equal vertices
    tris["v"][k:2 * k, 2] = (tris["v"][k:2 * k, 0] + (tris["v"][k:2 * k, 1] - tris["v"][k:2 * k, 0]) * np.float32(0.5)).astype(np.float32)  # collinear
    tris["v"][2 * k:3 * k] = tris["v"][3 * k:4 * k]  # exact duplicates
    tris["v"][4 * k:5 * k, :, 1] = np.float32(-2.0)  # a coplanar patch: exact t ties
    tris["color"] = rng.random((n, 3), dtype=np.float32)
    W, H = int(rng.integers(20, 120)), int(rng.integers(12, 90))
    eye = tuple(float(v) for v in rng.normal(size=3) * 6.0)
    at = tuple(float(v) for v in rng.normal(size=3))
    ref = _oracle_ao(oracle, tris, W, H, eye, at, use_bvh=False)  # 04_ao.cu:8-29: every triangle, in order
    for layout in (0, 1):
        r = _renderer(api, tris, W, H, eye, at, layout=layout)
        px = r.ambient_occlusion()
        assert np.array_equal(px, ref), f"seed {seed} layout {layout}: {_diff(px, ref)} pixels differ from brute force"
        assert r.path_trace_rays() == _ray_count(ref)
        r.close()


def test_strips_examples_buffers_and_errors(api, scenes, golden_dir):
    W, H = 200, 150
    tris = scenes.load_obj(_asset(golden_dir, "blocks_ao.obj"))
    eye, at = scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT
    whole = _renderer(api, tris, W, H, eye, at)
    acc0 = np.random.default_rng(3).random((W * H, 4), dtype=np.float32)
    whole.upload(api.RT_BUF_ACCUMULATION, acc0)
    full = whole.ambient_occlusion(6)
    assert np.array_equal(whole.download(api.RT_BUF_ACCUMULATION).view(np.uint32), acc0.view(np.uint32)), "AO wrote the accumulation buffer"
    assert np.array_equal(whole.ambient_occlusion(4), full), "04_ao and 06_ao_hiprt differ"
    whole.path_trace(6, 17)  # the frame number plays no part
    assert np.array_equal(whole.download(api.RT_BUF_PIXELS).view(np.uint8).reshape(H, W, 4), full)
    assert whole.path_trace_rays() == _ray_count(full)
    # three row strips (storage rows), concatenated == the whole image; each counts its own rays
    parts, rays = [], 0
    for rows in ((0, 41), (41, 100), (100, H)):
        s = _renderer(api, tris, W, H, eye, at, rows=rows)
        p = s.ambient_occlusion()
        assert p.shape == (rows[1] - rows[0], W, 4)
        parts.append(p)
        rays += s.path_trace_rays()
        s.close()
    assert np.array_equal(np.concatenate(parts), full)
    assert rays == _ray_count(full)
    # example 5 (05_ao_boundingbox) is not built; the path tracers' checks are unchanged
    assert whole.L.rt_path_trace(whole.h, 5, 1) == RT_ERR_ARG
    with pytest.raises(ValueError):
        whole.ambient_occlusion(5)
    whole.close()
    empty = api.Renderer(64, 48)
    assert empty.L.rt_path_trace(empty.h, 6, 0) == RT_ERR_STATE  # no scene, no camera
    empty.close()


def test_restir_app_example6_writes_the_reference_bytes(tmp_path, golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_ao04_256.npz"))
    out = os.path.join(str(tmp_path), "ao06.raw")
    cmd = [APP, "--example", "6", "--size", "256", "256", "--obj", _asset(golden_dir, "cornellbox1.obj"), "--rgba", out, "--frames", "3"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "06_ao_hiprt 256x256" in p.stdout and "Mray/s" in p.stdout, p.stdout
    px = np.fromfile(out, np.uint8).reshape(256, 256, 4)
    assert np.array_equal(px, g["pixels"]), f"{_diff(px, g['pixels'])} pixels differ from the reference kernel"
