"""The HIP kernels against what the REFERENCE'S OWN ray-using kernels recorded (tests/golden/ref_rays.npz, ref_rays_chain.npz,
ref_wide_pin.npz; made by tests/golden/make_golden.py from the reference's sources over the intersection by definition of
oracle/ref_driver.cpp). Only tests/golden/ is read here.

For each fixture case the recorded inputs are uploaded, the entry point is run (rt_raycast, rt_generate_candidate,
rt_temporal_resampling, rt_spatial_resampling, rt_resolve, rt_path_trace 6-9, rt_frame) and the result is held to
  * the reference's recording, exactly, for integer / ray-only results: G-buffer index, AO bytes, M, visibility flags, which light
    sample a reservoir holds, ray counts;
  * the oracle in MATH_PORTABLE on the same inputs, bit for bit, for floats (the existing GPU contract);
  * the reference's recording within the project's libm <-> portable contract for images: relative L2 <= 1e-4.

Measured on the CPU (oracle MATH_PORTABLE vs the fixtures; the GPU equals the oracle bit for bit): raycast, generate_candidate,
temporal / spatial with the shadowed target function, resolve and both frame chains reproduce the libm recording EXACTLY (every
field, every pixel, accumulation and 8-bit pixels); 07_pt exactly in all 7 cases; 08_nee / 09_ris differ in at most 22 of 1296
pixels by an ulp or two: relative L2 <= 2.3e-9 on cornellbox2 / quad room / blocks_pt, 5.1e-8 at worst (soup1, 09_ris depth 2),
and the same ray count in every case. So the 1e-4 gate holds for the path tracers too, with four orders of magnitude to spare,
and it is asserted for every case. (One soup case tried while choosing the fixtures, 08_nee depth 6 on soup2, had a path flip
between libm and portable: relative L2 3.0e-5, a different ray count; it was replaced by depth 2 because its ray count cannot
be held exactly to the reference's, not because of the gate.)
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

L2_GATE = 1e-4  # libm <-> portable, per image


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def scenes():
    from cedec_2024_rt_amd import scenes as s

    return s


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_rays.npz"))


@pytest.fixture(scope="module")
def ray_scenes(gold, golden_dir, scenes):
    sc = mg.ray_scenes(os.path.join(golden_dir, "assets"))
    for name, (tris, _, _) in sc.items():
        assert scenes.scene_sha256(tris) == str(gold[name + "_sha"]), f"scene {name} is not the one the fixture was recorded on"
    return sc


@pytest.fixture(autouse=True)
def _portable(oracle):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    yield
    oracle.set_math_mode(oracle.MATH_PORTABLE)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-300)))


def _fields_equal(a, b):
    for f in a.dtype.names:
        if f == "pad":
            continue
        if not np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)):
            return f
    return None


INT_FIELDS = ("M", "visibility", "radiance", "hit_normal")  # integers, and copies of the light triangle's data: which sample was kept


def _ints_equal(got, want):
    for f in INT_FIELDS:
        if not np.array_equal(np.ascontiguousarray(got[f]).view(np.uint8), np.ascontiguousarray(want[f]).view(np.uint8)):
            return f
    return None


def _open(api, oracle, gold, ray_scenes, name, opt):
    """one context per case: the fixture's scene, camera (rt_camera_set with the recorded raygen) and options"""
    tris, eye, at = ray_scenes[name]
    W, H = int(gold["W"]), int(gold["H"])
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.set_raygen(gold[name + "_raygen"], eye)
    r.set_options(opt)
    sc = oracle.Scene(tris, use_bvh=True)
    return r, sc, tris, gold[name + "_raygen"], np.asarray(eye, np.float32), W, H


def _expand(rows, shaded, oracle):
    r = np.zeros(len(shaded), oracle.RESERVOIR)
    r[shaded] = rows
    return r


@pytest.mark.parametrize("name", ["c1", "c2", "quad", "blocks_restir", "soup0", "soup1", "soup2"])
def test_raycast(api, oracle, gold, ray_scenes, name):
    r, sc, tris, rg, eye, W, H = _open(api, oracle, gold, ray_scenes, name, oracle.bench_options())
    r.raycast()
    vis = r.download(api.RT_BUF_VISIBILITY)
    want = gold[name + "_vis"]
    assert np.array_equal(vis["index"], want["index"]), f"{(vis['index'] != want['index']).sum()} pixels differ from the reference's raycast"
    o = sc.raycast(W, H, rg)
    assert np.array_equal(_bits(vis["uv"]), _bits(o["uv"])) and np.array_equal(vis["index"], o["index"])
    assert np.array_equal(_bits(vis["uv"]), _bits(want["uv"])), "uv is divisions only: the same in libm and portable math"
    r.close()


@pytest.mark.parametrize("name,variant", [("c2", "reuse"), ("c2", "shadowed"), ("c2", "both"), ("quad", "reuse"), ("quad", "shadowed"),
                                          ("quad", "both"), ("blocks_restir", "both")])
def test_generate_candidate(api, oracle, gold, ray_scenes, name, variant):
    opt = oracle.bench_options(**mg.GEN_VARIANTS[variant])
    r, sc, tris, rg, eye, W, H = _open(api, oracle, gold, ray_scenes, name, opt)
    vis = gold[name + "_vis"]
    shaded = mg.shaded_mask(vis, tris)
    r.upload(api.RT_BUF_VISIBILITY, vis)
    r.generate_candidate(1, api.RT_RES_0)
    got = r.download(api.RT_BUF_RES_0)
    want = gold[f"{name}_gen_{variant}"]
    assert _ints_equal(got[shaded], want) is None, f"differs from the reference: {_ints_equal(got[shaded], want)}"
    assert not got[~shaded].view(np.uint8).any()
    assert _fields_equal(got, sc.generate_candidate(W, H, 1, vis, eye, opt)) is None
    assert _rel_l2(got[shaded]["ucw"], want["ucw"]) <= L2_GATE and _rel_l2(got[shaded]["w_sum"], want["w_sum"]) <= L2_GATE
    r.close()


@pytest.mark.parametrize("name", ["c2", "quad"])
def test_shadowed_temporal_spatial(api, oracle, gold, ray_scenes, name):
    opt = oracle.bench_options(use_shadowed_target_function=1)
    r, sc, tris, rg, eye, W, H = _open(api, oracle, gold, ray_scenes, name, opt)
    vis = gold[name + "_vis"]
    shaded = mg.shaded_mask(vis, tris)
    r.upload(api.RT_BUF_VISIBILITY, vis)
    g1 = _expand(gold[f"{name}_gen_both"], shaded, oracle)  # the reference's own frame-1 candidates as the history
    r.upload(api.RT_BUF_RES_TEMPORAL, g1)
    r.generate_candidate(2, api.RT_RES_0)
    o = sc.generate_candidate(W, H, 2, vis, eye, opt)
    r.temporal_resampling(2, api.RT_RES_TEMPORAL, api.RT_RES_0)
    sc.temporal_resampling(W, H, 2, vis, eye, opt, g1, o)
    got = r.download(api.RT_BUF_RES_0)
    assert _ints_equal(got[shaded], gold[f"{name}_shadowed_temporal"]) is None
    assert _fields_equal(got[shaded], o[shaded]) is None
    src, dst, osrc = api.RT_RES_0, api.RT_RES_1, o
    for p in range(3):
        if p:
            src, dst = dst, src
        r.spatial_resampling(2, p, src, dst)
        odst = sc.spatial_resampling(W, H, 2, p, vis, eye, opt, osrc)
        got = r.download(api.RT_BUF_RES_0 + dst)
        want = gold[f"{name}_shadowed_spatial{p}"]
        assert _ints_equal(got[shaded], want) is None, f"pass {p}: differs from the reference"
        assert _fields_equal(got[shaded], odst[shaded]) is None, f"pass {p}"
        assert _rel_l2(got[shaded]["ucw"], want["ucw"]) <= L2_GATE
        osrc = odst
    r.close()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name", ["c2", "quad"])
def test_resolve(api, oracle, gold, ray_scenes, name, accumulate):
    opt = oracle.bench_options(accumulate=accumulate)
    r, sc, tris, rg, eye, W, H = _open(api, oracle, gold, ray_scenes, name, opt)
    vis = gold[name + "_vis"]
    shaded = mg.shaded_mask(vis, tris)
    res = _expand(gold[f"{name}_resolve_res"], shaded, oracle)
    prev = gold[f"{name}_resolve_prev"]
    r.upload(api.RT_BUF_VISIBILITY, vis)
    r.upload(api.RT_BUF_RES_1, res)
    r.upload(api.RT_BUF_ACCUMULATION, prev)
    r.resolve(api.RT_RES_1)
    acc = r.download(api.RT_BUF_ACCUMULATION).reshape(-1, 4)
    want = gold[f"{name}_resolve_acc{accumulate}"]
    o = prev.copy()
    sc.resolve(o, W, H, vis, eye, opt, res)
    assert np.array_equal(_bits(acc), _bits(o))
    assert np.array_equal(acc[:, 3], want[:, 3]) and np.array_equal(acc[:, :3] == 0, want[:, :3] == 0), "sample counts / where V = 0"
    assert _rel_l2(acc[:, :3], want[:, :3]) <= L2_GATE
    r.close()


@pytest.mark.parametrize("name,case", mg.PT_SCENE_CASES, ids=lambda v: v if isinstance(v, str) else v[0])
def test_path_trace(api, oracle, gold, ray_scenes, name, case):
    key, example, kw = case
    opt = oracle.default_options(sky_color=mg.PT_SKY, **kw)
    r, sc, tris, rg, eye, W, H = _open(api, oracle, gold, ray_scenes, name, opt)
    r.path_trace(example, 3)
    acc = r.download(api.RT_BUF_ACCUMULATION).reshape(-1, 4)
    want, trace = gold[f"{name}_{key}"], gold[f"{name}_{key}_trace"]
    o = np.zeros((W * H, 4), np.float32)
    sc.path_trace(example, W, H, 3, rg, opt, o)
    assert np.array_equal(_bits(acc), _bits(o)), f"{(acc != o).any(axis=1).sum()} pixels differ from the oracle"
    assert r.path_trace_rays() == int(trace[:, 0].sum()), "ray count of the reference's run"
    l2 = _rel_l2(acc[:, :3], want)
    print(f"{name} {key}: relative L2 to the reference's recording {l2:.3g}, {(acc[:, :3] != want).any(axis=1).sum()} pixels not bit-equal")
    assert l2 <= L2_GATE
    r.close()


@pytest.mark.parametrize("example", [7, 8, 9])
def test_path_trace_accumulate(api, oracle, gold, ray_scenes, example):
    opt = oracle.default_options(sky_color=mg.PT_SKY, accumulate=1)
    r, sc, tris, rg, eye, W, H = _open(api, oracle, gold, ray_scenes, "c2", opt)
    r.clear()
    o = np.zeros((W * H, 4), np.float32)
    for fr, rays in zip((1, 2, 3), gold[f"c2_pt{example}_accumulate3_rays"]):
        r.path_trace(example, fr)
        sc.path_trace(example, W, H, fr, rg, opt, o)
        assert r.path_trace_rays() == int(rays), f"frame {fr}"
    acc = r.download(api.RT_BUF_ACCUMULATION).reshape(-1, 4)
    want = gold[f"c2_pt{example}_accumulate3"]
    assert np.array_equal(_bits(acc), _bits(o)) and np.array_equal(acc[:, 3], want[:, 3])
    assert _rel_l2(acc[:, :3], want[:, :3]) <= L2_GATE
    r.close()


@pytest.mark.parametrize("example", [6, 4])
@pytest.mark.parametrize("name", ["blocks_ao", "c1", "soup0", "soup2"])
def test_ambient_occlusion(api, oracle, gold, ray_scenes, name, example):
    """rt_path_trace 6 == the bytes of the reference's 06_ao_hiprt kernel (and 4 == 04_ao's, which are the same bytes)"""
    r, sc, tris, rg, eye, W, H = _open(api, oracle, gold, ray_scenes, name, oracle.default_options())
    px = r.ambient_occlusion(example)
    want = gold[f"{name}_ao0{example}"]
    assert np.array_equal(px, want), f"{(px != want).any(axis=-1).sum()} pixels differ from the reference's kernel"
    assert r.path_trace_rays() == W * H + 64 * int((want[..., 0] != 32).sum())
    r.close()


@pytest.mark.parametrize("name", ["c2", "quad"])
def test_frame_chain(api, oracle, gold, ray_scenes, golden_dir, name):
    """rt_frame over the chain the reference's kernels recorded: rays and G-buffer exact, accumulation == the oracle bit for bit and
    within the gate of the recording, 8-bit pixels == the recording (they are on the CPU: measured, see the module docstring)"""
    ch = np.load(os.path.join(golden_dir, "ref_rays_chain.npz"))
    opt = ch[name + "_options"]
    r, sc, tris, rg, eye, W, H = _open(api, oracle, gold, ray_scenes, name, opt)
    st = oracle.new_state(W, H)
    for fr in range(1, int(ch[name + "_frames"]) + 1):
        final = r.frame(fr, clear_first=(fr == 1))
        sc.frame(W, H, fr, rg, eye, opt, st)
        acc = r.download(api.RT_BUF_ACCUMULATION).reshape(-1, 4)
        want = ch[f"{name}_frame{fr}_accum"]
        assert np.array_equal(_bits(acc), _bits(st["accum"])), f"frame {fr}"
        assert r.ray_count()[0] == int(ch[f"{name}_frame{fr}_rays"]), f"frame {fr}: rays of the reference's run"
        assert np.array_equal(acc[:, 3], want[:, 3]) and _rel_l2(acc[:, :3], want[:, :3]) <= L2_GATE, f"frame {fr}"
        px = r.download(api.RT_BUF_PIXELS).reshape(H, W, 4)
        assert np.array_equal(px, ch[f"{name}_frame{fr}_pixels"]), f"frame {fr}: {(px != ch[f'{name}_frame{fr}_pixels']).any(axis=-1).sum()} pixels"
    assert np.array_equal(r.download(api.RT_BUF_VISIBILITY)["index"], gold[name + "_vis"]["index"])
    shaded = mg.shaded_mask(gold[name + "_vis"], tris)
    M = r.download(api.RT_BUF_RES_0 + final)["M"]
    assert np.array_equal(M[shaded].astype(np.int16), ch[name + "_final_M"][shaded])
    r.close()


def test_wide_pin(api, oracle, scenes, golden_dir):
    """26 frames of rt_frame on the bench stand-in at 240x135, bench options: the history's M (clamped at 640, 10_restir_di.cu:185-187)
    and the visibility flags of the final reservoirs == what the reference's temporal / spatial kernels recorded, exactly"""
    w = np.load(os.path.join(golden_dir, "ref_wide_pin.npz"))
    W, H = int(w["W"]), int(w["H"])
    tris = scenes.make_blocks_restir()
    assert scenes.scene_sha256(tris) == str(w["scene_sha"])
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT)
    opt = oracle.bench_options()
    r.set_options(opt)
    for fr in range(1, int(w["frames"]) + 1):
        final = r.frame(fr, clear_first=(fr == 1))
    vis = r.download(api.RT_BUF_VISIBILITY)
    shaded = mg.shaded_mask(vis, tris)
    assert int(shaded.sum()) == int(w["shaded"])
    M = r.download(api.RT_BUF_RES_TEMPORAL)["M"][shaded]
    assert np.array_equal(M.astype(np.int16), w["main_M_temporal_26"]) and M.max() == 672
    flags = r.download(api.RT_BUF_RES_0 + final)["visibility"][shaded]
    assert np.array_equal(flags, np.unpackbits(w["main_visibility_26"])[: int(shaded.sum())])
    # and the whole state == the oracle's (portable math) after the same 26 frames
    sc = oracle.Scene(tris, use_bvh=True)
    rg = oracle.raygen_lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT, (0, 1, 0), mg.FOVY, W, H)
    eye = np.asarray(scenes.BLOCKS_RESTIR_EYE, np.float32)
    st = oracle.new_state(W, H)
    for fr in range(1, int(w["frames"]) + 1):
        sc.frame(W, H, fr, rg, eye, opt, st)
    assert _fields_equal(r.download(api.RT_BUF_RES_TEMPORAL)[shaded], st["temporal"][shaded]) is None
    assert np.array_equal(_bits(r.download(api.RT_BUF_ACCUMULATION).reshape(-1, 4)), _bits(st["accum"]))
    r.close()
