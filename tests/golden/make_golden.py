"""Generates the committed golden fixtures from the REFERENCE'S OWN code.

Run in the build container only (needs /root/reference and oracle/_ref/ref_kernels, i.e.
`make -C oracle`):   python tests/golden/make_golden.py

Outputs (data only — inputs and expected outputs, no reference source):
  scenes.npz        triangle arrays of assets/cornellbox1.obj / cornellbox2.obj as the reference's
                    loader orders them (own OBJ reader, counts pinned in tests), MIT-licensed assets
  ref_kat.json      integer / struct-size known answers printed by the reference's functions
  ref_functions.npz random inputs + outputs of the reference's inline functions (glibc math)
  ref_kernels.npz   inputs + outputs of the reference's kernels run on the host at 48x27:
                    04_ao kernelMain, generate_candidate (no visibility reuse here: ref_rays.npz has it),
                    temporal_resampling, 3 x spatial_resampling, tone_mapping
  ref_ao04_256.npz  BASELINE config #1 at its real size: 04_ao kernelMain, cornellbox1.obj, 256x256 (RGBA8)
  ref_camera.npz    the reference's CameraControl (common/misc.hpp:108-224) + RayGenerator::lookat over
                    sequences of random orbit / zoom / pan drags: eye, look-at, updated flag, raygen bits
  ref_tinyobj.npz   triangle arrays the reference's vendored tinyobjloader + common/loader.hpp:25-64 loop
                    produce for assets/cornellbox1.obj and assets/blocks_ao.obj
  assets/           those two OBJ/MTL pairs themselves (MIT-licensed data files of the reference, (c) 2024
                    Kenta Eto, see assets/ATTRIBUTION): the INPUTS of the OBJ-reader test on the GPU box
  ref_rays.npz     the reference's RAY-USING kernels run on the host over the intersection by definition of
                    oracle/ref_driver.cpp (48x27): raycast, generate_candidate with visibility reuse / the shadowed target
                    function, temporal + 3 x spatial with the shadowed target function, resolve, path_trace of 07_pt /
                    08_nee / 09_ris, 06_ao_hiprt next to 04_ao; scenes: cornellbox1/2, make_quad_room, thin
                    make_blocks_restir / make_blocks_pt, blocks_ao.obj, three seeded triangle soups (stored)
  ref_rays_chain.npz  frame chains (raycast -> ... -> resolve -> tone_mapping) through the reference's kernels only
  ref_wide_pin.npz SHA-256 digests (per field, shaded pixels) of the reference's temporal + spatial kernels on the
                    211 916-triangle bench stand-in at 240x135 over a 26-frame history (M reaches the 640 clamp)
The oracle (MATH_LIBM mode) must reproduce every output bit for bit: tests/test_oracle_golden.py and
tests/test_oracle_reference_rays.py. `python tests/golden/make_golden.py --only-rays` writes the last three only.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from cedec_2024_rt_amd import scenes  # noqa: E402
from oracle import binding as ob  # noqa: E402

REF = "/root/reference"


def resolve_inputs(rng, n):
    """operands of resolve's arithmetic (10_restir_di.cu:433-458) as a frame has them: Kd in [0,1], surface / light positions a few
    units apart, unit normals, radiance up to 120 (assets/blocks_restir.mtl Ke), ucw from tiny to large, V in {0, 1} (and a few other
    values: the expression multiplies by it), both accumulate settings, previous accumulation values, plus zeros / coincident points"""
    x = np.zeros((n, 25), np.float32)
    x[:, 0:3] = rng.random((n, 3), dtype=np.float32)
    x[:, 3:6] = (rng.random((n, 3), dtype=np.float32) * 40 - 20).astype(np.float32)
    nn = rng.standard_normal((n, 3)).astype(np.float32)
    x[:, 6:9] = nn / np.linalg.norm(nn, axis=1, keepdims=True).astype(np.float32)
    x[:, 9:12] = x[:, 3:6] + (rng.standard_normal((n, 3)) * np.float32(6)).astype(np.float32)
    nn = rng.standard_normal((n, 3)).astype(np.float32)
    x[:, 12:15] = nn / np.linalg.norm(nn, axis=1, keepdims=True).astype(np.float32)
    x[:, 15:18] = (rng.random((n, 3), dtype=np.float32) * np.float32(120)).astype(np.float32)
    x[:, 18] = np.exp(rng.random(n) * 30 - 20).astype(np.float32)
    x[:, 19] = (rng.random(n) < 0.7).astype(np.float32)
    x[::17, 19] = rng.random(len(x[::17]), dtype=np.float32)
    x[:, 20] = (rng.random(n) < 0.5).astype(np.float32)
    x[:, 21:24] = (rng.random((n, 3), dtype=np.float32) * np.float32(50)).astype(np.float32)
    x[:, 24] = np.floor(rng.random(n) * 64).astype(np.float32)
    x[::29, 9:12] = x[::29, 3:6]      # light sample on the surface point: G = 0/0
    x[::31, 18] = 0.0                 # ucw = 0 (p_hat = 0)
    x[::37, 15:18] = 0.0
    return x


# ------------------------------------------------------------------ the ray-using kernels (RNG streams of their own)
FOVY = np.float32(np.pi) / np.float32(4)
RW, RH = 48, 27
WIDE_W, WIDE_H, WIDE_FRAMES, WIDE_COMPARED = 240, 135, 26, (1, 2, 13, 25, 26)
WIDE_VARIANTS = dict(no_temporal=dict(use_temporal_resampling=0), no_spatial=dict(use_spatial_resampling=0),
                     passes2=dict(spatial_resampling_passes=2), samples7=dict(spatial_resampling_sample_count=7))
RESOLVE_VARIANTS = ("acc0", "acc1")
# (key, example, option overrides); frame = 3; every case has a sky colour != 0
PT_CASES = [(f"pt{ex}_d{d}", ex, dict(max_depth=d)) for ex in (7, 8, 9) for d in (1, 2, 6)] + [
    ("pt9_ris1", 9, dict(ris_sample_count=1)), ("pt9_shadowed", 9, dict(use_shadowed_target_function=1)),
    ("pt9_ris1_shadowed", 9, dict(ris_sample_count=1, use_shadowed_target_function=1))]
PT_SKY = (0.25, 0.5, 0.75)
_PT = {c[0]: c for c in PT_CASES}
PT_SCENE_CASES = [("c2", c) for c in PT_CASES] + [("quad", _PT[c]) for c in ("pt7_d6", "pt8_d6", "pt9_d6")] + [
    ("blocks_pt", _PT[c]) for c in ("pt7_d6", "pt8_d2")] + [("soup1", _PT[c]) for c in ("pt7_d6", "pt9_d2", "pt8_d6")] + [
    ("soup2", _PT[c]) for c in ("pt7_d2", "pt8_d2", "pt9_d6")]
GEN_VARIANTS = dict(reuse=dict(use_visibility_reuse=1, use_shadowed_target_function=0),
                    shadowed=dict(use_visibility_reuse=0, use_shadowed_target_function=1),
                    both=dict(use_visibility_reuse=1, use_shadowed_target_function=1))


def soup(seed, n):
    """a seeded triangle soup like those of test_random_triangle_soups_differential, with the definition's sharp edges:
    exact duplicates and a coplanar patch (t ties -> highest index), degenerate and collinear triangles (t = nan), triangles
    seen edge-on from the camera at the origin side, and a few emitters"""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, ob.TRIANGLE)
    c = rng.normal(size=(n, 1, 3)).astype(np.float32) * np.float32(3.0)
    size = np.float32(10.0) ** rng.uniform(-1.0, 0.7, size=(n, 1, 1)).astype(np.float32)
    t["v"] = (c + rng.normal(size=(n, 3, 3)).astype(np.float32) * size).astype(np.float32)
    k = n // 8
    t["v"][:k, 1] = t["v"][:k, 0]
    t["v"][k:2 * k, 2] = (t["v"][k:2 * k, 0] + (t["v"][k:2 * k, 1] - t["v"][k:2 * k, 0]) * np.float32(0.5)).astype(np.float32)
    t["v"][2 * k:3 * k] = t["v"][3 * k:4 * k]
    t["v"][4 * k:5 * k, :, 1] = np.float32(-2.0)
    t["v"][5 * k:6 * k, :, 0] = np.float32(0.0)  # in the plane x = 0, which holds the eye of SOUP_EYE: edge-on
    t["color"] = rng.random((n, 3), dtype=np.float32)
    lit = (rng.random(n) < 0.1) & (np.arange(n) >= 2 * k)  # no emitter of area 0: sample_light would divide by it
    t["emissive"][lit] = (rng.random((int(lit.sum()), 3), dtype=np.float32) * np.float32(20.0) + np.float32(1.0)).astype(np.float32)
    return t


SOUP_EYE, SOUP_AT = (0.0, 1.0, 9.0), (0.0, 0.0, 0.0)


def ray_scenes(assets_dir):
    """name -> (triangles, eye, look-at). The soups travel inside the fixture; the others are rebuilt by the tests."""
    g = np.load(os.path.join(HERE, "scenes.npz"))
    return dict(
        c1=(g["cornellbox1"], scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT),
        c2=(g["cornellbox2"], (0.3, 2.9, 6.2), (0.0, 2.5, -2.8)),
        quad=(scenes.make_quad_room(), (0.5, 2.5, 6.0), (0.0, 1.5, -1.0)),
        blocks_restir=(scenes.make_blocks_restir(detail=0.02), scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT),
        blocks_pt=(scenes.make_blocks_pt(detail=0.02), scenes.BLOCKS_PT_EYE, scenes.BLOCKS_PT_LOOKAT),
        blocks_ao=(scenes.load_obj(os.path.join(assets_dir, "blocks_ao.obj")), scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT),
        soup0=(soup(41001, 96), SOUP_EYE, SOUP_AT), soup1=(soup(41002, 240), SOUP_EYE, SOUP_AT), soup2=(soup(41003, 400), SOUP_EYE, SOUP_AT))


def shaded_mask(vis, tris):
    idx = vis["index"]
    return (idx >= 0) & ~np.isin(idx, scenes.light_indices(tris))


def pack_trace(tr):
    return tr.astype(np.int32)


def digest(res, mask):
    """SHA-256 per field over the masked pixels (padding bytes left out)"""
    return {f: hashlib.sha256(np.ascontiguousarray(res[f][mask]).tobytes()).hexdigest() for f in res.dtype.names if f != "pad"}


def resolve_reservoirs(rng, res, shaded):
    """reservoirs for the resolve cases: the kernels' own output with some ucw = 0 (p_hat = 0, 10_restir_di.cu:121) among them"""
    r = res.copy()
    r["pad"] = 0
    z = shaded & (rng.random(len(r)) < 0.1)
    r["ucw"][z] = 0.0
    r[~shaded] = np.zeros(1, ob.RESERVOIR)
    return r


def make_rays():
    ob.set_math_mode(ob.MATH_LIBM)
    W, H = RW, RH
    sc = ray_scenes(os.path.join(HERE, "assets"))
    k = dict(W=W, H=H)
    cam = {}
    for name, (tris, eye, at) in sc.items():
        rg = ob.raygen_lookat(eye, at, (0, 1, 0), FOVY, W, H)
        cam[name] = (rg, np.asarray(eye, np.float32), ob.Scene(tris, use_bvh=False).lights)
        k[name + "_sha"] = np.array(scenes.scene_sha256(tris))
        k[name + "_raygen"] = rg
        if name.startswith("soup"):
            k[name + "_tris"] = tris
    # raycast: index flip, the miss value, uv
    vis = {}
    for name in ("c1", "c2", "quad", "blocks_restir", "soup0", "soup1", "soup2"):
        vis[name], tr = ob.ref_raycast(W, H, sc[name][0], cam[name][0])
        vis[name]["pad"] = 0
        k[name + "_vis"] = vis[name]
    # generate_candidate: visibility reuse, the shadowed target function, both (frame 1); the unshadowed, reuse-less run too
    for name in ("c2", "quad", "blocks_restir"):
        tris, (rg, eye, lights) = sc[name][0], cam[name]
        sh = shaded_mask(vis[name], tris)
        plain, _ = ob.ref_generate_candidate(W, H, 1, tris, vis[name], eye, ob.bench_options(use_visibility_reuse=0), lights)
        for vname, kw in GEN_VARIANTS.items():
            if name == "blocks_restir" and vname != "both":
                continue
            r, tr = ob.ref_generate_candidate(W, H, 1, tris, vis[name], eye, ob.bench_options(**kw), lights)
            r["pad"] = 0
            assert not r[~sh].view(np.uint8).any()  # Reservoir{} (10_restir_di.cu:59,68)
            k[f"{name}_gen_{vname}"] = r[sh]
            k[f"{name}_gen_{vname}_shadow"] = np.array([tr[:, 2].sum(), tr[:, 3].sum()])
            k[f"{name}_gen_{vname}_differs"] = np.array(int((r[sh]["ucw"].view(np.uint32) != plain[sh]["ucw"].view(np.uint32)).sum()))
    # temporal + 3 x spatial with the shadowed target function (and visibility reuse), frame 2, history = frame 1
    for name in ("c2", "quad"):
        tris, (rg, eye, lights) = sc[name][0], cam[name]
        sh = shaded_mask(vis[name], tris)
        opt = ob.bench_options(use_shadowed_target_function=1)
        plain = ob.bench_options(use_shadowed_target_function=0)
        g1, _ = ob.ref_generate_candidate(W, H, 1, tris, vis[name], eye, opt, lights)
        g2, _ = ob.ref_generate_candidate(W, H, 2, tris, vis[name], eye, opt, lights)
        differs = []
        rin, tr = ob.ref_temporal_resampling(W, H, 2, tris, vis[name], eye, opt, g1, g2)
        rays = [tr[:, 0].sum()]
        other, _ = ob.ref_temporal_resampling(W, H, 2, tris, vis[name], eye, plain, g1, g2)
        differs.append(int((rin[sh]["ucw"].view(np.uint32) != other[sh]["ucw"].view(np.uint32)).sum()))
        rin["pad"] = 0
        k[f"{name}_shadowed_temporal"] = rin[sh]
        for p in range(3):
            out, tr = ob.ref_spatial_resampling(W, H, 2, p, tris, vis[name], eye, opt, rin)
            other, _ = ob.ref_spatial_resampling(W, H, 2, p, tris, vis[name], eye, plain, rin)
            differs.append(int((out[sh]["ucw"].view(np.uint32) != other[sh]["ucw"].view(np.uint32)).sum()))
            rays.append(tr[:, 0].sum())
            out["pad"] = 0
            k[f"{name}_shadowed_spatial{p}"] = out[sh]
            out[~sh] = np.zeros(1, ob.RESERVOIR)
            rin = out
        k[f"{name}_shadowed_differs"] = np.array(differs)
        k[f"{name}_shadowed_rays"] = np.array(rays)
        # resolve on the candidates of frame 1 with visibility reuse (samples the shadow ray rejects keep ucw > 0 there), some
        # ucw = 0, unshaded pixels; accumulate off and on
        rng = np.random.default_rng(20261016 + len(name))
        cand, _ = ob.ref_generate_candidate(W, H, 1, tris, vis[name], eye, ob.bench_options(), lights)
        res = resolve_reservoirs(rng, cand, sh)
        acc = (rng.random((W * H, 4), dtype=np.float32) * np.float32(3.0)).astype(np.float32)
        acc[:, 3] = np.floor(rng.random(W * H) * 9).astype(np.float32)
        k[f"{name}_resolve_res"] = res[sh]
        k[f"{name}_resolve_prev"] = acc
        for a in (0, 1):
            out, tr = ob.ref_resolve(W, H, tris, vis[name], eye, ob.bench_options(accumulate=a), res, acc)
            k[f"{name}_resolve_acc{a}"] = out
            k[f"{name}_resolve_shadow"] = np.array([tr[:, 2].sum(), tr[:, 3].sum()])
            # pixels where the ray's answer decides the result: it hit, and everything else in the product is > 0
            k[f"{name}_resolve_decided_by_V"] = np.array(int(((tr[:, 2] == 1) & (res["ucw"] > 0) & sh).sum()))
    # path tracers
    for name, (key, ex, kw) in PT_SCENE_CASES:
        tris, (rg, eye, lights) = sc[name][0], cam[name]
        opt = ob.default_options(sky_color=PT_SKY, **kw)
        out, tr = ob.ref_path_trace(ex, W, H, 3, tris, rg, opt, np.zeros((W * H, 4), np.float32), lights)
        k[f"{name}_{key}"] = out[:, :3].copy()
        assert (out[:, 3] == 1.0).all()
        k[f"{name}_{key}_trace"] = pack_trace(tr)
    # accumulate over 3 frames, from a cleared buffer
    for ex in (7, 8, 9):
        tris, (rg, eye, lights) = sc["c2"][0], cam["c2"]
        acc = np.zeros((W * H, 4), np.float32)
        rays = []
        for fr in (1, 2, 3):
            acc, tr = ob.ref_path_trace(ex, W, H, fr, tris, rg, ob.default_options(sky_color=PT_SKY, accumulate=1), acc, lights)
            rays.append(tr[:, 0].sum())
        k[f"c2_pt{ex}_accumulate3"] = acc
        k[f"c2_pt{ex}_accumulate3_rays"] = np.array(rays)
    # 06_ao_hiprt next to 04_ao
    for name in ("blocks_ao", "c1", "soup0", "soup2"):
        tris, (rg, eye, lights) = sc[name][0], cam[name]
        k[f"{name}_ao04"] = ob.ref_ao(4, W, H, tris, rg)
        k[f"{name}_ao06"] = ob.ref_ao(6, W, H, tris, rg)
    np.savez_compressed(os.path.join(HERE, "ref_rays.npz"), **k)

    # frame chains through the reference's kernels only
    c = dict(W=W, H=H)
    for name, kw, frames in (("c2", dict(), 4), ("quad", dict(use_shadowed_target_function=1, accumulate=1), 3)):
        tris, (rg, eye, lights) = sc[name][0], cam[name]
        opt = ob.bench_options(**kw)
        st = ob.new_state(W, H)
        for fr in range(1, frames + 1):
            rays = ob.ref_frame(W, H, fr, tris, rg, eye, opt, lights, st)
            c[f"{name}_frame{fr}_accum"] = st["accum"].copy()
            c[f"{name}_frame{fr}_pixels"] = st["pixels"].copy()
            c[f"{name}_frame{fr}_rays"] = np.array(rays)
            for b in ("r0", "r1"):  # what the next frame's kernels never read
                st[b][~shaded_mask(st["vis"], tris)] = np.zeros(1, ob.RESERVOIR)
        c[name + "_options"] = opt
        c[name + "_frames"] = np.array(frames)
        c[name + "_final_M"] = st["r1"]["M"].astype(np.int16)
    np.savez_compressed(os.path.join(HERE, "ref_rays_chain.npz"), **c)


def wide_chain(variant_kw, frames, compared, run_temporal, run_spatial, tris, vis, eye, candidates, history=None, first=1):
    """temporal + spatial passes over `frames` frames with the given kernels; returns {(frame, stage): reservoirs}, the last history"""
    W, H = WIDE_W, WIDE_H
    opt = ob.bench_options(**variant_kw)
    hist = np.zeros(W * H, ob.RESERVOIR) if history is None else history
    sh = shaded_mask(vis, tris)
    out = {}
    for fr in range(first, first + frames):
        t = run_temporal(W, H, fr, tris, vis, eye, opt, hist, candidates(fr))
        hist = t.copy()
        if fr in compared:
            out[(fr, "temporal")] = t
        rin = t
        for p in range(int(opt["spatial_resampling_passes"][0])):
            if fr not in compared:
                break  # the spatial passes feed nothing back (10_restir_di.cpp:314-321 saves the temporal output)
            o = run_spatial(W, H, fr, p, tris, vis, eye, opt, rin)
            o[~sh] = np.zeros(1, ob.RESERVOIR)
            out[(fr, f"spatial{p}")] = o
            rin = o
    return out, hist


def make_wide():
    """VERDICT next-step 2: the reference's temporal + spatial kernels on the bench stand-in, bench options (visibility reuse on),
    a history long enough for M to reach min(M, 20 * 32). The candidates come from the oracle (its generate_candidate is pinned
    by ref_rays.npz); no ray is needed in the reference's run."""
    ob.set_math_mode(ob.MATH_LIBM)
    W, H = WIDE_W, WIDE_H
    tris = scenes.make_blocks_restir()
    sc = ob.Scene(tris, use_bvh=True)
    eye = np.asarray(scenes.BLOCKS_RESTIR_EYE, np.float32)
    rg = ob.raygen_lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT, (0, 1, 0), FOVY, W, H)
    vis = sc.raycast(W, H, rg)
    sh = shaded_mask(vis, tris)
    opt = ob.bench_options()
    cand = lambda fr: sc.generate_candidate(W, H, fr, vis, eye, opt)  # noqa: E731
    rt = lambda *a: ob.ref_temporal_resampling(*a)[0]  # noqa: E731
    rs = lambda *a: ob.ref_spatial_resampling(*a)[0]  # noqa: E731
    w = dict(W=W, H=H, frames=WIDE_FRAMES, compared=np.array(WIDE_COMPARED), scene_sha=np.array(scenes.scene_sha256(tris)),
             shaded=np.array(int(sh.sum())))
    out, hist = wide_chain({}, WIDE_FRAMES, WIDE_COMPARED, rt, rs, tris, vis, eye, cand)
    for (fr, stage), r in out.items():
        for f, d in digest(r, sh).items():
            w[f"main_{fr}_{stage}_{f}"] = np.array(d)
    w["main_M_temporal_26"] = out[(26, "temporal")]["M"][sh].astype(np.int16)
    w["main_visibility_26"] = np.packbits(out[(26, "spatial2")]["visibility"][sh])
    for vname, kw in WIDE_VARIANTS.items():  # one frame more on the 26-frame history
        o2, _ = wide_chain(kw, 1, (27,), rt, rs, tris, vis, eye, cand, history=hist, first=27)
        for (fr, stage), r in o2.items():
            for f, d in digest(r, sh).items():
                w[f"{vname}_{fr}_{stage}_{f}"] = np.array(d)
    np.savez_compressed(os.path.join(HERE, "ref_wide_pin.npz"), **w)


def main():
    if "--only-rays" in sys.argv:
        make_rays()
        make_wide()
        return
    assert ob.have_ref(), "oracle/_ref/ref_kernels missing: make -C oracle"
    c1 = scenes.load_obj(os.path.join(REF, "assets/cornellbox1.obj"))
    c2 = scenes.load_obj(os.path.join(REF, "assets/cornellbox2.obj"))
    assert len(c1) == 36 and len(c2) == 3470
    np.savez_compressed(os.path.join(HERE, "scenes.npz"), cornellbox1=c1, cornellbox2=c2)

    with open(os.path.join(HERE, "ref_kat.json"), "w") as f:
        json.dump(ob.ref_run("kat"), f, indent=1)

    rng = np.random.default_rng(20240823)
    fn = {}
    for name, (fid, nin, nout) in ob.FN.items():
        if fid >= 20:
            continue
        if name == "resolve_arithmetic":  # (r05) a generator of its own: the fixtures of rounds 1-4 keep their random streams
            x = resolve_inputs(np.random.default_rng(20251003), 4000)
            fn[name + "_in"] = x
            fn[name + "_out"] = ob.ref_fn(name, x)
            continue
        x = rng.random((2000, nin), dtype=np.float32)
        if name == "intersect_ray_triangle":
            x = (x * 2 - 1).astype(np.float32)
            x[:, 6] = 0.0
            x[:, 7] = 1e30
        elif name in ("geometry_term", "normal_rejection", "depth_rejection", "triangle_props", "surface_ray", "tangent_world"):
            x = (x * 4 - 2).astype(np.float32)
        elif name == "aces":
            x = (x * 8).astype(np.float32)
        fn[name + "_in"] = x
        fn[name + "_out"] = ob.ref_fn(name, x)
    np.savez_compressed(os.path.join(HERE, "ref_functions.npz"), **fn)
    if "--only-functions" in sys.argv:
        return

    # kernels on cornellbox1, default camera (common/misc.hpp:217-218), 48x27
    W, H = 48, 27
    ob.set_math_mode(ob.MATH_LIBM)
    fovy = np.float32(np.pi) / np.float32(4)
    cam = np.array(list(scenes.DEFAULT_EYE) + list(scenes.DEFAULT_LOOKAT) + [0, 1, 0, fovy], dtype=np.float32)
    uv = rng.random((64, 2), dtype=np.float32)
    o = ob.ref_run("camera", cam=cam, W=W, H=H, uv=uv)
    rg = np.frombuffer(o["raygen"], dtype=ob.RAYGEN).copy()
    rays = np.frombuffer(o["rays"], dtype=np.float32).reshape(-1, 6).copy()
    eye = np.asarray(scenes.DEFAULT_EYE, dtype=np.float32)

    k = dict(W=W, H=H, raygen=rg, cam=cam, cam_uv=uv, cam_rays=rays, eye=eye)
    o = ob.ref_run("ao04", W=W, H=H, tris=c1, raygen=rg)
    k["ao04_pixels"] = np.frombuffer(o["pixels"], dtype=np.uint8).reshape(H, W, 4).copy()

    # visibility buffer: by the pinned definition (brute force of core.hpp:91-136), from the oracle. It is an INPUT of
    # the fixtures below (the reference's raycast kernel itself is recorded in ref_rays.npz).
    sc = ob.Scene(c1, use_bvh=False)
    vis = sc.raycast(W, H, rg)
    k["vis"] = vis
    opt = ob.bench_options(use_visibility_reuse=0)
    k["options"] = opt
    lights = sc.lights
    o = ob.ref_run("generate_candidate", W=W, H=H, frame=1, tris=c1, vis=vis, options=opt, eye=eye, lights=lights)
    gen1 = np.frombuffer(o["res"], dtype=ob.RESERVOIR).copy()
    o = ob.ref_run("generate_candidate", W=W, H=H, frame=2, tris=c1, vis=vis, options=opt, eye=eye, lights=lights)
    gen2 = np.frombuffer(o["res"], dtype=ob.RESERVOIR).copy()
    gen1["pad"] = 0
    gen2["pad"] = 0
    k["gen_frame1"], k["gen_frame2"] = gen1, gen2
    # frame 2: temporal with frame-1 candidates as history
    o = ob.ref_run("temporal_resampling", W=W, H=H, frame=2, tris=c1, vis=vis, options=opt, eye=eye, prev=gen1, res=gen2)
    tmp = np.frombuffer(o["res"], dtype=ob.RESERVOIR).copy()
    k["temporal_frame2"] = tmp
    rin = tmp
    for p in range(3):
        o = ob.ref_run("spatial_resampling", W=W, H=H, frame=2, tris=c1, vis=vis, options=opt, eye=eye, res=rin, **{"pass": p})
        out = np.frombuffer(o["res"], dtype=ob.RESERVOIR).copy()
        k[f"spatial_frame2_pass{p}"] = out
        rin = out
    acc = rng.random((W * H, 4), dtype=np.float32) * np.float32(4.0)
    acc[:, 3] = np.float32(1.0) + np.floor(acc[:, 3])
    o = ob.ref_run("tone_mapping", W=W, H=H, accum=acc)
    k["tone_accum"] = acc
    k["tone_pixels"] = np.frombuffer(o["pixels"], dtype=np.uint8).reshape(H, W, 4).copy()
    np.savez_compressed(os.path.join(HERE, "ref_kernels.npz"), **k)

    # BASELINE config #1 at its real size (256x256): the reference's 04_ao kernel on cornellbox1, default camera
    W2, H2 = 256, 256
    cam2 = np.array(list(scenes.DEFAULT_EYE) + list(scenes.DEFAULT_LOOKAT) + [0, 1, 0, fovy], dtype=np.float32)
    o = ob.ref_run("camera", cam=cam2, W=W2, H=H2, uv=uv)
    rg2 = np.frombuffer(o["raygen"], dtype=ob.RAYGEN).copy()
    o = ob.ref_run("ao04", W=W2, H=H2, tris=c1, raygen=rg2)
    np.savez_compressed(os.path.join(HERE, "ref_ao04_256.npz"), W=W2, H=H2, raygen=rg2,
                        pixels=np.frombuffer(o["pixels"], dtype=np.uint8).reshape(H2, W2, 4).copy())

    # interactive camera: random drag sequences from three start poses
    cam = {}
    poses = [(scenes.DEFAULT_EYE, scenes.DEFAULT_LOOKAT, 1920, 1080), (scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT, 1920, 1080),
             ((0.5, 2.5, 6.0), (0.0, 1.5, -1.0), 96, 54)]
    for i, (e0, a0, w, h) in enumerate(poses):
        ev = np.zeros((120, 3), dtype=np.float32)
        ev[:, 0] = rng.integers(0, 3, 120)
        ev[:, 1:] = (rng.normal(size=(120, 2)) * 80.0).astype(np.float32)
        ev[5] = (0, 0.0, 5000.0)   # orbit past the pole: the clamp of misc.hpp:172 keeps the old elevation
        ev[6] = (1, 0.0, 1e6)      # zoom through the look-at point: the 0.01 floor of :186
        out = ob.ref_camera_run(e0, a0, w, h, fovy, [(int(b), float(dx), float(dy)) for b, dx, dy in ev])
        cam[f"pose{i}_start"] = np.array(list(e0) + list(a0) + [w, h], dtype=np.float32)
        cam[f"pose{i}_events"] = ev
        cam[f"pose{i}_out"] = out
    cam["fovy"] = np.array([fovy], dtype=np.float32)
    np.savez_compressed(os.path.join(HERE, "ref_camera.npz"), **cam)

    # OBJ ingest: the reference's tinyobj path on two shipped scenes + the scene files themselves
    import shutil
    import subprocess
    import tempfile

    os.makedirs(os.path.join(HERE, "assets"), exist_ok=True)
    tiny = {}
    for name, count in (("cornellbox1", 36), ("blocks_ao", 3034)):
        for ext in ("obj", "mtl"):
            shutil.copyfile(os.path.join(REF, "assets", f"{name}.{ext}"), os.path.join(HERE, "assets", f"{name}.{ext}"))
        with tempfile.TemporaryDirectory() as d:
            outp = os.path.join(d, "t.tris")
            subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", "ref_tinyobj"), os.path.join(REF, "assets", name + ".obj"),
                                   os.path.join(REF, "assets") + "/", outp], stdout=subprocess.DEVNULL)
            t = np.fromfile(outp, dtype=ob.TRIANGLE)
        assert len(t) == count
        tiny[name] = t
    np.savez_compressed(os.path.join(HERE, "ref_tinyobj.npz"), **tiny)
    with open(os.path.join(HERE, "assets", "ATTRIBUTION"), "w") as f:
        f.write("cornellbox1.obj/.mtl, cornellbox2.obj/.mtl, blocks_ao.obj/.mtl and blocks_pt.mtl are data files of yumcyaWiz/CEDEC-2024-RT (assets/), MIT License,\n"
                "Copyright (c) 2024 Kenta Eto. They are test INPUTS here (OBJ reader parity on machines without the reference checkout).\n")
    make_rays()
    make_wide()
    for f in sorted(os.listdir(HERE)):
        print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
