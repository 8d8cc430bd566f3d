"""The oracle (MATH_LIBM) == the REFERENCE'S OWN ray-using kernels, bit for bit.

oracle/ref_driver.cpp defines the few HIPRT members the reference's headers only declare as the project's definition of the
intersection (closest hit of the reference's intersect_ray_triangle over all triangles, [tmin, tmax]
inclusive, ties -> highest index). With it raytrace(), check_visibility() and every kernel around them run unmodified on the
host: raycast, generate_candidate with visibility reuse / the shadowed target function, temporal / spatial resampling with the
shadowed target function, resolve, the path_trace kernels of 07_pt / 08_nee / 09_ris, 06_ao_hiprt, and whole frame chains.
What this pins is every line AROUND the ray (pixel flip, miss values, the order of RNG draws, exit conditions, throughput,
NEE, RIS weights, accumulation, the M clamp, p_hat *= visibility); the intersection itself stays pinned by definition.

Fixture form: tests/golden/ref_rays.npz, ref_rays_chain.npz, ref_wide_pin.npz (tests/golden/make_golden.py). Live form (where
oracle/_ref is built): the same comparisons on other cameras, frames and seeds. Both run the oracle's brute force AND its BVH.
Every test asserts that its input is not trivial with counts taken from the reference's output (`trace`: what the intersector
recorded while the reference's kernel ran a pixel), never from the oracle's.
"""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

BVH = pytest.mark.parametrize("use_bvh", [False, True], ids=["brute", "bvh"])


@pytest.fixture(autouse=True)
def _libm(oracle):
    oracle.set_math_mode(oracle.MATH_LIBM)
    yield
    oracle.set_math_mode(oracle.MATH_PORTABLE)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_rays.npz"))


@pytest.fixture(scope="module")
def chain_gold(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_rays_chain.npz"))


@pytest.fixture(scope="module")
def ray_scenes(gold, golden_dir):
    """name -> (triangles, eye, look-at): rebuilt here, checked against the digest the fixture was made with"""
    sc = mg.ray_scenes(os.path.join(golden_dir, "assets"))
    from cedec_2024_rt_amd import scenes

    for name, (tris, _, _) in sc.items():
        assert scenes.scene_sha256(tris) == str(gold[name + "_sha"]), f"scene {name} is not the one the fixture was recorded on"
        if name.startswith("soup"):
            assert tris.tobytes() == gold[name + "_tris"].tobytes()
    return sc


def _fields_equal(a, b, mask=None):
    for f in a.dtype.names:
        if f == "pad":
            continue
        x, y = (a[f], b[f]) if mask is None else (a[f][mask], b[f][mask])
        if not np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)):
            return f
    return None


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _setup(oracle, gold, ray_scenes, name, use_bvh):
    tris, eye, at = ray_scenes[name]
    W, H = int(gold["W"]), int(gold["H"])
    sc = oracle.Scene(tris, use_bvh=use_bvh)
    rg = oracle.raygen_lookat(eye, at, (0, 1, 0), mg.FOVY, W, H)
    assert rg.tobytes() == gold[name + "_raygen"].tobytes()
    return tris, sc, rg, np.asarray(eye, np.float32), W, H


def _expand(rows, shaded, oracle):
    """shaded rows of a fixture -> a whole reservoir buffer (non-shaded pixels = Reservoir{})"""
    r = np.zeros(len(shaded), oracle.RESERVOIR)
    r[shaded] = rows
    return r


# ------------------------------------------------------------------------------------------------ raycast
@BVH
@pytest.mark.parametrize("name", ["c1", "c2", "quad", "blocks_restir", "soup0", "soup1", "soup2"])
def test_raycast_fixture(oracle, gold, ray_scenes, name, use_bvh):
    """10_restir_di.cu:9-34: the pixel index flip, Visibility{uv, index} with index = -1 and uv = 0 on a miss"""
    tris, sc, rg, eye, W, H = _setup(oracle, gold, ray_scenes, name, use_bvh)
    want = gold[name + "_vis"]
    got = sc.raycast(W, H, rg)
    assert _fields_equal(got, want) is None
    miss = want["index"] == -1
    assert (~miss).sum() > 50
    if name == "blocks_restir":  # a closed room: every primary ray hits
        assert miss.sum() == 0
    else:
        assert miss.sum() > 0, "a raycast case in an open scene needs misses too"
    assert not want["uv"][miss].any()
    assert not np.array_equal(want["index"], want["index"][::-1]), "a vertically symmetric image would hide the row flip"


# ------------------------------------------------------------------------------------- generate_candidate
GEN_CASES = [("c2", "reuse"), ("c2", "shadowed"), ("c2", "both"), ("quad", "reuse"), ("quad", "shadowed"), ("quad", "both"),
             ("blocks_restir", "both")]


@BVH
@pytest.mark.parametrize("name,variant", GEN_CASES)
def test_generate_candidate_fixture(oracle, gold, ray_scenes, name, variant, use_bvh):
    """10_restir_di.cu:36-135 with use_visibility_reuse (:127-131, the setting of the headline benchmark) and
    use_shadowed_target_function (:115-118) on"""
    tris, sc, rg, eye, W, H = _setup(oracle, gold, ray_scenes, name, use_bvh)
    vis = gold[name + "_vis"]
    shaded = mg.shaded_mask(vis, tris)
    want = gold[f"{name}_gen_{variant}"]
    cnt = oracle.new_counters()
    got = sc.generate_candidate(W, H, 1, vis, eye, oracle.bench_options(**mg.GEN_VARIANTS[variant]), cnt=cnt)
    assert _fields_equal(got[shaded], want) is None
    assert not got[~shaded].view(np.uint8).any()
    hit, miss = (int(v) for v in gold[f"{name}_gen_{variant}_shadow"])
    assert hit > 0 and miss > 0, "shadow rays must answer both ways"
    assert int(cnt["rays"][0]) == hit + miss
    if variant != "shadowed":
        flags = np.bincount(want["visibility"], minlength=2)
        assert flags[0] > 0 and flags[1] > 0 and flags[0] == hit // (2 if variant == "both" else 1)
    else:
        assert not want["visibility"].any()
    if variant != "reuse":
        assert int(gold[f"{name}_gen_{variant}_differs"]) > 0, "the shadowed target function changed no reservoir"


# -------------------------------------------------------- temporal / spatial with the shadowed target function
@BVH
@pytest.mark.parametrize("name", ["c2", "quad"])
def test_shadowed_temporal_spatial_fixture(oracle, gold, ray_scenes, name, use_bvh):
    """10_restir_di.cu:137-237 and :256-388 with use_shadowed_target_function and use_visibility_reuse: up to six rays a pixel"""
    tris, sc, rg, eye, W, H = _setup(oracle, gold, ray_scenes, name, use_bvh)
    vis = gold[name + "_vis"]
    shaded = mg.shaded_mask(vis, tris)
    opt = oracle.bench_options(use_shadowed_target_function=1)
    g1 = sc.generate_candidate(W, H, 1, vis, eye, opt)
    t = sc.generate_candidate(W, H, 2, vis, eye, opt)
    cnt = oracle.new_counters()
    sc.temporal_resampling(W, H, 2, vis, eye, opt, g1, t, cnt=cnt)
    assert _fields_equal(t[shaded], gold[f"{name}_shadowed_temporal"]) is None
    rays = [int(cnt["rays"][0])]
    rin = t
    for p in range(3):
        cnt = oracle.new_counters()
        out = sc.spatial_resampling(W, H, 2, p, vis, eye, opt, rin, cnt=cnt)
        assert _fields_equal(out[shaded], gold[f"{name}_shadowed_spatial{p}"]) is None, f"pass {p}"
        rays.append(int(cnt["rays"][0]))
        out[~shaded] = np.zeros(1, oracle.RESERVOIR)
        rin = out
    assert rays == [int(v) for v in gold[f"{name}_shadowed_rays"]]
    assert rays[0] == 2 * int(shaded.sum()) and all(r > int(shaded.sum()) for r in rays[1:])
    assert all(int(d) > 0 for d in gold[f"{name}_shadowed_differs"]), "a stage where the shadowed target function changed nothing"
    assert (gold[f"{name}_shadowed_spatial2"]["M"] > 64).any()


# ------------------------------------------------------------------------------------------------ resolve
@BVH
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name", ["c2", "quad"])
def test_resolve_fixture(oracle, gold, ray_scenes, name, accumulate, use_bvh):
    """10_restir_di.cu:390-459 as a kernel: sky and light pixels, the shadow ray, `accumulate` both ways"""
    tris, sc, rg, eye, W, H = _setup(oracle, gold, ray_scenes, name, use_bvh)
    vis = gold[name + "_vis"]
    shaded = mg.shaded_mask(vis, tris)
    rows = gold[f"{name}_resolve_res"]
    res = _expand(rows, shaded, oracle)
    acc = gold[f"{name}_resolve_prev"].copy()
    cnt = oracle.new_counters()
    sc.resolve(acc, W, H, vis, eye, oracle.bench_options(accumulate=accumulate), res, cnt=cnt)
    want = gold[f"{name}_resolve_acc{accumulate}"]
    assert np.array_equal(_bits(acc), _bits(want))
    hit, miss = (int(v) for v in gold[f"{name}_resolve_shadow"])
    assert hit > 0 and miss > 0 and int(cnt["rays"][0]) == hit + miss == int(shaded.sum())
    assert int(gold[f"{name}_resolve_decided_by_V"]) > 10, "no pixel where V = 0 is what makes the result 0"
    assert (rows["visibility"] == 0).any() and (rows["visibility"] == 1).any() and (rows["ucw"] == 0).any() and (rows["ucw"] > 0).any()
    lights = np.isin(vis["index"], sc.lights)
    assert (vis["index"] == -1).any() and (lights.any() or name == "quad")
    assert (want[shaded][:, :3] > 0).any() and (want[vis["index"] == -1] == np.float32([0, 0, 0, 1])).all()
    if accumulate:
        assert (want[shaded][:, 3] == gold[f"{name}_resolve_prev"][shaded][:, 3] + 1).all()


# ------------------------------------------------------------------------------------------- path tracers
def _endings(trace, lights, oracle):
    """how the reference's paths ended, from the last ray each pixel traced: (sky, light, neither)"""
    last = trace[:, oracle.TRACE_LAST]
    lit = (last >= 0) & np.isin(last, lights)
    return int((last < 0).sum()), int(lit.sum()), int(((last >= 0) & ~lit).sum())


def _check_pt_nontrivial(example, trace, lights, oracle, what):
    sky, light, other = _endings(trace, lights, oracle)
    if example == 7:  # the last ray is the path's own: sky, a light, or a surface when max_depth ran out
        assert sky > 0 and light > 0 and other > 0, f"{what}: paths ending on sky / light / out of depth = {sky} / {light} / {other}"
    else:
        h, m = int(trace[:, oracle.TRACE_SHADOW_HIT].sum()), int(trace[:, oracle.TRACE_SHADOW_MISS].sum())
        assert h > 0 and m > 0, f"{what}: shadow rays answering 0 / 1 = {h} / {m}"


@BVH
@pytest.mark.parametrize("name,case", mg.PT_SCENE_CASES, ids=lambda v: v if isinstance(v, str) else v[0])
def test_path_trace_fixture(oracle, gold, ray_scenes, name, case, use_bvh):
    """07_pt.cu:11-90, 08_nee.cu:11-140, 09_ris.cu:11-166: the bounce loop, exit conditions, RNG draw order, throughput, NEE,
    RIS weights; max_depth 1 / 2 / 6, a sky colour != 0, ris_sample_count 1 / 32, the shadowed target function both ways"""
    key, example, kw = case
    tris, sc, rg, eye, W, H = _setup(oracle, gold, ray_scenes, name, use_bvh)
    want, trace = gold[f"{name}_{key}"], gold[f"{name}_{key}_trace"]
    acc = np.full((W * H, 4), 7.0, np.float32)  # accumulate = 0 overwrites
    cnt = oracle.new_counters()
    sc.path_trace(example, W, H, 3, rg, oracle.default_options(sky_color=mg.PT_SKY, **kw), acc, cnt=cnt)
    assert np.array_equal(_bits(acc[:, :3]), _bits(want)) and (acc[:, 3] == 1.0).all()
    assert int(cnt["rays"][0]) == int(trace[:, oracle.TRACE_RAYS].sum())
    _check_pt_nontrivial(example, trace, sc.lights, oracle, f"{name} {key}")
    assert (want > 0).any()


@BVH
@pytest.mark.parametrize("example", [7, 8, 9])
def test_path_trace_accumulate_fixture(oracle, gold, ray_scenes, example, use_bvh):
    """the `accumulate` branch (07_pt.cu:82-89 and its twins) over frames 1..3 from a cleared buffer"""
    tris, sc, rg, eye, W, H = _setup(oracle, gold, ray_scenes, "c2", use_bvh)
    acc = np.zeros((W * H, 4), np.float32)
    rays = []
    for fr in (1, 2, 3):
        cnt = oracle.new_counters()
        sc.path_trace(example, W, H, fr, rg, oracle.default_options(sky_color=mg.PT_SKY, accumulate=1), acc, cnt=cnt)
        rays.append(int(cnt["rays"][0]))
    want = gold[f"c2_pt{example}_accumulate3"]
    assert np.array_equal(_bits(acc), _bits(want)) and (want[:, 3] == 3.0).all()
    assert rays == [int(v) for v in gold[f"c2_pt{example}_accumulate3_rays"]] and len(set(rays)) > 1


# ---------------------------------------------------------------------------------- 06_ao_hiprt and 04_ao
@BVH
@pytest.mark.parametrize("name", ["blocks_ao", "c1", "soup0", "soup2"])
def test_ao06_equals_ao04_fixture(oracle, gold, ray_scenes, name, use_bvh):
    """06_ao_hiprt.cu:35-91 over the intersection by definition == 04_ao.cu:31-88 (its own loop) == the oracle's o_ao_04: the
    reference's two kernels agree with each other byte for byte, so rt_path_trace 6 is tied to the kernel it is named after"""
    tris, sc, rg, eye, W, H = _setup(oracle, gold, ray_scenes, name, use_bvh)
    a4, a6 = gold[name + "_ao04"], gold[name + "_ao06"]
    assert np.array_equal(a4, a6), "the reference's 04_ao and 06_ao_hiprt kernels differ on the same input"
    assert np.array_equal(np.asarray(sc.ao_04(W, H, rg)).reshape(H, W, 4), a6)
    hit = a6[..., 0] != 32
    assert hit.sum() > 50 and (~hit).sum() > 0 and len(np.unique(a6[..., 0][hit])) > 3


# ------------------------------------------------------------------------------------------ frame chains
@BVH
@pytest.mark.parametrize("name", ["c2", "quad"])
def test_frame_chain_fixture(oracle, chain_gold, gold, ray_scenes, name, use_bvh):
    """raycast -> generate -> temporal -> save -> spatial x passes -> resolve -> tone_mapping through the reference's kernels only
    (sequenced as 10_restir_di.cpp:257-379) == Scene.frame, every frame: accumulation, pixels, rays. c2: bench options, 4 frames;
    quad: the shadowed target function and accumulate = 1, 3 frames"""
    tris, sc, rg, eye, W, H = _setup(oracle, gold, ray_scenes, name, use_bvh)
    opt = chain_gold[name + "_options"]
    st = oracle.new_state(W, H)
    frames = int(chain_gold[name + "_frames"])
    assert frames >= 3
    for fr in range(1, frames + 1):
        cnt = oracle.new_counters()
        sc.frame(W, H, fr, rg, eye, opt, st, cnt=cnt)
        assert np.array_equal(_bits(st["accum"]), _bits(chain_gold[f"{name}_frame{fr}_accum"])), f"frame {fr}"
        assert np.array_equal(st["pixels"], chain_gold[f"{name}_frame{fr}_pixels"]), f"frame {fr}"
        assert int(cnt["rays"][0]) == int(chain_gold[f"{name}_frame{fr}_rays"]), f"frame {fr}"
    M = chain_gold[name + "_final_M"]
    assert M.max() > 32 * frames, "the history never carried M forward"
    assert not np.array_equal(chain_gold[f"{name}_frame1_pixels"], chain_gold[f"{name}_frame{frames}_pixels"])
    if int(opt["accumulate"][0]):
        assert (chain_gold[f"{name}_frame{frames}_accum"][mg.shaded_mask(st["vis"], tris)][:, 3] == frames).all()


# --------------------------------------------------------------------------------------------- wide pin
def _oracle_wide(oracle, W, H, variant_kw, frames, compared, tris=None, history=None, first=1, scene=None):
    from cedec_2024_rt_amd import scenes

    sc, vis, eye = scene
    opt = oracle.bench_options()
    cand = lambda fr: sc.generate_candidate(W, H, fr, vis, eye, opt)  # noqa: E731

    def temporal(W, H, fr, tris, vis, eye, opt, prev, res):
        return sc.temporal_resampling(W, H, fr, vis, eye, opt, prev, res.copy())

    def spatial(W, H, fr, p, tris, vis, eye, opt, rin):
        return sc.spatial_resampling(W, H, fr, p, vis, eye, opt, rin)

    return mg.wide_chain(variant_kw, frames, compared, temporal, spatial, tris, vis, eye, cand, history=history, first=first)


def test_wide_pin_fixture(oracle, golden_dir):
    """The reference's temporal + 3 x spatial kernels on the 211 916-triangle bench stand-in at 240x135, bench options with
    visibility reuse on, a 26-frame history: `previous_reservoir.M = min(M, 20 * ris_sample_count)` (10_restir_di.cu:185-187) is
    reached and `p_hat *= sample.visibility` (:201-204, :353-356) is live. Frames 1, 2, 13, 25, 26 are compared (SHA-256 per field
    over the shaded pixels); frame 27 once each with temporal off, spatial off, 2 passes, 7 samples."""
    from cedec_2024_rt_amd import scenes

    w = np.load(os.path.join(golden_dir, "ref_wide_pin.npz"))
    W, H = int(w["W"]), int(w["H"])
    assert W >= 240 and H >= 135 and int(w["frames"]) >= 22
    tris = scenes.make_blocks_restir()
    assert scenes.scene_sha256(tris) == str(w["scene_sha"])
    sc = oracle.Scene(tris, use_bvh=True)
    eye = np.asarray(scenes.BLOCKS_RESTIR_EYE, np.float32)
    rg = oracle.raygen_lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT, (0, 1, 0), mg.FOVY, W, H)
    vis = sc.raycast(W, H, rg)
    sh = mg.shaded_mask(vis, tris)
    assert int(sh.sum()) == int(w["shaded"])
    compared = tuple(int(v) for v in w["compared"])
    out, hist = _oracle_wide(oracle, W, H, {}, int(w["frames"]), compared, tris=tris, scene=(sc, vis, eye))
    assert len(out) == 4 * len(compared)
    for (fr, stage), r in out.items():
        for f, d in mg.digest(r, sh).items():
            assert d == str(w[f"main_{fr}_{stage}_{f}"]), f"frame {fr} {stage}: field {f} differs from the reference's kernel"
    M = w["main_M_temporal_26"]
    assert M.max() >= 640 and (M == 672).sum() > 1000, "the M clamp was never reached in the reference's run"
    flags = np.unpackbits(w["main_visibility_26"])[: int(sh.sum())]
    assert (flags == 0).sum() > 100 and (flags == 1).sum() > 100
    for vname, kw in mg.WIDE_VARIANTS.items():
        o2, _ = _oracle_wide(oracle, W, H, kw, 1, (27,), tris=tris, history=hist, first=27, scene=(sc, vis, eye))
        for (fr, stage), r in o2.items():
            for f, d in mg.digest(r, sh).items():
                assert d == str(w[f"{vname}_{fr}_{stage}_{f}"]), f"{vname} frame {fr} {stage}: field {f}"
    assert str(w["no_temporal_27_temporal_M"]) != str(w["main_26_temporal_M"])


# ================================================================================================ live form
needs_ref = pytest.mark.skipif(not __import__("oracle.binding", fromlist=["x"]).have_ref_rays(),
                               reason="oracle/_ref/ref_kernels with the ray-using kernels not built here")

LIVE = {  # other cameras than the fixtures', other frames
    "c1": ((6.0, 9.0, 7.0), (0.0, 0.5, 0.0)), "c2": ((-0.8, 3.4, 5.0), (0.4, 2.0, -2.8)), "quad": ((-1.5, 3.0, 5.0), (0.5, 1.0, -1.0)),
}


def _live_setup(oracle, name, use_bvh, golden_dir, W=40, H=30, seed=None):
    if name == "soup":
        tris, (eye, at) = mg.soup(seed, 180), ((0.0, -1.5, 8.0), (0.0, 0.5, 0.0))
    else:
        tris, (eye, at) = mg.ray_scenes(os.path.join(golden_dir, "assets"))[name][0], LIVE[name]
    sc = oracle.Scene(tris, use_bvh=use_bvh)
    return tris, sc, oracle.raygen_lookat(eye, at, (0, 1, 0), mg.FOVY, W, H), np.asarray(eye, np.float32), W, H


@needs_ref
@BVH
@pytest.mark.parametrize("name", ["c1", "c2", "quad"])
def test_restir_ray_kernels_live(oracle, golden_dir, name, use_bvh):
    """raycast, generate_candidate (3 variants), temporal + 2 x spatial with the shadowed target function, resolve: fresh runs"""
    tris, sc, rg, eye, W, H = _live_setup(oracle, name, use_bvh, golden_dir)
    vis, _ = oracle.ref_raycast(W, H, tris, rg)
    assert _fields_equal(sc.raycast(W, H, rg), vis) is None
    shaded = mg.shaded_mask(vis, tris)
    assert shaded.sum() > 100 and (vis["index"] == -1).any()
    gens = {}
    for fr in (7, 8):
        for vname, kw in mg.GEN_VARIANTS.items():
            opt = oracle.bench_options(**kw)
            want, tr = oracle.ref_generate_candidate(W, H, fr, tris, vis, eye, opt, sc.lights)
            got = sc.generate_candidate(W, H, fr, vis, eye, opt)
            assert _fields_equal(got, want) is None, (fr, vname)
            assert tr[:, oracle.TRACE_SHADOW_HIT].sum() > 0 and tr[:, oracle.TRACE_SHADOW_MISS].sum() > 0
            if vname != "shadowed":
                assert len(np.unique(want["visibility"][shaded])) == 2
            gens[(fr, vname)] = got
    opt = oracle.bench_options(use_shadowed_target_function=1, spatial_resampling_radius=10.0)
    plain = oracle.bench_options(use_shadowed_target_function=0, spatial_resampling_radius=10.0)
    want, _ = oracle.ref_temporal_resampling(W, H, 8, tris, vis, eye, opt, gens[(7, "both")], gens[(8, "both")])
    other, _ = oracle.ref_temporal_resampling(W, H, 8, tris, vis, eye, plain, gens[(7, "both")], gens[(8, "both")])
    assert (want["ucw"][shaded] != other["ucw"][shaded]).any()
    t = gens[(8, "both")].copy()
    sc.temporal_resampling(W, H, 8, vis, eye, opt, gens[(7, "both")], t)
    assert _fields_equal(t, want) is None
    rin = t
    for p in range(2):
        want, _ = oracle.ref_spatial_resampling(W, H, 8, p, tris, vis, eye, opt, rin)
        other, _ = oracle.ref_spatial_resampling(W, H, 8, p, tris, vis, eye, plain, rin)
        assert (want["ucw"][shaded] != other["ucw"][shaded]).any()
        out = sc.spatial_resampling(W, H, 8, p, vis, eye, opt, rin)
        assert _fields_equal(out, want, mask=shaded) is None, f"pass {p}"
        out[~shaded] = np.zeros(1, oracle.RESERVOIR)
        rin = out
    rng = np.random.default_rng(77)
    res = mg.resolve_reservoirs(rng, gens[(8, "reuse")], shaded)  # samples the shadow ray rejects keep ucw > 0 here
    prev = rng.random((W * H, 4), dtype=np.float32)
    for a in (0, 1):
        want, tr = oracle.ref_resolve(W, H, tris, vis, eye, oracle.bench_options(accumulate=a), res, prev)
        acc = prev.copy()
        sc.resolve(acc, W, H, vis, eye, oracle.bench_options(accumulate=a), res)
        assert np.array_equal(_bits(acc), _bits(want)), f"accumulate {a}"
        assert tr[:, oracle.TRACE_SHADOW_HIT].sum() > 0 and tr[:, oracle.TRACE_SHADOW_MISS].sum() > 0
        assert ((tr[:, oracle.TRACE_SHADOW_HIT] == 1) & (res["ucw"] > 0)).sum() > 0


@needs_ref
@BVH
@pytest.mark.parametrize("name,seed", [("c2", None), ("quad", None), ("soup", 52001), ("soup", 52002)])
def test_path_trace_and_ao_live(oracle, golden_dir, name, seed, use_bvh):
    tris, sc, rg, eye, W, H = _live_setup(oracle, name, use_bvh, golden_dir, seed=seed)
    for example in (7, 8, 9):
        for kw in (dict(max_depth=3), dict(max_depth=5, ris_sample_count=4, use_shadowed_target_function=1, accumulate=1)):
            opt = oracle.default_options(sky_color=(0.6, 0.1, 0.3), **kw)
            prev = np.random.default_rng(5).random((W * H, 4), dtype=np.float32)
            want, tr = oracle.ref_path_trace(example, W, H, 11, tris, rg, opt, prev, sc.lights)
            acc, cnt = prev.copy(), oracle.new_counters()
            sc.path_trace(example, W, H, 11, rg, opt, acc, cnt=cnt)
            assert np.array_equal(_bits(acc), _bits(want)), (example, kw)
            assert int(cnt["rays"][0]) == int(tr[:, oracle.TRACE_RAYS].sum())
            _check_pt_nontrivial(example, tr, sc.lights, oracle, f"{name} {example}")
    a4, a6 = oracle.ref_ao(4, W, H, tris, rg), oracle.ref_ao(6, W, H, tris, rg)
    assert np.array_equal(a4, a6) and np.array_equal(np.asarray(sc.ao_04(W, H, rg)).reshape(H, W, 4), a6)
    assert (a6[..., 0] != 32).sum() > 50


@needs_ref
@BVH
def test_frame_chain_live(oracle, golden_dir, use_bvh):
    tris, sc, rg, eye, W, H = _live_setup(oracle, "c1", use_bvh, golden_dir, W=36, H=24)
    opt = oracle.bench_options(use_shadowed_target_function=1, accumulate=1, spatial_resampling_passes=2, spatial_resampling_radius=8.0)
    ref, st = oracle.new_state(W, H), oracle.new_state(W, H)
    for fr in (4, 5, 6):
        rays = oracle.ref_frame(W, H, fr, tris, rg, eye, opt, sc.lights, ref)
        cnt = oracle.new_counters()
        sc.frame(W, H, fr, rg, eye, opt, st, cnt=cnt)
        assert np.array_equal(_bits(st["accum"]), _bits(ref["accum"])) and np.array_equal(st["pixels"], ref["pixels"]), f"frame {fr}"
        assert int(cnt["rays"][0]) == rays
        sh = mg.shaded_mask(ref["vis"], tris)
        for b in ("r0", "r1"):
            ref[b][~sh] = np.zeros(1, oracle.RESERVOIR)
    assert ref["temporal"]["M"].max() > 64 and sh.sum() > 100


@needs_ref
def test_m_clamp_live(oracle):
    """a 23-frame history at 64x36 on the quad room, visibility reuse on: the reference's temporal kernel clamps M at 640"""
    from cedec_2024_rt_amd import scenes

    W, H = 64, 36
    tris = scenes.make_quad_room()
    sc = oracle.Scene(tris, use_bvh=True)
    eye = np.asarray(LIVE["quad"][0], np.float32)
    rg = oracle.raygen_lookat(LIVE["quad"][0], LIVE["quad"][1], (0, 1, 0), mg.FOVY, W, H)
    vis = sc.raycast(W, H, rg)
    sh = mg.shaded_mask(vis, tris)
    opt = oracle.bench_options()
    hist_ref, hist = np.zeros(W * H, oracle.RESERVOIR), np.zeros(W * H, oracle.RESERVOIR)
    for fr in range(1, 24):
        cand = sc.generate_candidate(W, H, fr, vis, eye, opt)
        hist_ref, _ = oracle.ref_temporal_resampling(W, H, fr, tris, vis, eye, opt, hist_ref, cand)
        t = cand.copy()
        sc.temporal_resampling(W, H, fr, vis, eye, opt, hist, t)
        hist = t
        assert _fields_equal(hist, hist_ref) is None, f"frame {fr}"
    assert hist_ref["M"][sh].max() == 672 and (hist_ref["visibility"][sh] == 0).any()
    want, _ = oracle.ref_spatial_resampling(W, H, 23, 0, tris, vis, eye, opt, hist_ref)
    assert _fields_equal(sc.spatial_resampling(W, H, 23, 0, vis, eye, opt, hist), want, mask=sh) is None
