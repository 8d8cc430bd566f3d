"""The frame kernels at degenerate image shapes and on thin strips: the HIP path against the oracle, bit for bit, on the cases of
tests/shape_space_cases.py (tests/test_shape_space_cpu.py shows on the oracle alone that none of them passes vacuously).

The kernels' own structure is what can go wrong here, and nothing faults when it does: the tracing kernels run one wavefront on an
8 x 8 tile and share an LDS stack (and, in the work-sharing forms, work) between lanes of which at 1 x N and N x 1 almost all are off
the image; k_spatial_coop keeps those lanes alive through every gather round; tile_pixel_at maps workgroups to tiles in eight orders
over 8 XCDs on a grid padded to 128, with 33 = 4 * 8 + 1 tiles along one axis and one along the other; the path tracers and the
ray-major ambient occlusion size their lists from W * H; the sparse-halo plan has never run with a halo of 1, 9 or 29 rows.

    a. test_kernel_by_kernel            every reference kernel through its own entry point, every shape / view / radius
    b. test_frame_forms, test_tile_orders   rt_frame and its launch forms, six frames back to back; the eight tile orders per kernel
    c. test_experiment_forms            the A/B forms of the experiments library
    d. test_unbiased_*, test_power_*    the modes with a restatement of their own
    e. test_path_tracers, test_ambient_occlusion
    f. test_thin_strips_*               strips exactly one halo tall, with interior rows, with a last strip of another height
"""
import math

import numpy as np
import pytest

import shape_space_cases as ssc
from test_gpu_parity import _eq_bits, _res_fields_equal
from test_mg_native import _Rig

pytestmark = pytest.mark.gpu

RT_ERR_ARG, RT_ERR_STATE = 1, 3  # include/restir_rt.h


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def tris():
    from cedec_2024_rt_amd import scenes

    return scenes.make_quad_room()


_scene = []


def _oracle(oracle, tris, W, H, camera, radius, **optkw):
    """(scene, raygen, options, eye) of the oracle for one camera = (eye, lookat, fovy)"""
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    if not _scene:
        _scene.append(oracle.Scene(tris, use_bvh=True))
    eye, at, fovy = camera
    rg = oracle.raygen_lookat(eye, at, (0, 1, 0), fovy, W, H)
    return _scene[0], rg, oracle.bench_options(spatial_resampling_radius=radius, **optkw), np.asarray(eye, np.float32)


def _renderer(api, tris, W, H, camera, radius, exp=False, tuning=(), rows=None, halo=0, **optkw):
    from cedec_2024_rt_amd.types import bench_options

    r = api.Renderer(W, H, rows=rows, halo=halo, exp=exp)
    for key, value in tuning:
        r.tuning(key, value)
    r.set_scene(tris)
    eye, at, fovy = camera
    r.lookat(eye, at, fovy=fovy)
    r.set_options(bench_options(spatial_resampling_radius=radius, **optkw))
    return r


def _shaded(sc, vis):
    return (vis["index"] >= 0) & ~np.isin(vis["index"], sc.lights)


def _first_diff(got, want, W):
    """how many pixels differ and the (x, row) of the first, for the messages; both arrays have one entry per pixel along axis 0"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = np.flatnonzero((g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)).any(axis=1))
    return f"{len(bad)} pixels differ, the first at (x {int(bad[0]) % W}, row {int(bad[0]) // W})" if len(bad) else "equal"


def _frozen(*arrays):
    out = []
    for a in arrays:
        a = a.copy()
        a.setflags(write=False)
        out.append(a)
    return out


_refs = {}


def _reference(oracle, tris, W, H, view, radius, frames, **optkw):
    """per (shape, view, radius, frames, options), once: the oracle's state after `frames` frames: dict(accum (W*H, 4), pixels (H, W, 4),
    temporal, shaded, rays of the last frame, rays_total of all frames); read-only"""
    key = (W, H, view, radius, frames, tuple(sorted(optkw.items())))
    if key not in _refs:
        sc, rg, opt, eyev = _oracle(oracle, tris, W, H, ssc.camera(view, W, H), radius, **optkw)
        st = oracle.new_state(W, H)
        rays_total = 0
        for frame in range(1, frames + 1):
            cnt = oracle.new_counters()
            sc.frame(W, H, frame, rg, eyev, opt, st, cnt)
            rays_total += int(cnt["rays"][0])
        accum, pixels, temporal, shaded = _frozen(st["accum"].reshape(W * H, 4), st["pixels"], st["temporal"], _shaded(sc, st["vis"]))
        _refs[key] = dict(accum=accum, pixels=pixels, temporal=temporal, shaded=shaded, rays=int(cnt["rays"][0]), rays_total=rays_total)
    return _refs[key]


def _check_against(api, r, ref, W, H, what, rays=True):
    acc = r.download(api.RT_BUF_ACCUMULATION)
    assert _eq_bits(acc, ref["accum"]), f"{what}: accumulation: {_first_diff(acc, ref['accum'], W)}"
    px = r.download(api.RT_BUF_PIXELS)
    assert np.array_equal(px.reshape(H, W, 4), ref["pixels"]), f"{what}: pixels: {_first_diff(px, ref['pixels'].reshape(W * H, 4), W)}"
    bad = _res_fields_equal(r.download(api.RT_BUF_RES_TEMPORAL), ref["temporal"], mask=ref["shaded"])
    assert not bad, f"{what}: temporal history {bad}"
    if rays:
        assert r.ray_count() == (ref["rays"], int(ref["shaded"].sum())), f"{what}: ray count"


# =============================================================================================== a. kernel by kernel
KERNEL_CASES = [(W, H, view, radius, {}) for W, H, view, radius in ssc.ALL_CASES]
KERNEL_CASES += [(W, H, view, radius, dict(use_shadowed_target_function=1, accumulate=1))
                 for W, H in ssc.SHADOWED_ACCUMULATE_SHAPES for view in ssc.VIEWS for radius in ssc.RADII]


@pytest.mark.parametrize("W,H,view,radius,optkw", KERNEL_CASES,
                         ids=[ssc.case_id(W, H, view, radius) + ("_shadowed_accumulate" if kw else "") for W, H, view, radius, kw in KERNEL_CASES])
def test_kernel_by_kernel(api, oracle, tris, W, H, view, radius, optkw):
    """The sequence of tests/test_gpu_parity.py::test_kernel_by_kernel_parity, frames 1 to 3: after every entry point the buffer it wrote
    against the oracle's - every byte of the Visibility records; every field of the candidates' and the temporal merge's reservoirs on
    all pixels; the spatial passes' on the shaded ones (the reference writes no others); the shaded pixels of every row as the device
    counts them; accumulation; pixels. Then rt_ray_count against the counters of the oracle's kernels."""
    camera = ssc.camera(view, W, H)
    sc, rg, opt, eyev = _oracle(oracle, tris, W, H, camera, radius, **optkw)
    r = _renderer(api, tris, W, H, camera, radius, **optkw)
    assert rg.tobytes() == r.raygen().tobytes()
    r.clear()
    st = oracle.new_state(W, H)
    for frame in ssc.FRAMES:
        at = f"{ssc.case_id(W, H, view, radius)} frame {frame}"
        cnt = oracle.new_counters()
        r.raycast()
        sc.raycast(W, H, rg, st["vis"], cnt=cnt)
        vis = r.download(api.RT_BUF_VISIBILITY)
        assert _eq_bits(vis, st["vis"]), f"{at}: raycast: {_first_diff(vis, st['vis'], W)}"
        shaded = _shaded(sc, st["vis"])
        assert np.array_equal(r.row_shaded(), shaded.reshape(H, W).sum(axis=1)), f"{at}: shaded pixels per row"
        r.generate_candidate(frame, api.RT_RES_0)
        sc.generate_candidate(W, H, frame, st["vis"], eyev, opt, st["r0"], cnt=cnt)
        bad = _res_fields_equal(r.download(api.RT_BUF_RES_0), st["r0"])
        assert not bad, f"{at}: generate_candidate {bad}"
        r.temporal_resampling(frame, api.RT_RES_TEMPORAL, api.RT_RES_0)
        sc.temporal_resampling(W, H, frame, st["vis"], eyev, opt, st["temporal"], st["r0"], cnt=cnt)
        bad = _res_fields_equal(r.download(api.RT_BUF_RES_0), st["r0"])
        assert not bad, f"{at}: temporal_resampling {bad}"
        r.save_temporal_reservoir(api.RT_RES_0, api.RT_RES_TEMPORAL)
        oracle.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        bad = _res_fields_equal(r.download(api.RT_BUF_RES_TEMPORAL), st["temporal"])
        assert not bad, f"{at}: save_temporal_reservoir {bad}"
        src, dst = api.RT_RES_0, api.RT_RES_1
        osrc, odst = st["r0"], st["r1"]
        for k in range(3):
            if k:
                src, dst = dst, src
                osrc, odst = odst, osrc
            r.spatial_resampling(frame, k, src, dst)
            sc.spatial_resampling(W, H, frame, k, st["vis"], eyev, opt, osrc, odst, cnt=cnt)
            bad = _res_fields_equal(r.download(api.RT_BUF_RES_0 + dst), odst, mask=shaded)
            assert not bad, f"{at}: spatial pass {k} {bad}"
        r.resolve(dst)
        sc.resolve(st["accum"], W, H, st["vis"], eyev, opt, odst, cnt=cnt)
        acc = r.download(api.RT_BUF_ACCUMULATION)
        assert _eq_bits(acc, st["accum"].reshape(acc.shape)), f"{at}: resolve: {_first_diff(acc, st['accum'].reshape(acc.shape), W)}"
        r.tone_mapping()
        px = r.download(api.RT_BUF_PIXELS).reshape(H, W, 4)
        assert np.array_equal(px, oracle.tone_mapping(st["accum"], W, H)), f"{at}: tone_mapping"
        assert r.ray_count() == (int(cnt["rays"][0]), int(shaded.sum())), f"{at}: ray count"
    r.close()


# =============================================================================================== b. rt_frame and its forms
SIX = 6


def _six_frames(r, by_kernels=False, after_first=None):
    """six frames enqueued back to back, nothing waits in between"""
    for frame in range(1, SIX + 1):
        if by_kernels:
            r.frame_by_kernels(frame)
        else:
            r.frame(frame)
        if frame == 1 and after_first:
            after_first(r)


def _frame_forms(api):
    """(name, experiments library?, rt_tuning pairs, switch to throw on the context or None, what stage0_one_launch must say or None)"""
    T = api.Tune
    forms = [
        ("defaults", False, (), None, None),
        ("spec0_tail0", False, ((T.SPEC, 0), (T.TAIL, 0)), None, None),
        ("fuse_raycast0", False, ((T.FUSE_RAYCAST, 0),), None, False),
        # one launch is the candidates' work-sharing walk behind a primary ray of the plain walk; a launch this small would take the
        # work-sharing primary walk (WS_PRIMARY auto) and with it two launches
        ("fuse_raycast1", False, ((T.FUSE_RAYCAST, 1), (T.WS_PRIMARY, 0)), None, True),
        ("stream1", True, ((T.STREAM, 1),), None, None),  # the product library carries STREAM = 0 alone
    ]
    forms += [(f"ws{v}", False, ((T.WS, v),), None, None) for v in (-1, 0, 1)]
    forms += [(f"ws_primary{v}", False, ((T.WS_PRIMARY, v),), None, None) for v in (-1, 0, 1)]
    forms += [
        ("timing", False, (), lambda r: r.timing_enable(True), None),
        ("walk_stats", False, (), lambda r: r.walk_stats_enable(True), None),
        ("gbuffer_reuse1", False, (), lambda r: r.gbuffer_reuse(True), None),
        ("gbuffer_reuse0", False, (), lambda r: r.gbuffer_reuse(False), None),
        ("occluder_hints1", False, (), lambda r: r.occluder_hints(True), None),
        ("occluder_hints0", False, (), lambda r: r.occluder_hints(False), None),
    ]
    forms += [(f"neighbour_pick{m}", False, (), (lambda m: lambda r: r.neighbour_pick(m))(m), None) for m in (0, 1, 2)]
    forms.append(("frame_by_kernels", False, (), None, None))
    return forms


def test_the_forms_name_every_value_the_product_library_accepts(api, tris):
    """WS and WS_PRIMARY: -1, 0, 1 are what librestir_rt.so takes (WS_PRIMARY = 2 and STREAM = 1 are A/B forms of the experiments
    library); neighbour_pick has modes 0, 1, 2"""
    r = api.Renderer(8, 8)
    for key, ok, refused in ((api.Tune.WS, (-1, 0, 1), (-2, 2)), (api.Tune.WS_PRIMARY, (-1, 0, 1), (-2, 2, 3)), (api.Tune.STREAM, (0,), (1,))):
        for v in ok:
            r.tuning(key, v)
        for v in refused:
            with pytest.raises(api.RtError):
                r.tuning(key, v)
    for mode in (0, 1, 2):
        r.neighbour_pick(mode)
    for mode in (-1, 3):
        with pytest.raises(api.RtError):
            r.neighbour_pick(mode)
    r.close()


VIEW_AND_RADIUS = [("floor", 3.0), ("mixed", 30.0)]  # every pixel shaded and neighbours on the image; sky and lamps beside shaded pixels, most picks off it


@pytest.mark.parametrize("view,radius", VIEW_AND_RADIUS)
@pytest.mark.parametrize("W,H", ssc.FRAME_FORM_SHAPES, ids=[ssc.case_id(W, H) for W, H in ssc.FRAME_FORM_SHAPES])
def test_frame_forms(api, oracle, tris, W, H, view, radius):
    """rt_frame in every launch form the product library has (and STREAM = 1 of the experiments library): six frames back to back with
    no sync; the last frame's accumulation, pixels, temporal history and ray count == the oracle's"""
    ref = _reference(oracle, tris, W, H, view, radius, SIX)
    camera = ssc.camera(view, W, H)
    for name, exp, tuning, switch, one_launch in _frame_forms(api):
        name = f"{view} radius {radius:g} {name}"
        r = _renderer(api, tris, W, H, camera, radius, exp=exp, tuning=tuning)
        if switch:
            switch(r)
        seen = []
        _six_frames(r, by_kernels=name.endswith("frame_by_kernels"), after_first=lambda r: seen.append(r.stage0_one_launch()))
        if one_launch is not None:
            assert seen == [one_launch], f"{W}x{H} {name}: stage 0 of frame 1 ran as {'one launch' if seen[0] else 'two launches'}"
        _check_against(api, r, ref, W, H, f"{W}x{H} {name}")
        if name.endswith(" timing"):
            ms = np.float32(list(r.timing().values()))
            assert len(ms) == 9 and np.isfinite(ms).all() and (ms >= 0).all(), ms
        if name.endswith("walk_stats"):
            ws = r.walk_stats()
            for k, v in ws.items():
                assert v["walked"] + v["self_test"] + v["not_evaluated"] == v["reference_rays"], (k, v)
            assert ws["raycast"]["reference_rays"] > 0
        r.close()


TILE_KEYS = ("TILE_RAYCAST", "TILE_GENERATE", "TILE_SPATIAL", "TILE_RESOLVE")


@pytest.mark.parametrize("view,radius", VIEW_AND_RADIUS)
@pytest.mark.parametrize("key", TILE_KEYS)
@pytest.mark.parametrize("W,H", ssc.TILE_ORDER_SHAPES, ids=[ssc.case_id(W, H) for W, H in ssc.TILE_ORDER_SHAPES])
def test_tile_orders(api, oracle, tris, W, H, key, view, radius):
    """each of the eight tile orders on one kernel class at a time, accumulating: a tile that resolve visits twice adds its radiance
    twice, a tile missed keeps the previous frame's; the stage-0 forms that run the tracing kernels apart (FUSE_RAYCAST = 0) included.
    A second visit by raycast, the candidates or a spatial pass writes the same bytes again, so every order runs once more with the
    walk counters on (for the spatial key with the shadowed target, whose passes trace rays): each kernel counts its reference rays
    as often as it ran a pixel, and the counts must be the oracle's."""
    T = api.Tune
    camera = ssc.camera(view, W, H)
    ref = _reference(oracle, tris, W, H, view, radius, SIX, accumulate=1)
    counted = _reference(oracle, tris, W, H, view, radius, SIX, accumulate=1, use_shadowed_target_function=1)
    n_shaded = int(ref["shaded"].sum())
    for order in range(8):
        for extra in ((), ((T.FUSE_RAYCAST, 0), (T.SPEC, 0))) if key in ("TILE_RAYCAST", "TILE_GENERATE") else ((),):
            what = f"{W}x{H} {view} radius {radius:g} {key} = {order} {extra}"
            r = _renderer(api, tris, W, H, camera, radius, tuning=((T[key], order),) + extra, accumulate=1)
            assert r.tuning_get(T[key]) == order
            r.clear()
            _six_frames(r)
            _check_against(api, r, ref, W, H, what)
            r.close()
        # SPEC = 0: every kernel runs exactly once per frame (no stage 0 of a frame that is never rendered), as in
        # tests/test_gpu_round4.py::test_walk_stats_account_for_every_reference_ray, whose relations these are
        shadowed = key == "TILE_SPATIAL"  # the unshadowed pass traces nothing; the shadowed candidates' kernel counts nothing
        want = counted if shadowed else ref
        r = _renderer(api, tris, W, H, camera, radius, tuning=((T[key], order), (T.SPEC, 0)), accumulate=1, use_shadowed_target_function=int(shadowed))
        r.walk_stats_enable(True)
        r.clear()
        _six_frames(r)
        what = f"{W}x{H} {view} radius {radius:g} {key} = {order}, walk counters"
        _check_against(api, r, want, W, H, what)
        ws = {k: c["reference_rays"] for k, c in r.walk_stats().items()}
        assert ws["raycast"] == W * H * SIX and ws["resolve"] == n_shaded * SIX, f"{what}: {ws}"
        if shadowed:
            # the reference's rays of six frames less the primary rays and, per shaded pixel and frame, the candidate's p-hat ray, its
            # visibility-reuse ray, the temporal merge's two and resolve's one (rt_ray_count, restir_rt.hip): what the passes traced
            assert ws["spatial_resampling"] == want["rays_total"] - W * H * SIX - 5 * n_shaded * SIX, f"{what}: {ws}"
        else:
            assert ws["generate_candidate"] == n_shaded * SIX and ws["spatial_resampling"] == 0, f"{what}: {ws}"
            assert sum(ws.values()) == want["rays_total"], f"{what}: {ws}"
        r.close()


# =============================================================================================== c. the experiments library's forms
def _experiment_forms(api):
    T = api.Tune
    forms = [("half_raycast", ((T.HALF_RAYCAST, 1),))]
    forms += [(f"spatial_variant{v}", ((T.SPATIAL_VARIANT, v),)) for v in (0, 1, 3, 4)]
    forms += [(f"fuse_final{v}", ((T.FUSE_FINAL, v),)) for v in (1, 2)]
    forms += [("defer_vis", ((T.DEFER_VIS, 1),)), ("ris_pipe", ((T.RIS_PIPE, 1),))]
    return forms


@pytest.mark.parametrize("view,radius", VIEW_AND_RADIUS)
@pytest.mark.parametrize("W,H", ssc.EXPERIMENT_SHAPES, ids=[ssc.case_id(W, H) for W, H in ssc.EXPERIMENT_SHAPES])
def test_experiment_forms(api, oracle, tris, W, H, view, radius):
    """librestir_rt_exp.so: the half-density raycast, the gather / LDS-staged / software-pipelined / one-wavefront spatial passes (the
    LDS-staged ones keep a window of +-87 rows and 7 words of shaded bits around a tile: here the whole image is smaller than the
    window), the last pass fused with resolve, the deferred visibility queue and the pipelined RIS loop: six frames back to back"""
    ref = _reference(oracle, tris, W, H, view, radius, SIX)
    camera = ssc.camera(view, W, H)
    for name, tuning in _experiment_forms(api):
        r = _renderer(api, tris, W, H, camera, radius, exp=True, tuning=tuning)
        for key, value in tuning:
            assert r.tuning_get(key) == value
        _six_frames(r)
        # rt_ray_count is the reference's count whatever the build walks; the deferred queue's own count is rt_visibility_rays_walked
        _check_against(api, r, ref, W, H, f"{W}x{H} {view} radius {radius:g} {name}")
        r.close()


# =============================================================================================== d. modes with a restatement of their own
class _Cpu:
    """the frame of 10_restir_di.cpp:257-379 on the CPU: the oracle's kernels, with the candidates from tests/light_sampling_ref.py
    (power) or the spatial pass from tests/restir_unbiased_ref.py (unbiased): the _Cpu of tests/test_gpu_light_sampling.py and
    tests/test_gpu_restir_unbiased.py with the camera as an argument"""

    def __init__(self, oracle, tris, W, H, camera, radius, power=False, unbiased=False):
        self.o, self.tris, self.W, self.H, self.power, self.unbiased = oracle, tris, W, H, power, unbiased
        self.sc, self.rg, self.opt, self.eye = _oracle(oracle, tris, W, H, camera, radius)
        self.st = oracle.new_state(W, H)
        self.sc.raycast(W, H, self.rg, self.st["vis"])
        self.shaded = _shaded(self.sc, self.st["vis"])

    def frame(self, frame):
        import light_sampling_ref as ls
        import restir_unbiased_ref as ru

        sc, st, W, H, opt = self.sc, self.st, self.W, self.H, self.opt
        if self.power:
            ls.generate_candidate(W, H, frame, self.tris, st["vis"], self.eye, opt, ls.POWER, st["r0"])
        else:
            sc.generate_candidate(W, H, frame, st["vis"], self.eye, opt, st["r0"])
        sc.temporal_resampling(W, H, frame, st["vis"], self.eye, opt, st["temporal"], st["r0"])
        self.o.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        src, dst = "r0", "r1"
        for k in range(int(opt["spatial_resampling_passes"][0])):
            if k:
                src, dst = dst, src
            if self.unbiased:
                st[dst] = ru.spatial(W, H, frame, k, self.tris, st["vis"], self.eye, opt, st[src])[0]
            else:
                st[dst] = sc.spatial_resampling(W, H, frame, k, st["vis"], self.eye, opt, st[src])
        sc.resolve(st["accum"], W, H, st["vis"], self.eye, opt, st[dst])
        st["pixels"] = self.o.tone_mapping(st["accum"], W, H)
        return st[dst]


def _restated_mode(api, oracle, tris, W, H, view, radius, power, unbiased):
    camera = ssc.camera(view, W, H)
    cpu = _Cpu(oracle, tris, W, H, camera, radius, power=power, unbiased=unbiased)
    plain = _Cpu(oracle, tris, W, H, camera, radius)
    rs = {}
    for how in ("rt_frame", "frame_by_kernels"):
        r = _renderer(api, tris, W, H, camera, radius)
        if power:
            assert r.light_sampling(api.RT_LIGHTS_POWER) == api.RT_LIGHTS_POWER
        if unbiased:
            assert r.spatial_unbiased(True) is True
        rs[how] = r
    differs = 0
    for frame in ssc.FRAMES:
        last = cpu.frame(frame)
        differs += int((last.view(np.uint8).reshape(W * H, -1) != plain.frame(frame).view(np.uint8).reshape(W * H, -1)).any(axis=1)[cpu.shaded].sum())
        for how, r in rs.items():
            out = r.frame(frame) if how == "rt_frame" else r.frame_by_kernels(frame)
            what = f"{ssc.case_id(W, H, view, radius)} {how} frame {frame}"
            acc = r.download(api.RT_BUF_ACCUMULATION)
            assert _eq_bits(acc, cpu.st["accum"].reshape(acc.shape)), f"{what}: accumulation: {_first_diff(acc, cpu.st['accum'].reshape(acc.shape), W)}"
            assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), cpu.st["pixels"]), f"{what}: pixels"
            bad = _res_fields_equal(r.download(api.RT_BUF_RES_0 + out), last, mask=cpu.shaded)
            assert not bad, f"{what}: records after the frame {bad}"
            bad = _res_fields_equal(r.download(api.RT_BUF_RES_TEMPORAL), cpu.st["temporal"], mask=cpu.shaded)
            assert not bad, f"{what}: temporal history {bad}"
    for r in rs.values():
        r.close()
    return differs, int(cpu.shaded.sum())


RESTATED_CASES = [(W, H, view, radius) for W, H in ssc.RESTATED_MODE_SHAPES for view, radius in (("floor", 3.0), ("mixed", 30.0))]
RESTATED_IDS = [ssc.case_id(*c) for c in RESTATED_CASES]


@pytest.mark.parametrize("W,H,view,radius", RESTATED_CASES, ids=RESTATED_IDS)
def test_unbiased_spatial_reuse(api, oracle, tris, W, H, view, radius):
    """rt_spatial_unbiased: k_spatial_unbiased runs on the tracing kernels' 8 x 8 tiles and walks shadow rays between lanes of which most
    are off these images; rt_frame and the kernel sequence against the restatement, three frames"""
    differs, shaded = _restated_mode(api, oracle, tris, W, H, view, radius, power=False, unbiased=True)
    print(f"{ssc.case_id(W, H, view, radius)}: unbiased: {differs} final records in 3 frames differ from the reference's pass, {shaded} shaded pixels")
    if view == "floor" and shaded >= 49:
        assert differs > 0  # 1/Z and 1/M differ wherever a neighbour could not have produced the sample


@pytest.mark.parametrize("W,H,view,radius", RESTATED_CASES, ids=RESTATED_IDS)
def test_power_light_sampling(api, oracle, tris, W, H, view, radius):
    """rt_light_sampling(RT_LIGHTS_POWER): the candidates' kernel with the alias table, rt_frame (stage 0 in its launch forms) and the
    kernel sequence against the restatement, three frames"""
    differs, shaded = _restated_mode(api, oracle, tris, W, H, view, radius, power=True, unbiased=False)
    print(f"{ssc.case_id(W, H, view, radius)}: power: {differs} final records in 3 frames differ from uniform selection's, {shaded} shaded pixels")
    if shaded >= 9:
        assert differs > 0  # another light table gives other candidates


# =============================================================================================== e. path tracers and ambient occlusion
PT_CONFIGS = [(7, {}), (8, {}), (9, {}), (9, dict(use_shadowed_target_function=1))]


@pytest.mark.parametrize("W,H", list(ssc.SHAPES), ids=[ssc.case_id(W, H) for W, H in ssc.SHAPES])
def test_path_tracers(api, oracle, tris, W, H):
    """07_pt, 08_nee and 09_ris (unshadowed and shadowed target) in the `mixed` view: one launch per frame, the wavefront form (k_pt_init,
    k_pt_bounce: bounce lists and counters sized from W * H) and auto; max_depth 1 and 6; three accumulating frames: accumulation,
    pixels and the reference's ray count"""
    from cedec_2024_rt_amd.types import default_options

    camera = ssc.camera("mixed", W, H)
    sc, rg, _, _ = _oracle(oracle, tris, W, H, camera, 30.0)
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(camera[0], camera[1], fovy=camera[2])
    lit = 0
    for example, kw in PT_CONFIGS:
        for depth in (1, 6):
            optkw = dict(kw, accumulate=1, max_depth=depth)
            opt = oracle.default_options(**optkw)
            want, per_frame = np.zeros((W * H, 4), np.float32), []
            for frame in ssc.FRAMES:
                cnt = oracle.new_counters()
                sc.path_trace(example, W, H, frame, rg, opt, want, cnt=cnt)
                per_frame.append((want.copy(), oracle.tone_mapping(want, W, H), int(cnt["rays"][0])))
            assert np.isfinite(want).all()
            lit += int((want[:, :3] > 0).any(axis=1).sum())
            r.set_options(default_options(**optkw))
            for wavefront in (0, 1, 2):
                r.tuning(api.Tune.PT_WAVEFRONT, wavefront)
                r.clear()
                for frame, (acc_ref, px_ref, rays) in zip(ssc.FRAMES, per_frame):
                    what = f"{W}x{H} example {example} {kw} max_depth {depth} wavefront {wavefront} frame {frame}"
                    r.path_trace(example, frame)
                    acc = r.download(api.RT_BUF_ACCUMULATION)
                    assert _eq_bits(acc, acc_ref), f"{what}: accumulation: {_first_diff(acc, acc_ref, W)}"
                    r.tone_mapping()
                    assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), px_ref), f"{what}: pixels"
                    assert r.path_trace_rays() == rays, f"{what}: rays"
    if W * H >= 49:
        assert lit > 0
    r.close()


@pytest.mark.parametrize("W,H", list(ssc.SHAPES), ids=[ssc.case_id(W, H) for W, H in ssc.SHAPES])
def test_ambient_occlusion(api, oracle, tris, W, H):
    """04_ao and 06_ao_hiprt in the `mixed` view, pixel-major and ray-major (64 rays of a pixel on the 64 lanes of a wavefront: the
    layout's lists are sized from W * H): every byte of the image against the oracle's o_ao_04 (tests/test_gpu_ao.py's reference),
    the reference's ray count, and the accumulation buffer left alone"""
    camera = ssc.camera("mixed", W, H)
    sc, rg, _, _ = _oracle(oracle, tris, W, H, camera, 30.0)
    want = np.asarray(sc.ao_04(W, H, rg)).reshape(H, W, 4)
    rays = W * H + 64 * int((want[..., 0] != 32).sum())  # 32 is no hit value: 0/64 -> 0, 1/64 -> 38 (tests/test_gpu_ao.py)
    if W * H >= 49:
        assert (want[..., 0] != 32).any() and (want[..., 0] == 32).any()  # hit pixels and sky
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(camera[0], camera[1], fovy=camera[2])
    r.clear()
    for example in (4, 6):
        for layout in (0, 1):
            r.tuning(api.Tune.AO_LAYOUT, layout)
            px = r.ambient_occlusion(example)
            what = f"{W}x{H} example {example} layout {layout}"
            assert np.array_equal(px, want), f"{what}: {int((px != want).any(axis=-1).sum())} pixels differ from o_ao_04"
            assert r.path_trace_rays() == rays, f"{what}: rays"
            assert not r.download(api.RT_BUF_ACCUMULATION).any(), f"{what}: the accumulation buffer was written"
    r.close()


# =============================================================================================== f. thin strips
STRIP_EYE_2 = (0.9, 2.6, 1.6)  # the camera of frame 3: same look-at point and field of view
_strip_refs = {}


def _strip_cameras(W, H):
    eye, at, fovy = ssc.camera("floor", W, H)
    return (eye, at, fovy), (STRIP_EYE_2, at, fovy)


def _strip_halo(radius):
    from cedec_2024_rt_amd import strips

    return math.ceil(strips.halo_bound(radius))


def _strip_reference(oracle, tris, case):
    """per case, once: the oracle's frames 1, 2 and, after the camera move and a clear, 3, accumulating; read-only"""
    if case not in _strip_refs:
        W, H, radius, _ = ssc.STRIP_CASES[case]
        out = []
        st = oracle.new_state(W, H)
        for frame in ssc.FRAMES:
            sc, rg, opt, eyev = _oracle(oracle, tris, W, H, _strip_cameras(W, H)[frame == 3], radius, accumulate=1)
            if frame == 3:
                oracle.clear(st["accum"], W, H)
            cnt = oracle.new_counters()
            sc.frame(W, H, frame, rg, eyev, opt, st, cnt)
            shaded = _shaded(sc, st["vis"])
            assert 2 * int(shaded.sum()) > W * H, f"{case}: frame {frame}: most pixels should be shaded"
            accum, pixels, temporal, shaded = _frozen(st["accum"].reshape(W * H, 4), st["pixels"], st["temporal"], shaded)
            out.append(dict(accum=accum, pixels=pixels, temporal=temporal, shaded=shaded, rays=int(cnt["rays"][0])))
        _strip_refs[case] = out
    return _strip_refs[case]


def _move_camera(contexts, W, H):
    eye, at, fovy = _strip_cameras(W, H)[1]
    for c in contexts:
        c.lookat(eye, at, fovy=fovy)


def _check_strips(api, full, ctxs, bounds, W, H, what):
    """every strip's owned rows of accumulation, pixels and temporal history == the whole-frame context's; the rays add up"""
    ref = full.download(api.RT_BUF_ACCUMULATION).reshape(H, W, 4)
    refpx = full.download(api.RT_BUF_PIXELS).reshape(H, W, 4)
    refhist = full.download(api.RT_BUF_RES_TEMPORAL).reshape(H, W)
    for c, (a, b) in zip(ctxs, bounds):
        own = slice(a - c.local_row0, b - c.local_row0)
        acc = c.download(api.RT_BUF_ACCUMULATION).reshape(c.local_rows, W, 4)[own]
        assert _eq_bits(acc, ref[a:b]), f"{what}: rows {a}:{b}: accumulation: {_first_diff(acc.reshape(-1, 4), ref[a:b].reshape(-1, 4), W)} of the strip"
        assert np.array_equal(c.download(api.RT_BUF_PIXELS).reshape(c.local_rows, W, 4)[own], refpx[a:b]), f"{what}: rows {a}:{b}: pixels"
        assert _eq_bits(c.download(api.RT_BUF_RES_TEMPORAL).reshape(c.local_rows, W)[own], refhist[a:b]), f"{what}: rows {a}:{b}: temporal history"
    assert sum(c.ray_count()[0] for c in ctxs) == full.ray_count()[0], f"{what}: rays"


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("case", list(ssc.STRIP_CASES))
def test_thin_strips_python_driver(api, oracle, tris, case, sparse):
    """strips.run_frame_local with halos of 1, 9 and 29 rows: rt_halo_flags_*, rt_halo_mark, the scans and the sparse pack / unpack (or the
    dense halos) on regions down to one row of one pixel; frames 1 to 3 with a camera move and a clear before frame 3"""
    import torch

    from cedec_2024_rt_amd import strips

    W, H, radius, bounds = ssc.STRIP_CASES[case]
    halo = _strip_halo(radius)
    assert halo == ssc.STRIP_RADII[radius] and min(b - a for a, b in bounds) == halo
    refs = _strip_reference(oracle, tris, case)
    cam = _strip_cameras(W, H)[0]
    full = _renderer(api, tris, W, H, cam, radius, accumulate=1)
    ctxs = [_renderer(api, tris, W, H, cam, radius, rows=b, halo=halo, accumulate=1) for b in bounds]
    stats = []
    try:
        for frame in ssc.FRAMES:
            if frame == 3:
                _move_camera([full] + ctxs, W, H)
            full.frame(frame, clear_first=frame == 3)
            strips.run_frame_local(ctxs, bounds, frame, torch.device("cuda:0"), halo=halo, sparse=sparse, stats=stats, clear_first=frame == 3)
            what = f"{case} {'sparse' if sparse else 'dense'} frame {frame}"
            _check_against(api, full, refs[frame - 1], W, H, f"{what}: the whole frame against the oracle")
            _check_strips(api, full, ctxs, bounds, W, H, what)
        if sparse:
            sent, of = sum(s[0] for s in stats), sum(s[1] for s in stats)
            print(f"{case}: {sent} of {of} halo records travelled")
            assert 0 < sent <= of
    finally:
        for c in [full] + ctxs:
            c.close()


class _ThinRig(_Rig):
    """tests/test_mg_native.py's _Rig (a whole-frame context, the strip contexts and their native drivers over the LOCAL transport)
    with the case's camera, radius and halo"""

    def __init__(self, api, tris, case, flags):
        from cedec_2024_rt_amd.types import bench_options

        W, H, radius, bounds = ssc.STRIP_CASES[case]
        halo = _strip_halo(radius)
        cam = _strip_cameras(W, H)[0]
        self.api, self.W, self.H, self.bounds = api, W, H, bounds
        self.opt = bench_options(spatial_resampling_radius=radius, accumulate=1)
        self.full = _renderer(api, tris, W, H, cam, radius, accumulate=1)
        self.ctxs = [_renderer(api, tris, W, H, cam, radius, rows=b, halo=halo, accumulate=1) for b in bounds]
        self.hub = api.MgHub(len(bounds), renderer=self.ctxs[0])
        self.mgs = [api.MultiGpu(c, k, bounds, transport=api.RT_MG_TRANSPORT_LOCAL, hub=self.hub, flags=flags) for k, c in enumerate(self.ctxs)]


@pytest.mark.parametrize("flags", ssc.MG_FLAGS, ids=[f"flags{f}" for f in ssc.MG_FLAGS])
@pytest.mark.parametrize("case", list(ssc.STRIP_CASES))
def test_thin_strips_native_driver(api, oracle, tris, case, flags):
    """rt_mg over the LOCAL hub: sparse halos packed by the passes (0), dense halos (RT_MG_DENSE), one lane (RT_MG_ONE_LANE), packs and
    unpacks as launches of their own (RT_MG_SEPARATE_PACK); frame 2 rides on the plan frame 1 prepared, frame 3 is cold (camera move)"""
    W, H, radius, bounds = ssc.STRIP_CASES[case]
    refs = _strip_reference(oracle, tris, case)
    rig = _ThinRig(api, tris, case, flags)
    try:  # a failed comparison must not leave the drivers to the garbage collector: they go before their contexts (_Rig.close)
        for frame in ssc.FRAMES:
            if frame == 3:
                _move_camera(rig.everyone(), W, H)
            rig.frame(frame, clear_first=frame == 3)
            what = f"{case} flags {flags} frame {frame}"
            _check_against(api, rig.full, refs[frame - 1], W, H, f"{what}: the whole frame against the oracle")
            _check_strips(api, rig.full, rig.ctxs, bounds, W, H, what)
        st = [m.stats() for m in rig.mgs]
        assert all(s["frames"] == 3 for s in st), st
        if not flags & api.RT_MG_DENSE:
            assert all(s["cold_frames"] == 2 for s in st), st  # frame 1 (no plan) and frame 3 (the camera moved)
            assert sum(s["records_sent"] for s in st) > 0, st
    finally:
        rig.close()


def test_a_strip_shorter_than_its_halo_is_refused(api, tris):
    """rt_mg_partition and rt_mg_create answer RT_ERR_ARG where a strip would be shorter than the halo (a halo must not reach beyond the
    adjacent strip), and say which strip; nothing is rendered"""
    from cedec_2024_rt_amd import strips

    W, H, radius, halo = 5, 17, 3.0, 9
    assert _strip_halo(radius) == halo
    L = api.load_library()
    out = np.zeros(3, np.int32)
    assert L.rt_mg_partition(H, 2, halo, None, out.ctypes.data) == RT_ERR_ARG
    assert L.rt_mg_partition(H + 1, 2, halo, None, out.ctypes.data) == 0 and out.tolist() == [0, 9, 18]
    with pytest.raises(ValueError, match="thinner than the 9-row halo"):
        api.mg_partition(H, 2, halo)
    with pytest.raises(ValueError, match="thinner than the 9-row halo"):
        strips.partition_rows(H, 2, halo=halo)
    bounds = [(0, 9), (9, 17)]
    cam = _strip_cameras(W, H)[0]
    ctxs = [_renderer(api, tris, W, H, cam, radius, rows=b, halo=halo) for b in bounds]
    hub = api.MgHub(2, renderer=ctxs[0])
    for k, c in enumerate(ctxs):
        with pytest.raises(api.RtError, match=rf"rt_mg_create -> {RT_ERR_ARG}: strip 1 has 8 rows, fewer than the 9-row halo"):
            api.MultiGpu(c, k, bounds, transport=api.RT_MG_TRANSPORT_LOCAL, hub=hub)
        with pytest.raises(api.RtError, match=rf"error {RT_ERR_STATE}: no G-buffer yet"):
            c.ray_count()  # no frame ran on the context
    hub.close()
    for c in ctxs:
        c.close()
