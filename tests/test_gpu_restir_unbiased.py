"""rt_spatial_unbiased on the device: k_spatial_unbiased against tests/restir_unbiased_ref.py (the restatement compiled from the
kernel's own headers, anchored to the oracle by tests/test_restir_unbiased_cpu.py), bit for bit: every field of every record after
every pass, then the accumulation buffer and the pixels. Everything around the pass (primary rays, candidates, temporal merge,
resolve, tone mapping) is the oracle's, as in tests/test_gpu_parity.py.

Sizes: 64 x 48 (whole tiles), 37 x 29 (partial tiles in both directions), 8 x 8 (one tile, one wavefront), 200 x 120 (a radius-30
window crosses several tile rows and the XCD interleave wraps)."""
import ctypes as C

import numpy as np
import pytest

import restir_unbiased_ref as ru

pytestmark = pytest.mark.gpu

EYE, AT, FOVY = (0.5, 3.0, 6.0), (0.0, 1.0, -1.5), np.float32(0.9)
RT_ERR_UNSUPPORTED = 5  # include/restir_rt.h


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _eq_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _res_diff(a, b, mask):
    """fields of two reservoir arrays (padding excluded) that differ on `mask`, with the number of records"""
    bad = []
    for f in a.dtype.names:
        if f == "pad":
            continue
        x, y = np.ascontiguousarray(a[f][mask]), np.ascontiguousarray(b[f][mask])
        if not _eq_bits(x, y):
            bad.append((f, int((_bits(x).reshape(len(x), -1) != _bits(y).reshape(len(y), -1)).any(axis=1).sum())))
    return bad


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


def _soup():
    """a random soup: triangles of very different sizes around the origin, a third of them lights"""
    from cedec_2024_rt_amd.types import TRIANGLE

    rng = np.random.default_rng(15)
    n = 150
    t = np.zeros(n, TRIANGLE)
    c = rng.normal(size=(n, 1, 3)).astype(np.float32) * np.float32(3.0)
    size = np.float32(10.0) ** rng.uniform(-1.0, 0.6, size=(n, 1, 1)).astype(np.float32)
    t["v"] = (c + rng.normal(size=(n, 3, 3)).astype(np.float32) * size).astype(np.float32)
    t["color"] = rng.random((n, 3), dtype=np.float32)
    lights = rng.random(n) < 0.3
    lights[0] = True
    t["emissive"][lights] = (rng.random((int(lights.sum()), 3), dtype=np.float32) * np.float32(20.0)).astype(np.float32)
    return t


@pytest.fixture(scope="module")
def worlds(oracle):
    from cedec_2024_rt_amd import scenes

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    out = {}
    for name, tris, eye, at in (("room", scenes.make_quad_room(), EYE, AT), ("soup", _soup(), (1.0, 2.0, 9.0), (0.0, 0.0, 0.0)),
                                ("ledge", ru.make_ledge(oracle.TRIANGLE), ru.LEDGE_EYE, ru.LEDGE_AT)):
        out[name] = dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True), eye=eye, at=at)
    return out


class _Cpu:
    """the frame of 10_restir_di.cpp:257-379 on the CPU: the oracle's kernels, with the spatial pass from the restatement"""

    def __init__(self, oracle, world, W, H, opt, unbiased=True):
        self.o, self.w, self.W, self.H, self.opt, self.unbiased = oracle, world, W, H, opt, unbiased
        self.rg = oracle.raygen_lookat(world["eye"], world["at"], (0, 1, 0), FOVY, W, H)
        self.st = oracle.new_state(W, H)
        self.eye = np.asarray(world["eye"], np.float32)
        world["scene"].raycast(W, H, self.rg, self.st["vis"])
        e = world["tris"]["emissive"]
        vis = self.st["vis"]
        self.shaded = (vis["index"] >= 0) & ~(e > 0).any(axis=1)[np.maximum(vis["index"], 0)]
        self.by_geometry = 0  # neighbours with Mk > 0 that the geometry term kept out of Z, without a ray

    def spatial(self, frame, pas, rin):
        if self.unbiased:
            out, diag = ru.spatial(self.W, self.H, frame, pas, self.w["tris"], self.st["vis"], self.eye, self.opt, rin)
            self.by_geometry += int(np.count_nonzero(diag[:, 2]))
            return out
        return self.w["scene"].spatial_resampling(self.W, self.H, frame, pas, self.st["vis"], self.eye, self.opt, rin)

    def frame(self, frame, check=None):
        """check(step, reservoirs or None): called after every kernel"""
        sc, st, W, H, opt = self.w["scene"], self.st, self.W, self.H, self.opt
        check = check or (lambda *a: None)
        sc.generate_candidate(W, H, frame, st["vis"], self.eye, opt, st["r0"])
        check("generate_candidate", st["r0"])
        sc.temporal_resampling(W, H, frame, st["vis"], self.eye, opt, st["temporal"], st["r0"])
        check("temporal_resampling", st["r0"])
        self.o.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        src, dst = "r0", "r1"
        for k in range(int(opt["spatial_resampling_passes"][0])):
            if k:
                src, dst = dst, src
            st[dst] = self.spatial(frame, k, st[src])
            check(f"spatial pass {k}", st[dst])
        sc.resolve(st["accum"], W, H, st["vis"], self.eye, opt, st[dst])
        check("resolve", None)
        st["pixels"] = self.o.tone_mapping(st["accum"], W, H)
        return st[dst]


def _renderer(api, world, W, H, opt, unbiased=True, **kw):
    r = api.Renderer(W, H, **kw)
    r.set_scene(world["tris"])
    r.lookat(world["eye"], world["at"], fovy=FOVY)
    r.set_options(opt)
    if unbiased:
        assert r.spatial_unbiased(True) is True
    return r


CASES = [
    # world, W, H, use_visibility_reuse, neighbours, radius, passes, temporal (then 4 frames)
    ("room", 64, 48, 1, 5, 30.0, 3, 0),
    ("room", 37, 29, 1, 3, 5.0, 2, 0),
    ("room", 8, 8, 1, 5, 5.0, 1, 0),
    ("room", 200, 120, 1, 5, 30.0, 3, 0),
    ("room", 64, 48, 0, 5, 30.0, 3, 0),
    ("room", 37, 29, 0, 1, 30.0, 1, 1),
    ("room", 64, 48, 1, 5, 30.0, 3, 1),
    ("room", 200, 120, 0, 3, 5.0, 2, 1),
    ("soup", 64, 48, 1, 5, 30.0, 3, 0),
    ("soup", 37, 29, 0, 3, 5.0, 2, 1),
    ("soup", 64, 48, 1, 1, 30.0, 3, 1),
    ("soup", 8, 8, 0, 5, 30.0, 2, 0),
    # a lamp in the floor's plane: the geometry term alone keeps floor neighbours out of a ramp pixel's Z, in either setting
    ("ledge", 64, 48, 1, 5, 30.0, 3, 0),
    ("ledge", 37, 29, 0, 5, 30.0, 2, 1),
    # past the reference's defaults (tests/test_gpu_option_space.py): pass indices 3 and 4, a reach of 130 px
    ("room", 64, 48, 1, 5, 45.0, 5, 1),
    ("soup", 37, 29, 0, 3, 45.0, 4, 0),
]


@pytest.mark.parametrize("name,W,H,vis_reuse,count,radius,passes,temporal", CASES)
def test_kernel_sequence_equals_the_restatement(api, oracle, worlds, name, W, H, vis_reuse, count, radius, passes, temporal):
    world = worlds[name]
    kw = dict(use_spatial_resampling=1, use_temporal_resampling=temporal, use_visibility_reuse=vis_reuse, accumulate=temporal,
              spatial_resampling_sample_count=count, spatial_resampling_radius=radius, spatial_resampling_passes=passes)
    opt = oracle.default_options(**kw)
    cpu = _Cpu(oracle, world, W, H, opt)
    assert cpu.shaded.any()
    r = _renderer(api, world, W, H, opt)
    assert _eq_bits(cpu.rg, r.raygen())
    merged = 0
    for frame in range(1, 5 if temporal else 2):
        r.raycast()
        assert _eq_bits(r.download(api.RT_BUF_VISIBILITY), cpu.st["vis"]), f"frame {frame}: raycast"
        r.generate_candidate(frame, api.RT_RES_0)
        got = {}
        got["generate_candidate"] = r.download(api.RT_BUF_RES_0)
        r.temporal_resampling(frame, api.RT_RES_TEMPORAL, api.RT_RES_0)
        got["temporal_resampling"] = r.download(api.RT_BUF_RES_0)
        r.save_temporal_reservoir(api.RT_RES_0, api.RT_RES_TEMPORAL)
        src, dst = api.RT_RES_0, api.RT_RES_1
        for k in range(passes):
            if k:
                src, dst = dst, src
            r.spatial_resampling(frame, k, src, dst)
            got[f"spatial pass {k}"] = r.download(api.RT_BUF_RES_0 + dst)
        r.resolve(dst)
        r.tone_mapping()

        def check(step, res):
            if res is None:
                return
            bad = _res_diff(got[step], res, cpu.shaded)
            assert not bad, f"frame {frame}: {step}: {bad} of {int(cpu.shaded.sum())} shaded pixels"
            if step.startswith("spatial"):
                # sky and emissive pixels: the pass writes an empty record, all 76 bytes
                assert not _bits(got[step][~cpu.shaded]).any(), f"frame {frame}: {step}: records at unshaded pixels"
                assert not _bits(res[~cpu.shaded]).any()

        last = cpu.frame(frame, check)
        merged += int((last["M"][cpu.shaded] > 0).sum())
        acc = r.download(api.RT_BUF_ACCUMULATION)
        assert _eq_bits(acc, cpu.st["accum"].reshape(acc.shape)), f"frame {frame}: accumulation"
        assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), cpu.st["pixels"]), f"frame {frame}: pixels"
    assert merged > 0
    if name == "ledge":
        assert cpu.by_geometry > 0, "the geometry term decided nothing: the case would not cover its branch"
    r.close()


def test_frame_equals_the_kernel_sequence_and_the_restatement(api, oracle, worlds):
    """rt_frame over 6 frames with temporal reuse on: the staged frame hands the own ray's answer to resolve through the
    own-visibility flags, the per-kernel sequence walks every ray"""
    world, W, H = worlds["room"], 64, 48
    opt = oracle.bench_options(accumulate=1)
    cpu = _Cpu(oracle, world, W, H, opt)
    rf, rk = _renderer(api, world, W, H, opt), _renderer(api, world, W, H, opt)
    for frame in range(1, 7):
        out_f = rf.frame(frame)
        out_k = rk.frame_by_kernels(frame)
        last = cpu.frame(frame)
        for what, r, out in (("rt_frame", rf, out_f), ("frame_by_kernels", rk, out_k)):
            acc = r.download(api.RT_BUF_ACCUMULATION)
            assert _eq_bits(acc, cpu.st["accum"].reshape(acc.shape)), f"{what} frame {frame}: accumulation"
            assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), cpu.st["pixels"]), f"{what} frame {frame}: pixels"
            bad = _res_diff(r.download(api.RT_BUF_RES_0 + out), last, cpu.shaded)
            assert not bad, f"{what} frame {frame}: resolved reservoirs {bad}"
            bad = _res_diff(r.download(api.RT_BUF_RES_TEMPORAL), cpu.st["temporal"], cpu.shaded)
            assert not bad, f"{what} frame {frame}: temporal history {bad}"
    # and the mode does something: the reference's pass gives other records
    biased = _Cpu(oracle, world, W, H, opt, unbiased=False)
    assert _res_diff(biased.frame(1), _Cpu(oracle, world, W, H, opt).frame(1), cpu.shaded)
    rf.close(), rk.close()


def _epoch(r):
    e = C.c_uint64()
    assert r.L.rt_state_epoch(r.h, C.byref(e)) == 0
    return e.value


def test_on_then_off_equals_a_context_that_never_had_the_mode(api, oracle, worlds):
    world, W, H = worlds["room"], 64, 48
    opt = oracle.bench_options()
    a, b = _renderer(api, world, W, H, opt, unbiased=False), _renderer(api, world, W, H, opt, unbiased=False)
    assert a.spatial_unbiased() is False
    e0 = _epoch(a)
    assert a.spatial_unbiased(True) is True and _epoch(a) != e0
    a.frame(1), b.frame(1)
    assert not _eq_bits(a.download(api.RT_BUF_ACCUMULATION), b.download(api.RT_BUF_ACCUMULATION))
    e1 = _epoch(a)
    assert a.spatial_unbiased(False) is False and _epoch(a) != e1
    # the history is saved before the spatial passes, so the unbiased frame left the same one behind; only the accumulation differs
    for frame in (2, 3):
        oa, ob_ = a.frame(frame, clear_first=frame == 2), b.frame(frame, clear_first=frame == 2)
        assert oa == ob_
        for buf in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0 + oa):
            assert _eq_bits(a.download(buf), b.download(buf)), f"frame {frame}: buffer {buf}"
    a.close(), b.close()


@pytest.mark.parametrize("keys", [((0, 1), (1, 2), (2, 3), (3, 5)), ((2, 1), (13, 1), (17, 0)), ((2, 7), (13, 0), (14, 0), (20, 0), (25, 0)),
                                  ((14, 2), (17, 1), (25, 1), (2, 4))])
def test_tuning_keys_leave_the_output_unchanged(api, oracle, worlds, keys):
    world, W, H = worlds["room"], 100, 76
    opt = oracle.bench_options()
    plain, tuned = _renderer(api, world, W, H, opt), _renderer(api, world, W, H, opt)
    for k, v in keys:
        tuned.tuning(k, v)
    for frame in (1, 2, 3):
        op, ot = plain.frame(frame), tuned.frame(frame)
        assert op == ot
        for buf in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0 + op):
            assert _eq_bits(plain.download(buf), tuned.download(buf)), f"keys {keys} frame {frame}: buffer {buf}"
    plain.close(), tuned.close()


def test_error_codes(api, oracle, worlds):
    world, W, H = worlds["room"], 64, 48
    strip = api.Renderer(W, H, rows=(0, 24), halo=8)
    with pytest.raises(api.RtError) as e:
        strip.spatial_unbiased(True)
    assert f"error {RT_ERR_UNSUPPORTED}:" in str(e.value), str(e.value)
    strip.close()
    for kw in (dict(use_shadowed_target_function=1), dict(spatial_resampling_sample_count=6, spatial_resampling_passes=2)):
        r = _renderer(api, world, W, H, oracle.bench_options(**kw))
        r.raycast()
        r.generate_candidate(1, api.RT_RES_0)
        assert r.L.rt_spatial_resampling(r.h, 1, 0, api.RT_RES_0, api.RT_RES_1) == RT_ERR_UNSUPPORTED, kw
        out = C.c_int(-1)
        assert r.L.rt_frame(r.h, 1, 0, C.byref(out)) == RT_ERR_UNSUPPORTED, kw
        # with spatial reuse off the pass copies its input in either mode
        r.set_options(oracle.bench_options(use_spatial_resampling=0, **kw))
        r.frame(1)
        r.close()
