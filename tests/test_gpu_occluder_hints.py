"""rt_occluder_hints: the candidates of a staged frame test the triangles that occluded their pixel's earlier shadow rays before they
walk the BVH (csrc/occluder_hint.h).

A remembered triangle is tested exactly, with the ray's own origin, direction and range, so the images cannot depend on the switch nor
on what the hint buffer holds: every comparison of test 1 is bit for bit, after every frame. 100 x 76 on the bench scene, as
tests/test_gpu_gbuffer_reuse.py: a width off the 8-pixel tile, more than eight tile rows, a partial last tile row.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 100, 76
EYE2 = (-1.25, 22.6, -6.1)
AT2 = (5.0, 20.5, 1.9)
RADIUS2 = 17.0
ROOM_EYE, ROOM_AT = (0.5, 2.5, 6.0), (0.0, 1.5, -1.0)  # the quad room as __graft_entry__.smoke() sees it
N_FRAMES = 20


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def scenes():
    from cedec_2024_rt_amd import scenes as s

    return s


@pytest.fixture(scope="module")
def world(scenes):
    """the bench scene, the same with the first half of the light span moved, and a room of a few dozen triangles"""
    A = scenes.make_blocks_restir()
    lights = scenes.light_indices(A)
    lo, hi = int(lights.min()), int(lights.max()) + 1
    mid = lo + max(1, (hi - lo) // 2)
    mask = np.zeros(len(A), bool)
    mask[lights[lights < mid]] = True
    assert mask.any()
    B = scenes.move_triangles(A, mask, (0.25, 0.125, -0.5))
    room = scenes.make_quad_room()
    assert len(room) < 100 < len(A)  # every index remembered on the bench scene is out of the room's range
    return dict(A=A, B=B, room=room, lo=lo, mid=mid, eye=scenes.BLOCKS_RESTIR_EYE, at=scenes.BLOCKS_RESTIR_LOOKAT)


def _renderer(api, world, tune=(), reuse=True, hints=True):
    from cedec_2024_rt_amd.types import bench_options

    r = api.Renderer(W, H)
    r.set_scene(world["A"])
    r.lookat(world["eye"], world["at"])
    r.set_options(bench_options())
    for k, v in tune:
        r.tuning(k, v)
    if not reuse:
        r.gbuffer_reuse(False)
    if not hints:
        r.occluder_hints(False)
    return r


def _snapshot(api, r):
    return dict(acc=r.download(api.RT_BUF_ACCUMULATION), pix=r.download(api.RT_BUF_PIXELS), hist=r.download(api.RT_BUF_RES_TEMPORAL))


def _same(a, b, what):
    for k in ("acc", "pix"):
        assert _eq_bits(a[k], b[k]), f"{what}: {k}: {int((np.ascontiguousarray(a[k]).view(np.uint8) != np.ascontiguousarray(b[k]).view(np.uint8)).sum())} bytes differ"
    for f in a["hist"].dtype.names:
        if f != "pad":
            assert _eq_bits(a["hist"][f], b["hist"][f]), f"{what}: temporal history, field {f}"


def _script(api, world, r, step):
    """frames 1-4; lookat, 5-7; update_scene of half the light span, 8-10; set_options, 11-12; set_scene(the quad room, with its camera),
    13-15; set_scene back to the bench scene (and its camera), 16-20. Returns the buffers after every frame."""
    from cedec_2024_rt_amd.types import bench_options

    snaps = []
    for f in range(1, N_FRAMES + 1):
        if f == 5:
            r.lookat(EYE2, AT2)
        if f == 8:
            r.update_scene(world["B"][world["lo"]:world["mid"]], world["lo"])
        if f == 11:
            r.set_options(bench_options(spatial_resampling_radius=RADIUS2))
        if f == 13:
            r.set_scene(world["room"])
            r.lookat(ROOM_EYE, ROOM_AT)
        if f == 16:
            r.set_scene(world["A"])
            r.lookat(EYE2, AT2)
        step(f)
        snaps.append(_snapshot(api, r))
    return snaps


@pytest.fixture(scope="module")
def kernel_sequence(api, world):
    """the script through frame_by_kernels (the reference's launch sequence: rt_generate_candidate gets no hint buffer), computed once"""
    r = _renderer(api, world)
    out = _script(api, world, r, r.frame_by_kernels)
    r.close()
    return out


@pytest.mark.parametrize("look_ahead", [False, True], ids=["tuning14_0", "tuning14_default"])
@pytest.mark.parametrize("reuse", [True, False], ids=["gbuffer_reuse", "tracing_frames"])
def test_bit_identity_after_every_frame(api, world, kernel_sequence, reuse, look_ahead):
    tune = () if look_ahead else ((api.Tune.SPEC, 0),)
    runs = {}
    for hints in (True, False):
        r = _renderer(api, world, tune, reuse=reuse, hints=hints)
        runs[hints] = _script(api, world, r, r.frame)
        r.close()
    for f in range(1, N_FRAMES + 1):
        _same(runs[True][f - 1], runs[False][f - 1], f"frame {f} against occluder_hints(False)")
        _same(runs[True][f - 1], kernel_sequence[f - 1], f"frame {f} against frame_by_kernels")
        _same(runs[False][f - 1], kernel_sequence[f - 1], f"frame {f}, hints off, against frame_by_kernels")


def test_the_hints_settle_rays_before_the_walk(api, world):
    """steady frames 9-12: generate_candidate walks at most 0.85 times the rays it walks without hints. The CPU simulation with ONE
    remembered triangle gives 0.72-0.74 at this size on these frames and 0.35-0.40 with four; the bound leaves room for an any-hit walk
    that remembers another occluder than the closest one, and fails on a record that is never written or never read."""
    stats = {}
    for hints in (True, False):
        r = _renderer(api, world, ((api.Tune.SPEC, 0), (api.Tune.TAIL, 0)), hints=hints)
        for f in range(1, 13):
            if f == 9:
                r.walk_stats_enable(True)
            r.frame(f)
        stats[hints] = (r.walk_stats()["generate_candidate"], r.occluder_hint_stats())
        r.walk_stats_enable(False)
        r.close()
    (on, hs_on), (off, hs_off) = stats[True], stats[False]
    print("hints on ", on, hs_on)
    print("hints off", off, hs_off)
    for g in (on, off):
        assert g["reference_rays"] > 0 and g["reference_rays"] == g["walked"] + g["self_test"] + g["not_evaluated"], g
    assert on["reference_rays"] == off["reference_rays"]
    assert on["not_evaluated"] == off["not_evaluated"]
    assert on["walked"] <= 0.85 * off["walked"], (on, off)
    # the rays the hints settled are the ones that left the walk, and they count as one-triangle tests
    assert hs_on["settled"] == off["walked"] - on["walked"] == on["self_test"] - off["self_test"], (hs_on, on, off)
    assert hs_on["settled"] <= hs_on["rays_with_hint"] <= hs_on["tests"] <= 4 * hs_on["rays_with_hint"], hs_on
    assert hs_off == dict(rays_with_hint=0, settled=0, tests=0), hs_off


def test_the_walk_names_a_triangle_that_occludes_the_ray(api, oracle, world):
    """4096 segments between random points of the scene's box, through the work-sharing any-hit walk asked for its occluder: every
    triangle it names is one the oracle's intersect_ray_triangle accepts for that ray, and it names one iff the walk says occluded"""
    A = world["A"]
    v = A["v"].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    rng = np.random.default_rng(19)
    n = 4096
    p0 = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    p1 = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    rays = np.concatenate([p0, p1 - p0, np.zeros((n, 1), np.float32), np.ones((n, 1), np.float32)], axis=1).astype(np.float32)
    r = _renderer(api, world)
    tri = r.trace_occluders(rays)
    r.trace_mode(api.TraceMode.OCCLUDED_WS)
    occluded = r.trace_closest(rays).view(np.int32)[:, 3] >= 0
    r.trace_mode(api.TraceMode.WIDE)
    r.close()
    print("occluded", float(occluded.mean()))
    assert 0.2 < occluded.mean() < 0.8  # 0.36 on this scene: both answers are exercised
    assert np.array_equal(tri >= 0, occluded)
    assert tri.max() < len(A) and tri.min() >= -1
    named = np.nonzero(tri >= 0)[0]
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    got = oracle.fn_bulk("intersect_ray_triangle", np.concatenate([rays[named], A["v"][tri[named]].reshape(-1, 9)], axis=1))
    assert (got[:, 0] == 1).all(), f"{int((got[:, 0] != 1).sum())} of {len(named)} named triangles do not occlude their ray"


def test_an_all_visible_scene_tests_nothing(api):
    """a floor and one light above it: no candidate ray is ever occluded by the walk, so no record is ever written and none is tested"""
    from cedec_2024_rt_amd.types import TRIANGLE, bench_options

    t = np.zeros(4, TRIANGLE)
    t["v"][0] = [[-10, 0, -10], [-10, 0, 10], [10, 0, 10]]
    t["v"][1] = [[-10, 0, -10], [10, 0, 10], [10, 0, -10]]
    t["v"][2] = [[-0.5, 3, -0.5], [0.5, 3, 0.5], [-0.5, 3, 0.5]]
    t["v"][3] = [[-0.5, 3, -0.5], [0.5, 3, -0.5], [0.5, 3, 0.5]]
    t["color"] = 0.5
    t["emissive"][2:] = 10.0
    r = api.Renderer(W, H)
    r.set_scene(t)
    r.lookat((0.0, 1.0, 4.0), (0.0, 0.0, 0.0))
    r.set_options(bench_options())
    r.walk_stats_enable(True)
    for f in range(1, 7):
        r.frame(f)
    g, hs = r.walk_stats()["generate_candidate"], r.occluder_hint_stats()
    r.close()
    print(g, hs)
    assert g["walked"] > 1000, g  # the floor is in view and its candidates walk
    assert hs == dict(rays_with_hint=0, settled=0, tests=0), hs
