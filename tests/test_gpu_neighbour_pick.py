"""GPU. The neighbour pick of the unshadowed spatial pass (csrc/neighbour_pick.h, rt_neighbour_pick): the hardware's log2 / sqrt / sin /
cos behind an interval guard must give the bytes the portable functions give.

* frames: 97 x 61 and 200 x 120 (no multiples of the 8 x 8 / 32 x 8 tiles), 3 frames with temporal + spatial reuse, radius 30 and 86,
  5 and 1 neighbours: every reservoir buffer after every pass and the accumulation buffer are the same bytes in mode 1 (default),
  mode 0 (portable functions only) and mode 2 (guard forced to fail), and the default equals the oracle as tests/test_gpu_parity.py
  compares it (records on the shaded pixels field by field, accumulation bit for bit);
* strips: 200 x 120 as two strips over the LOCAL transport (the pass's FUSED form; radius 20, so that a 60-row strip holds its
  halo), every mode against the whole frame;
* the pick itself on the device: 2^16 (rv0, rv1) pairs whose values include the 512 smallest and the 512 largest draws, crossed with
  x in {0, 1, 959, 1919, 3839}: where the guard passes its integers are the exact ones, and neighbour_pick equals the exact pick;
* the cap: on the 200 x 120 frame at radius 30 at most 2 % of the picks are near ties (and mode 2 counts all, mode 0 none).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOVY = np.float32(np.pi) / np.float32(4)
MODES = (1, 0, 2)  # default first


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def worlds(golden_dir):
    from cedec_2024_rt_amd import scenes as s

    g = np.load(os.path.join(golden_dir, "scenes.npz"))
    return {"quad_room": (s.make_quad_room(), (0.5, 2.5, 6.0), (0.0, 1.5, -1.0)),
            "cornellbox1": (g["cornellbox1"], s.DEFAULT_EYE, s.DEFAULT_LOOKAT)}


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _res_fields_differ(a, b, mask):
    """reservoir arrays field by field (padding excluded) on the masked pixels, as tests/test_gpu_parity.py compares them"""
    bad = []
    for f in a.dtype.names:
        if f == "pad":
            continue
        x, y = np.ascontiguousarray(a[f][mask]), np.ascontiguousarray(b[f][mask])
        if not _eq_bits(x, y):
            bad.append((f, int((x.reshape(len(x), -1) != y.reshape(len(y), -1)).any(axis=1).sum())))
    return bad


def _renderer(api, world, W, H, optkw, mode, rows=None, halo=0):
    from cedec_2024_rt_amd.types import bench_options

    tris, eye, center = world
    r = api.Renderer(W, H, rows=rows, halo=halo) if rows is not None else api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(eye, center)
    r.set_options(bench_options(**optkw))
    r.neighbour_pick(mode)
    return r


@pytest.mark.parametrize("count", [5, 1])
@pytest.mark.parametrize("radius", [30.0, 86.0])
@pytest.mark.parametrize("W,H,scene", [(97, 61, "cornellbox1"), (200, 120, "quad_room")])
def test_every_buffer_after_every_pass_is_the_same_in_every_mode_and_the_oracles(api, oracle, worlds, W, H, scene, radius, count):
    optkw = dict(spatial_resampling_radius=radius, spatial_resampling_sample_count=count)
    world = worlds[scene]
    tris, eye, center = world
    ctx = [_renderer(api, world, W, H, optkw, m) for m in MODES]
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    sc = oracle.Scene(tris, use_bvh=True)
    rg = oracle.raygen_lookat(eye, center, (0, 1, 0), FOVY, W, H)
    assert rg.tobytes() == ctx[0].raygen().tobytes()
    opt, eyev = oracle.bench_options(**optkw), np.asarray(eye, np.float32)
    assert int(opt["use_temporal_resampling"][0]) == 1 and int(opt["use_spatial_resampling"][0]) == 1
    passes = int(opt["spatial_resampling_passes"][0])
    st = oracle.new_state(W, H)
    lights = list(set(sc.lights.tolist()))
    for frame in (1, 2, 3):
        for r in ctx:
            r.raycast()
            r.generate_candidate(frame, api.RT_RES_0)
            r.temporal_resampling(frame, api.RT_RES_TEMPORAL, api.RT_RES_0)
            r.save_temporal_reservoir(api.RT_RES_0, api.RT_RES_TEMPORAL)
        sc.raycast(W, H, rg, st["vis"])
        sc.generate_candidate(W, H, frame, st["vis"], eyev, opt, st["r0"])
        sc.temporal_resampling(W, H, frame, st["vis"], eyev, opt, st["temporal"], st["r0"])
        oracle.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        shaded = (st["vis"]["index"] >= 0) & ~np.isin(st["vis"]["index"], lights)
        assert shaded.mean() > 0.1
        src, dst = api.RT_RES_0, api.RT_RES_1
        osrc, odst = st["r0"], st["r1"]
        for k in range(passes):
            if k:
                src, dst = dst, src
                osrc, odst = odst, osrc
            for r in ctx:
                r.spatial_resampling(frame, k, src, dst)
            sc.spatial_resampling(W, H, frame, k, st["vis"], eyev, opt, osrc, odst)
            got = [r.download(api.RT_BUF_RES_0 + dst) for r in ctx]
            for m, g in zip(MODES[1:], got[1:]):
                assert _eq_bits(got[0], g), f"frame {frame} pass {k}: mode {m} differs from the default in {int((got[0].view(np.uint8).reshape(W * H, -1) != g.view(np.uint8).reshape(W * H, -1)).any(axis=1).sum())} records"
            bad = _res_fields_differ(got[0], odst, shaded)
            assert not bad, f"frame {frame} pass {k}: default against the oracle: {bad}"
        for r in ctx:
            r.resolve(dst)
        sc.resolve(st["accum"], W, H, st["vis"], eyev, opt, odst)
        acc = [r.download(api.RT_BUF_ACCUMULATION) for r in ctx]
        for m, a in zip(MODES[1:], acc[1:]):
            assert _eq_bits(acc[0], a), f"frame {frame}: accumulation of mode {m}"
        assert _eq_bits(acc[0], st["accum"].reshape(acc[0].shape)), f"frame {frame}: accumulation against the oracle"
        hist = [r.download(api.RT_BUF_RES_TEMPORAL) for r in ctx]
        assert _eq_bits(hist[0], hist[1]) and _eq_bits(hist[0], hist[2]), f"frame {frame}: temporal history"
    for r in ctx:
        r.close()


def test_two_strips_equal_the_whole_frame_in_every_mode(api, worlds):
    """the FUSED form of the pass (halo records in the exchange lists): 200 x 120 as two strips over the LOCAL transport, three frames.
    The strip driver wants strips no shorter than their halo, so the radius is 20 here: ceil(20 / 1.96 * 5.6471) = 58 halo rows for
    strips of 60."""
    W, H, bounds, halo = 200, 120, [(0, 60), (60, 120)], 58
    world, optkw = worlds["quad_room"], dict(spatial_resampling_radius=20.0)
    full = _renderer(api, world, W, H, optkw, 1)
    rigs = []
    for m in MODES:
        ctxs = [_renderer(api, world, W, H, optkw, m, rows=b, halo=halo) for b in bounds]
        hub = api.MgHub(len(bounds), renderer=ctxs[0])
        mgs = [api.MultiGpu(c, k, bounds, transport=api.RT_MG_TRANSPORT_LOCAL, hub=hub) for k, c in enumerate(ctxs)]
        rigs.append((m, ctxs, hub, mgs))
    rigs[0][1][0].walk_stats_enable(True)
    for frame in (1, 2, 3):
        full.frame(frame)
        ref = full.download(api.RT_BUF_ACCUMULATION).reshape(H, W, 4)
        hist = full.download(api.RT_BUF_RES_TEMPORAL).reshape(H, W)
        for m, ctxs, hub, mgs in rigs:
            api.mg_frame_lockstep(mgs, frame, False)
            for c, (a, b) in zip(ctxs, bounds):
                rows = slice(a - c.local_row0, b - c.local_row0)
                acc = c.download(api.RT_BUF_ACCUMULATION).reshape(c.local_rows, W, 4)[rows]
                assert _eq_bits(acc, ref[a:b]), f"mode {m} frame {frame} rows {a}:{b}: {int((acc != ref[a:b]).any(axis=2).sum())} pixels differ"
                assert _eq_bits(c.download(api.RT_BUF_RES_TEMPORAL).reshape(c.local_rows, W)[rows], hist[a:b]), f"mode {m} frame {frame} rows {a}:{b}: history"
    st = rigs[0][1][0].neighbour_pick_stats()
    assert st["picks"] > 0 and st["near_ties"] <= 0.02 * st["picks"], st  # the strips' passes ran the pick under test
    for m, ctxs, hub, mgs in rigs:
        for g in mgs:
            g.close()
        hub.close()
        for c in ctxs:
            c.close()
    full.close()


@pytest.mark.parametrize("radius", [30.0, 86.0, 1.0])
def test_the_pick_on_the_device(api, radius):
    """k_math_eval function 45: bit 0 the guard passed, bit 1 it passed with integers that are not the exact ones, bit 2 / 3
    neighbour_pick in mode 1 / 2 differs from neighbour_pick_exact"""
    rng = np.random.default_rng(20260122)
    N = 1 << 23
    pool = np.concatenate([np.arange(512), np.arange(N - 512, N), rng.integers(512, N - 512, 1024)]).astype(np.uint32)  # the 512 smallest and largest draws + seeded ones
    rv0 = np.tile(pool, 32)
    rv1 = np.concatenate([rng.permutation(pool) for _ in range(32)])
    assert len(rv0) == 1 << 16
    to_f = lambda k: (k.astype(np.float64) * 2.0 ** -23).astype(np.float32)  # noqa: E731
    xs = np.array([0, 1, 959, 1919, 3839], np.float32)
    n = len(rv0) * len(xs)
    item = np.empty((n, 5), np.float32)
    item[:, 0] = np.repeat(to_f(rv0), len(xs))
    item[:, 1] = np.repeat(to_f(rv1), len(xs))
    item[:, 2] = np.tile(xs, len(rv0))
    item[:, 3] = rng.choice(np.array([0, 1, 539, 1079, 2159], np.float32), n)
    item[:, 4] = np.float32(radius) / np.float32(1.96)
    r = api.Renderer(64, 48)
    out = r.math_eval(45, item).view(np.uint32)
    r.close()
    assert not (out & 2).any(), f"{int(((out & 2) != 0).sum())} picks cleared by the guard are not the exact ones, e.g. {item[(out & 2) != 0][:3].tolist()}"
    assert not (out & 4).any(), f"neighbour_pick differs from the exact pick in {int(((out & 4) != 0).sum())} items"
    assert not (out & 8).any(), f"neighbour_pick with the guard forced to fail differs from the exact pick in {int(((out & 8) != 0).sum())} items"
    zero = item[:, 0] == 0.0
    assert zero.sum() == 32 * len(xs) and not (out[zero] & 1).any(), "the guard must fail for rv0 = 0"
    # The extreme draws are where real ties live (rv0 -> 1: radius -> 0; rv1 -> 0 or 1: sin -> 0, so the sum sits on the integer yi), so
    # a share of cleared picks means something only for the seeded draws: there a coordinate is a near tie when the sum lies within E
    # plus a unit in the last place of an integer, some 1e-3 of the picks at radius 86 and fewer below; the frame's cap, 2 %, holds.
    seeded = np.repeat((np.tile(np.arange(len(pool)), 32) >= 1024) & (rv1 >= 512) & (rv1 < N - 512), len(xs))
    cleared = (out[seeded] & 1).mean()
    print(f"radius {radius}: the guard cleared {cleared:.5f} of {int(seeded.sum())} seeded picks, {(out[~zero] & 1).mean():.5f} of all with rv0 > 0")
    assert seeded.sum() >= 1 << 16 and cleared >= 0.98, f"the guard cleared only {cleared:.4f} of the seeded picks"


def test_near_ties_stay_under_two_percent(api, worlds):
    """the cap on the fallback: 200 x 120, radius 30 (the default options), three frames of three passes with five neighbours"""
    W, H = 200, 120
    counts = {}
    for m in MODES:
        r = _renderer(api, worlds["quad_room"], W, H, {}, m)
        r.walk_stats_enable(True)
        for frame in (1, 2, 3):
            r.frame(frame)
        counts[m] = r.neighbour_pick_stats()
        r.close()
    print("neighbour picks / near ties per mode:", counts)
    picks = counts[1]["picks"]
    assert picks > 3 * 3 * 0.1 * W * H  # one pick per shaded pixel, pass and neighbour: the pass under test ran
    assert counts[0]["picks"] == picks and counts[2]["picks"] == picks
    assert counts[0]["near_ties"] == 0 and counts[2]["near_ties"] == picks
    assert counts[1]["near_ties"] <= 0.02 * picks, counts[1]
