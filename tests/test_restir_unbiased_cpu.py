"""The unbiased spatial pass (rt_spatial_unbiased) on the CPU: tests/restir_unbiased_ref.py, the restatement the
GPU tests compare the kernel with, is (1) anchored to the oracle through its "reference" switch, (2) equal to the reference's
normalisation where every contributor has the same support, (3) unbiased where the reference's pass is not, and (4) shown to let
the shadow rays decide on the quad room and the geometry term on a scene with a light in a shaded surface's plane.

Setup of (3), as measured when the mode was specified: scenes.make_quad_room() (92 triangles), 64 x 48, eye (0.5, 3, 6) ->
(0, 1, -1.5), fovy 0.9, default options (32 candidates, visibility reuse on, temporal off, 5 neighbours, radius 30, 3 passes),
2 329 shaded pixels. Statistic: mean of R + G + B of `accumulation` over the shaded pixels, 2 000 independent frames (accumulate = 0,
the sequences' frames numbered apart). Truth: the oracle with spatial reuse off, plain RIS, unbiased by construction.
    truth, two halves against each other:                 0.20324,                     0 / 0 pixels with z < -4 / z > 4
    oracle, spatial reuse on:                             0.19851 = -2.33 % = -36.6 SE, 66 / 0
    float64 prototype of the unbiased pass:               0.203277 = +0.02 % = +0.3 SE,  1 / 0 (max |z| 4.2)
"""
import numpy as np
import pytest

import restir_unbiased_ref as ru

EYE, AT, FOVY = (0.5, 3.0, 6.0), (0.0, 1.0, -1.5), np.float32(0.9)
N_FRAMES = 2000


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def room(oracle):
    from cedec_2024_rt_amd import scenes

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    tris = scenes.make_quad_room()
    return dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True))


def _view(oracle, world, W, H, eye=EYE, at=AT, fovy=FOVY):
    rg = oracle.raygen_lookat(eye, at, (0, 1, 0), fovy, W, H)
    vis = world["scene"].raycast(W, H, rg)
    e = world["tris"]["emissive"]
    lit = (e > 0).any(axis=1)
    shaded = (vis["index"] >= 0) & ~lit[np.maximum(vis["index"], 0)]
    return vis, shaded


@pytest.mark.parametrize("W,H", [(64, 48), (37, 29)])
def test_reference_switch_equals_the_oracle(oracle, room, W, H):
    """with the switch on "reference" the restatement IS the oracle's spatial_resampling, byte for byte, passes 0-2 chained"""
    vis, shaded = _view(oracle, room, W, H)
    assert shaded.sum() > W * H // 3
    opt = oracle.default_options(use_spatial_resampling=1)
    cur = room["scene"].generate_candidate(W, H, 3, vis, EYE, opt)
    for pas in range(3):
        want = room["scene"].spatial_resampling(W, H, 3, pas, vis, EYE, opt, cur)
        got, diag = ru.spatial(W, H, 3, pas, room["tris"], vis, EYE, opt, cur, mode=ru.REFERENCE)
        assert np.array_equal(_bits(got), _bits(want)), f"pass {pas}: {int((_bits(got) != _bits(want)).reshape(W * H, 76).any(axis=1).sum())} records differ"
        assert np.array_equal(diag[:, 0], diag[:, 1]) and not diag[:, 2:].any()
        assert (got["M"][shaded] > cur["M"][shaded]).any(), "no neighbour was merged: the comparison would show nothing"
        cur = want


def test_equal_supports_give_the_reference_normalisation(oracle):
    """a floor, one light above it, nothing else: every contributor could have produced every sample, so Z = M_sum everywhere and
    the unbiased ucw is w_sum / (M_sum p-hat) bit for bit"""
    t = np.zeros(4, dtype=oracle.TRIANGLE)
    floor = np.array([(-6, 0, -6), (6, 0, -6), (6, 0, 6), (-6, 0, 6)], np.float32)
    lamp = np.array([(-0.5, 4, -0.5), (0.5, 4, -0.5), (0.5, 4, 0.5), (-0.5, 4, 0.5)], np.float32)
    for i, (q, col, ke) in enumerate(((floor, 0.7, 0.0), (lamp, 0.0, 10.0))):
        t["v"][2 * i], t["v"][2 * i + 1] = q[[0, 1, 2]], q[[0, 2, 3]]
        t["color"][2 * i:2 * i + 2], t["emissive"][2 * i:2 * i + 2] = col, ke
    world = dict(tris=t, scene=oracle.Scene(t, use_bvh=True))
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    W, H, eye = 40, 30, (0.0, 3.0, 7.0)
    vis, shaded = _view(oracle, world, W, H, eye=eye, at=(0.0, 0.0, 0.0), fovy=np.float32(0.8))
    assert shaded.sum() > W * H // 3
    opt = oracle.default_options(use_spatial_resampling=1)
    cur = world["scene"].generate_candidate(W, H, 1, vis, eye, opt)
    assert cur["visibility"][shaded].all()
    for pas in range(3):
        out, diag = ru.spatial(W, H, 1, pas, t, vis, eye, opt, cur)
        assert np.array_equal(diag[shaded, 0], diag[shaded, 1]) and not diag[:, 2:].any()
        assert np.array_equal(diag[shaded, 1], out["M"][shaded]) and (out["M"][shaded] > cur["M"][shaded]).any()
        assert out["visibility"][shaded].all()
        # p-hat of the output sample at the pixel, from the oracle's own functions
        surf = np.zeros((W * H, 6), np.float32)
        idx = np.nonzero(shaded)[0]
        tv = t["v"][vis["index"][idx]]
        u, v = vis["uv"][idx, 0:1], vis["uv"][idx, 1:2]
        surf[idx, :3] = (np.float32(1) - u - v) * tv[:, 0] + u * tv[:, 1] + v * tv[:, 2]
        surf[idx, 3:] = (0.0, 1.0, 0.0)  # the floor, seen from above
        G = oracle.fn_bulk("geometry_term", np.concatenate([surf[idx], out["hit_position"][idx], out["hit_normal"][idx]], axis=1))[:, 0]
        lum = oracle.fn_bulk("luminance", out["radiance"][idx])[:, 0]
        p_hat = (np.float32(1) / np.float32(np.pi)) * G * lum
        assert (p_hat > 0).all()
        want = out["w_sum"][idx] / (out["M"][idx].astype(np.float32) * p_hat)
        assert np.array_equal(want.view(np.uint32), out["ucw"][idx].view(np.uint32))
        cur = out


class _Seq:
    """per-frame statistic and per-pixel moments of one sequence of independent frames"""

    def __init__(self, n_px):
        self.stat, self.s1, self.s2 = [], np.zeros(n_px), np.zeros(n_px)

    def add(self, rgb_sum):
        v = rgb_sum.astype(np.float64)
        self.stat.append(v.mean())
        self.s1 += v
        self.s2 += v * v

    def done(self):
        n = len(self.stat)
        self.stat = np.array(self.stat)
        self.mean, self.var = self.s1 / n, np.maximum(self.s2 / n - (self.s1 / n) ** 2, 0.0) * n / (n - 1)
        self.n = n
        return self


def _compare(a, truth):
    """(difference of the statistic in SE of that difference, per-pixel z)"""
    se = np.sqrt(a.stat.var(ddof=1) / a.n + truth.stat.var(ddof=1) / truth.n)
    d = (a.stat.mean() - truth.stat.mean()) / se
    den = np.sqrt(a.var / a.n + truth.var / truth.n)
    z = np.where(den > 0, (a.mean - truth.mean) / np.where(den > 0, den, 1.0), 0.0)
    return d, z


def test_unbiased_where_the_reference_pass_is_not(oracle, room):
    W, H = 64, 48
    vis, shaded = _view(oracle, room, W, H)
    assert int(shaded.sum()) == 2329
    sc, tris = room["scene"], room["tris"]
    plain = oracle.default_options()
    reuse = oracle.default_options(use_spatial_resampling=1)
    acc = np.zeros((W * H, 4), np.float32)

    def shade(res):
        sc.resolve(acc, W, H, vis, EYE, plain, res)
        return acc[shaded, :3].sum(axis=1)

    truth, biased, unbiased = _Seq(int(shaded.sum())), _Seq(int(shaded.sum())), _Seq(int(shaded.sum()))
    for f in range(N_FRAMES):
        truth.add(shade(sc.generate_candidate(W, H, 1 + f, vis, EYE, plain)))
        a = sc.generate_candidate(W, H, 100001 + f, vis, EYE, reuse)
        b = sc.generate_candidate(W, H, 200001 + f, vis, EYE, reuse)
        for pas in range(3):
            a = sc.spatial_resampling(W, H, 100001 + f, pas, vis, EYE, reuse, a)
            b, _ = ru.spatial(W, H, 200001 + f, pas, tris, vis, EYE, reuse, b)
        biased.add(shade(a))
        unbiased.add(shade(b))
    truth.done(), biased.done(), unbiased.done()
    d_b, z_b = _compare(biased, truth)
    d_u, z_u = _compare(unbiased, truth)
    print(f"truth {truth.stat.mean():.6f}  biased {biased.stat.mean():.6f} ({d_b:+.1f} SE, {int((z_b < -4).sum())} / {int((z_b > 4).sum())} pixels beyond 4)  "
          f"unbiased {unbiased.stat.mean():.6f} ({d_u:+.1f} SE, {int((z_u < -4).sum())} / {int((z_u > 4).sum())}, max |z| {np.abs(z_u).max():.2f})")
    # the test can fail: the reference's pass does (measured -36.6 SE and 66 pixels)
    assert d_b <= -10.0 and int((z_b < -4).sum()) >= 30
    assert abs(d_u) <= 4.0
    assert int((np.abs(z_u) > 4).sum()) <= 6


def _decided(oracle, world, W, H, eye, at):
    """pixels with Z < M_sum by geometry alone / by the ray alone: frame 3, the three passes summed"""
    vis, shaded = _view(oracle, world, W, H, eye=eye, at=at)
    opt = oracle.default_options(use_spatial_resampling=1)
    cur = world["scene"].generate_candidate(W, H, 3, vis, eye, opt)
    by_geometry = by_ray = 0
    for pas in range(3):
        cur, diag = ru.spatial(W, H, 3, pas, world["tris"], vis, eye, opt, cur)
        assert (diag[:, 0] <= diag[:, 1]).all() and not diag[~shaded].any()
        less = diag[:, 0] < diag[:, 1]
        assert np.array_equal(less, (diag[:, 2] | diag[:, 3]) != 0)
        by_geometry += int(((diag[:, 2] != 0) & (diag[:, 3] == 0)).sum())
        by_ray += int(((diag[:, 3] != 0) & (diag[:, 2] == 0)).sum())
    print("pixels with Z < M_sum by geometry alone / by the ray alone:", by_geometry, by_ray)
    return by_geometry, by_ray


def test_geometry_and_rays_decide(oracle, room):
    """Z < M_sum happens, and the counters say through which indicator. First run of this test on the quad room: 347 pixels where a
    shadow ray alone kept a neighbour with Mk > 0 out of Z, 0 where the geometry term alone did: the reference's geometry term takes
    |cos| at both ends (common/core.hpp:287-295), so it is zero only for a sample that lies exactly in the neighbour's plane, and in
    this room no light does. test_geometry_decides has such a light. Asserted: 300 of the 347."""
    by_geometry, by_ray = _decided(oracle, room, 64, 48, EYE, AT)
    assert by_ray >= 300


def test_geometry_decides(oracle):
    """ru.make_ledge(): a lamp in the floor's plane next to a ramp. Ramp pixels select it, their floor neighbours have G = 0 exactly
    and stay out of Z without a ray. First run of this test: 89 pixels by geometry alone (and none by the ray alone: nothing stands
    between the floor and the lamps); asserted: 75 of the 89."""
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    tris = ru.make_ledge(oracle.TRIANGLE)
    world = dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True))
    by_geometry, by_ray = _decided(oracle, world, 64, 48, ru.LEDGE_EYE, ru.LEDGE_AT)
    assert by_geometry >= 75
