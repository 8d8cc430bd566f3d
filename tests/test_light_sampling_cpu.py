"""Power-proportional light selection (rt_light_sampling, csrc/light_alias.h) on the CPU: (1) the invariants of
the alias table the library's host code builds, (2) light_select realising exactly the counts the pdf is made from, (3) the
restatement of generate_candidate (tests/light_sampling_ref.py, what the GPU tests compare the kernel with) anchored to the oracle in
uniform mode, and (4) the statistics: power mode has the expectation of uniform mode and less variance.

Setup of (4), as measured when the mode was specified: light_sampling_ref.make_lamp_room() (132 triangles, 82 lights: a 2 x 2 panel
with Ke = 20 and 40 tiles of 0.05 x 0.05 with Ke in [1, 5]), 64 x 48, eye (0.5, 3, 6) -> (0, 1, -1.5), fovy 0.9, default options
(32 candidates, visibility reuse on, temporal and spatial reuse off), 2 336 shaded pixels, frames 0 .. 5 999 (49 s on 6 CPUs),
statistic R + G + B of `accumulation`:
    mean over the shaded pixels, uniform / power:         0.77752 / 0.77750, difference -0.08 SE
    largest per-pixel |z| of the difference:              3.49
    summed per-pixel variance, uniform / power:           2693.68 / 63.94 = ratio 0.0237 (the bound below: its geometric mean with 1)
With 600 frames the per-pixel means of uniform mode are not normal yet (a pixel's estimate is large in the 55 % of frames in which one
of its 32 candidates lands on the panel and near zero otherwise): one pixel then stands 5.8 standard errors off; hence 6 000.
What is left in power mode is the shadow ray's answer (the target function is unshadowed) and the position on the panel; the choice
of the light is what the mode removes."""
import numpy as np
import pytest

import light_sampling_ref as ls

EYE, AT, FOVY = ls.LAMP_EYE, ls.LAMP_AT, np.float32(0.9)
N_FRAMES = 6000
MEASURED_VARIANCE_RATIO = 0.0237  # var_power / var_uniform, this test's own setup, as measured on the CPU (docstring)
ONE = ls.ONE


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _soup():
    """the soup of tests/test_gpu_restir_unbiased.py"""
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


def _weight_sets():
    rng = np.random.default_rng(21)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    sets = {
        "one": [3.0],
        "two, ratio 1e9": [1.0e9, 1.0],
        "two, ratio 1e9, small first": [1.0, 1.0e9],
        "all equal": [0.37] * 13,
        "1000 spanning 2^40": np.float32(2.0) ** rng.uniform(-20.0, 20.0, size=1000).astype(np.float32),
        "zero area among lights": [2.0, 0.0, 5.0, 0.0, 0.0, 1.0, 7.5],
        "non-finite among lights": [2.0, inf, 5.0, nan, 0.0, 1.0e-30, -1.0, 3.0e38],
        "only one selectable": [0.0, nan, 4.0, 0.0],
        "lamp room": ls.lights(ls.make_lamp_room())[1],
        "soup": ls.lights(_soup())[1],
    }
    return {k: np.asarray(v, np.float32) for k, v in sets.items()}


WEIGHTS = _weight_sets()


@pytest.mark.parametrize("name", list(WEIGHTS))
def test_table_invariants(name):
    w = WEIGHTS[name]
    L = len(w)
    t = ls.table(w)
    q, thr, alias, K = (t[k].astype(object) for k in ("q", "thr", "alias", "K"))  # Python integers: exact
    T = t["T"]
    assert t["ok"] and T == sum(q) and T > 0
    # the quantisation: relative to the largest finite weight, at least 1 for every positive finite weight, 0 otherwise
    ok = np.isfinite(w) & (w > 0)
    assert all((q[i] >= 1) == bool(ok[i]) for i in range(L)) and max(q) == 1 << 32
    if name == "lamp room":
        assert L == 82 and 0.995 < float(sum(q[:2])) / T < 0.997, "the panel does not carry the power the docstring says"
    assert all(0 <= x <= ONE for x in thr) and all(0 <= a < L for a in alias)
    # the realised counts, recomputed here from thr and alias
    Kc = [0] * L
    names = [1] * L  # slots that name light i: its own, and those whose alias it is
    for s in range(L):
        Kc[s] += thr[s]
        Kc[alias[s]] += ONE - thr[s]
        if alias[s] != s:
            names[alias[s]] += 1
    assert Kc == list(K)
    assert sum(K) == L * ONE
    assert all((K[i] > 0) == (q[i] > 0) for i in range(L))
    assert all(q[alias[s]] > 0 for s in range(L)), "an alias names a light that must never be selected"
    assert all(thr[s] >= 1 for s in range(L) if q[s] > 0)
    assert all(thr[s] == 0 for s in range(L) if q[s] == 0)
    # |K_i - q_i L 2^23 / T| <= slots that name i, in exact integers: |K_i T - q_i L 2^23| <= names_i T
    worst = max(abs(K[i] * T - q[i] * L * ONE) - names[i] * T for i in range(L))
    assert worst <= 0, f"a realised count is further from its exact share than the header's bound: by {worst / T} counts"


def test_no_selectable_light_is_reported():
    for w in ([0.0], [0.0, np.nan, np.inf, -2.0], []):
        t = ls.table(np.asarray(w, np.float32))
        assert not t["ok"] and t["T"] == 0 and not t["K"].any() and not t["thr"].any()


def test_light_select_realises_the_counts_exhaustively():
    """L = 7: every slot, all 2^23 values PCG::uniformf can give ra"""
    w = np.asarray([5.0, 0.0, 0.3, 40.0, 1.0, 0.002, 9.0], np.float32)
    t = ls.table(w)
    L = len(w)
    total = np.zeros(L, np.uint64)
    for s in range(L):
        slot, counts = ls.select_all(t, (s + 0.5) / L)
        assert slot == s
        want = np.zeros(L, np.uint64)
        want[s] += np.uint64(t["thr"][s])
        want[t["alias"][s]] += np.uint64(ONE - int(t["thr"][s]))
        assert np.array_equal(counts, want), f"slot {s}: {counts} for thr {t['thr'][s]} alias {t['alias'][s]}"
        total += counts
    assert np.array_equal(total, t["K"]) and total[1] == 0 and (total[[0, 2, 3, 4, 5, 6]] > 0).all()
    # the slot draw is the reference's: floor(rv0 L) with the clamp (rv0 < 1 always; the clamp is for a product that rounds up to L)
    assert ls.select(t, 0.0, 0.0) in (0, int(t["alias"][0]))
    big = ls.table(np.ones(3, np.float32))
    assert ls.select(big, np.float32(1.0) - np.float32(2.0) ** -23, 0.0) == 2 and ls.select(big, 1.0, 0.0) == 2


@pytest.fixture(scope="module")
def worlds(oracle):
    from cedec_2024_rt_amd import scenes

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    out = {}
    for name, tris, eye, at in (("room", scenes.make_quad_room(), EYE, AT), ("soup", _soup(), (1.0, 2.0, 9.0), (0.0, 0.0, 0.0)),
                                ("lamp", ls.make_lamp_room(), EYE, AT)):
        out[name] = dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True), eye=eye, at=at)
    return out


def _view(oracle, world, W, H):
    rg = oracle.raygen_lookat(world["eye"], world["at"], (0, 1, 0), FOVY, W, H)
    vis = world["scene"].raycast(W, H, rg)
    lit = (world["tris"]["emissive"] > 0).any(axis=1)
    return vis, (vis["index"] >= 0) & ~lit[np.maximum(vis["index"], 0)]


@pytest.mark.parametrize("name", ["room", "soup"])
@pytest.mark.parametrize("kw", [dict(), dict(use_visibility_reuse=0, ris_sample_count=1), dict(use_shadowed_target_function=1)])
def test_uniform_mode_equals_the_oracle(oracle, worlds, name, kw):
    """the anchor: in uniform mode the restatement IS the oracle's generate_candidate, byte for byte"""
    world, W, H = worlds[name], 64, 48
    vis, shaded = _view(oracle, world, W, H)
    assert shaded.sum() > W * H // 4
    opt = oracle.default_options(**kw)
    for frame in (0, 3):
        want = world["scene"].generate_candidate(W, H, frame, vis, world["eye"], opt)
        got = ls.generate_candidate(W, H, frame, world["tris"], vis, world["eye"], opt, ls.UNIFORM)
        assert np.array_equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).reshape(W * H, 76).any(axis=1).sum())} records differ"
        power = ls.generate_candidate(W, H, frame, world["tris"], vis, world["eye"], opt, ls.POWER)
        assert not np.array_equal(_bits(power[shaded]), _bits(want[shaded])), "the mode changes nothing: the GPU tests would show nothing"
        assert np.array_equal(power["M"], want["M"]) and not _bits(power[~shaded]).any()


def test_power_mode_has_the_expectation_of_uniform_mode_and_less_variance(oracle, worlds):
    world, W, H = worlds["lamp"], 64, 48
    sc = world["scene"]
    vis, shaded = _view(oracle, world, W, H)
    n = int(shaded.sum())
    assert n > W * H // 3
    opt = oracle.default_options()  # temporal and spatial reuse off, accumulate off
    eye = np.asarray(world["eye"], np.float32)
    s1, s2, per_frame = np.zeros((2, n)), np.zeros((2, n)), np.zeros((2, N_FRAMES))
    accum = oracle.new_state(W, H)["accum"]
    for frame in range(N_FRAMES):
        for m, mode in enumerate((ls.UNIFORM, ls.POWER)):
            res = ls.generate_candidate(W, H, frame, world["tris"], vis, eye, opt, mode)
            sc.resolve(accum, W, H, vis, eye, opt, res)
            v = accum.reshape(W * H, 4)[shaded, :3].astype(np.float64).sum(axis=1)
            s1[m] += v
            s2[m] += v * v
            per_frame[m, frame] = v.mean()
    F = N_FRAMES
    mean = s1 / F
    var = (s2 - F * mean * mean) / (F - 1)
    # expectation, whole image: the per-frame image means are independent draws
    d = per_frame[1] - per_frame[0]
    se = np.sqrt(per_frame[0].var(ddof=1) / F + per_frame[1].var(ddof=1) / F)
    z_image = d.mean() / se
    # expectation, per pixel
    pse = np.sqrt((var[0] + var[1]) / F)
    live = pse > 0
    z = np.zeros(n)
    z[live] = (mean[1] - mean[0])[live] / pse[live]
    ratio = var[1].sum() / var[0].sum()
    print(f"shaded {n}; mean uniform {per_frame[0].mean():.5f} power {per_frame[1].mean():.5f} difference {z_image:+.2f} SE; "
          f"max |z| {np.abs(z).max():.2f}; summed variance uniform {var[0].sum():.2f} power {var[1].sum():.2f} ratio {ratio:.4f}")
    assert np.array_equal(mean[0][~live], mean[1][~live]), "pixels without variance in either mode must agree exactly"
    assert abs(z_image) <= 4.0, f"power mode's image mean is {z_image:+.2f} standard errors from uniform mode's"
    assert np.abs(z).max() <= 5.0, f"{int((np.abs(z) > 5).sum())} pixels further than 5 standard errors apart, worst {np.abs(z).max():.2f}"
    r = np.sqrt(1.0 * MEASURED_VARIANCE_RATIO)
    assert var[1].sum() <= var[0].sum() * r, f"summed per-pixel variance {var[1].sum():.3f} against uniform's {var[0].sum():.3f}: ratio {ratio:.4f} > {r:.4f}"
