"""Distance-aware light selection (rt_light_grid, csrc/light_grid.h) on the CPU: (1) exact-integer invariants of
the tables the library's host code builds, (2) the two selection levels realising exactly the counts the pdf is made from, (3) an
independent float64 statement of cell_of, the Morton order, the run cuts and the cell weights, (4) the statistics: the grid has the
expectation of uniform selection and less variance where it should, and (5) the restatement with the grid off is the oracle's.

Setup of (4), as measured when the mode was specified: light_grid_ref.make_lamp_field() (562 triangles, 512 lights of equal power on a
16 x 16 lattice over a 20 x 20 floor with four boxes), 64 x 48, eye (0, 6, 14) -> (0, 0, 0), fovy 0.9, default options (32 candidates,
visibility reuse on, temporal and spatial reuse off), 1 854 shaded pixels, frames 0 .. 299 (uniform's standard error of the image mean
is 0.10 % of it: 0.2 % needs 75), the grid at (16, 64), statistic R + G + B of `accumulation`:
    mean over the shaded pixels, uniform / power / grid:   1.12285 / 1.12470 / 1.12446; grid - uniform = +1.31 SE
    pixels beyond |z| = 4, grid against uniform:           0 (largest 3.61); two uniform runs (frames 0.. and 300..) against each other: 0 (3.47)
    summed per-pixel variance, uniform / power / grid:     1373.4 / 1366.2 / 255.5: grid / uniform = 0.186, grid / power = 0.187
    other settings, grid / uniform:                        (8, 16) 0.415, (16, 256) 0.156, (32, 64) 0.175
The lamps have equal power, so power mode is uniform mode there (0.995); what the grid adds is the distance. On r21's lamp room
(light_sampling_ref.make_lamp_room, one panel with 99.6 % of the power), 600 frames, grid against power: mean +1.47 SE, largest per-pixel
|z| 3.69, summed variance 63.59 / 63.73 = 0.998: the panel is one run, nearly every cell's table gives it nearly all the mass, and the
grid neither gains nor loses against power mode."""
from fractions import Fraction

import numpy as np
import pytest

import light_grid_ref as lg
import light_sampling_ref as ls

ONE = lg.ONE
FOVY = np.float32(0.9)
N_FRAMES = 300
MEASURED_VARIANCE_RATIO = 0.186  # var_grid / var_uniform at (16, 64), this test's own setup, as measured on the CPU (docstring)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _tris(n_plain, n_lights, seed, flat=False):
    """random triangles: n_plain without emission first, then n_lights emissive ones of varied size and emission"""
    from cedec_2024_rt_amd.types import TRIANGLE

    rng = np.random.default_rng(seed)
    n = n_plain + n_lights
    t = np.zeros(n, TRIANGLE)
    c = (rng.random((n, 1, 3)) * 8.0 - 4.0).astype(np.float32)
    size = (10.0 ** rng.uniform(-1.0, 0.3, size=(n, 1, 1))).astype(np.float32)
    t["v"] = (c + (rng.random((n, 3, 3)) - 0.5).astype(np.float32) * size).astype(np.float32)
    if flat:
        t["v"][:, :, 1] = np.float32(1.5)
    t["color"] = 0.7
    t["emissive"][n_plain:] = (rng.random((n_lights, 3)) * 20.0 + 0.01).astype(np.float32)
    return t


def _configs():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    zero_area = _tris(5, 9, 3)
    zero_area["v"][7][2] = zero_area["v"][7][1]  # light 2: two equal vertices
    non_finite = _tris(5, 9, 4)
    non_finite["v"][8][1][0] = inf  # light 3: a vertex at infinity
    non_finite["v"][11][0][2] = nan  # light 6
    non_finite["emissive"][12] = inf  # light 7: finite vertices, no finite weight
    dark_run = _tris(3, 6, 5)
    dark_run["v"][3:5, 2] = dark_run["v"][3:5, 1]  # whatever run they fall into; with B = L every light is a run: two runs with P = 0
    return {
        "L = 1": (_tris(4, 1, 1), 4, 8),
        "L = 7, B = 3": (_tris(6, 7, 2), 2, 3),
        "B > L": (_tris(6, 7, 2), 3, 256),
        "B = 1": (_tris(6, 20, 6), 4, 1),
        "N = 1": (_tris(6, 20, 6), 1, 5),
        "a zero-area light": (zero_area, 3, 4),
        "non-finite lights": (non_finite, 3, 4),
        "runs without power": (dark_run, 2, 256),
        "a flat scene": (_tris(5, 12, 7, flat=True), 4, 5),
        "lamp field": (lg.make_lamp_field(), 16, 64),
        "lamp room at the limits": (ls.make_lamp_room(), 32, 256),
    }


CONFIGS = _configs()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_table_invariants(name):
    tris, N, clusters = CONFIGS[name]
    g = lg.Grid(tris, N, clusters)
    L, B = g.L, g.B
    ids, w = ls.lights(tris)
    assert L == len(ids) and np.array_equal(g.ids, ids) and np.array_equal(_bits(g.w), _bits(w))
    assert B == min(clusters, L) and g.N == N and g.ok
    ok = np.isfinite(w) & (w > 0)
    # every light is in exactly one run; the runs are the cuts floor(r L / B) of the sorted positions, never empty
    assert sorted(g.perm.tolist()) == list(range(L))
    assert g.run_start.tolist() == [r * L // B for r in range(B + 1)] and (np.diff(g.run_start.astype(np.int64)) >= 1).all()
    n_r = np.diff(g.run_start.astype(np.int64))
    run_of_pos = np.repeat(np.arange(B), n_r)
    assert np.array_equal(g.cluster_of[g.perm], run_of_pos)
    # per run: the counts of its lights add up to n_r 2^23 (or to 0 if it has no power), a light without weight has none
    K_light = np.zeros(L, object)
    K_light[g.perm] = g.run_K.astype(object)
    powered = np.zeros(B, bool)
    for r in range(B):
        a, b = int(g.run_start[r]), int(g.run_start[r + 1])
        members = g.perm[a:b]
        powered[r] = ok[members].any()
        assert (g.P[r] > 0) == powered[r]
        assert sum(g.run_K[a:b].astype(object)) == (int(n_r[r]) * ONE if powered[r] else 0)
        assert all(0 <= int(x) < b - a for x in g.run_alias[a:b]) and all(0 <= int(x) <= ONE for x in g.run_thr[a:b])
        # the counts recomputed from the slots
        Kc = [0] * (b - a)
        for s in range(b - a):
            Kc[s] += int(g.run_thr[a + s])
            Kc[int(g.run_alias[a + s])] += (ONE - int(g.run_thr[a + s])) if powered[r] else 0
        assert Kc == [int(x) for x in g.run_K[a:b]]
    assert all((K_light[i] > 0) == bool(ok[i]) for i in range(L)), "a light's count is positive exactly if its weight is positive and finite"
    if name == "runs without power":
        assert (~powered).sum() == 2
    if name == "non-finite lights":
        assert (~ok).sum() == 3
    # per cell: the counts of the runs add up to B 2^23; a run without power has count 0, every other a positive one in EVERY cell; and
    # the total probability, sum_i K_{c, run(i)} / (B 2^23) x K_i / (n_r 2^23), is exactly 1
    cells = N ** 3
    cK = g.cell_K.reshape(cells, B).astype(object)
    cw = g.cell_w.reshape(cells, B)
    assert (cK.sum(axis=1) == B * ONE).all()
    assert ((cK > 0) == powered[None, :]).all() and ((cw > 0) == powered[None, :]).all() and np.isfinite(cw).all()
    check = range(cells) if cells <= 64 else np.random.default_rng(1).choice(cells, 24, replace=False)
    for c in check:
        total = sum(Fraction(int(cK[c, g.cluster_of[i]]), B * ONE) * Fraction(int(K_light[i]), int(n_r[g.cluster_of[i]]) * ONE) for i in range(L))
        assert total == 1, f"cell {c}: the probabilities of the lights add up to {total}"
    thr, alias = g.cell_thr.reshape(cells, B), g.cell_alias.reshape(cells, B)
    assert (alias < B).all() and (thr <= ONE).all()
    assert powered[alias].all(), "an alias names a run that must never be selected"
    # the binary32 factors the kernel multiplies are the counts' quotients
    assert np.array_equal(g.cell_prob, (g.cell_K.astype(np.float64) / (B * float(ONE))).astype(np.float32))
    assert np.array_equal(g.run_prob, (g.run_K.astype(np.float64) / (n_r[run_of_pos] * float(ONE))).astype(np.float32))


def test_no_selectable_light_is_reported():
    tris = _tris(4, 3, 8)
    tris["v"][4:, 2] = tris["v"][4:, 1]
    g = lg.Grid(tris, 2, 2)
    assert g.L == 3 and not g.ok and not g.cell_K.any() and not g.run_K.any()
    g = lg.Grid(_tris(4, 0, 8), 2, 2)
    assert g.L == 0 and g.B == 0 and not g.ok


def test_both_levels_realise_their_counts_exhaustively():
    """L = 7, B' = 3, two cells: light_select_slot over all 2^23 values of ra in every cell slot, and of rb in every run slot. The two
    levels use independent draws, so the product needs no joint enumeration."""
    tris, N, clusters = CONFIGS["L = 7, B = 3"]
    g = lg.Grid(tris, N, clusters)
    assert (g.L, g.B, g.N) == (7, 3, 2)
    for cell in (0, 7):
        total = np.zeros(3, np.uint64)
        for s in range(3):
            counts = g.cell_slot_all(cell, s)
            k = cell * 3 + s
            want = np.zeros(3, np.uint64)
            want[s] += np.uint64(g.cell_thr[k])
            want[g.cell_alias[k]] += np.uint64(ONE - int(g.cell_thr[k]))
            assert np.array_equal(counts, want), f"cell {cell} slot {s}: {counts}"
            total += counts
        assert np.array_equal(total, g.cell_K[cell * 3:cell * 3 + 3])
    for r in range(3):
        a, b = int(g.run_start[r]), int(g.run_start[r + 1])
        total = np.zeros(b - a, np.uint64)
        for t in range(b - a):
            total += g.run_slot_all(r, t)
        assert np.array_equal(total, g.run_K[a:b])
    # one whole selection follows the two tables: slot floor(rv0 B), floor(rc n_r), thresholds against ra and rb
    rng = np.random.default_rng(5)
    for rv0, ra, rc, rb in (rng.integers(0, ONE, size=(200, 4)) / float(ONE)).astype(np.float32):
        for cell in (0, 7):
            light, run, pos, prob = g.select(cell, rv0, ra, rc, rb)
            s = min(int(np.float32(rv0) * np.float32(3)), 2)
            k = cell * 3 + s
            r = s if int(ra * ONE) < g.cell_thr[k] else int(g.cell_alias[k])
            a, n = int(g.run_start[r]), int(g.run_start[r + 1] - g.run_start[r])
            t = min(int(np.float32(rc) * np.float32(n)), n - 1)
            t = t if int(rb * ONE) < g.run_thr[a + t] else int(g.run_alias[a + t])
            assert (run, pos, light) == (r, a + t, int(g.perm[a + t])) and prob == g.cell_prob[cell * 3 + r]


# ---- (3) the float64 statement: numpy only, nothing of the header's

def _finite_box(v):
    """per axis min / max over the finite coordinates of the vertices v (n, 3, 3); [0, 0] without any"""
    lo, hi = np.zeros(3), np.zeros(3)
    for a in range(3):
        x = v[:, :, a].ravel()
        x = x[np.isfinite(x)]
        if len(x):
            lo[a], hi[a] = x.min(), x.max()
    return lo, hi


def _axis_cells(p, lo, hi, N, dtype):
    """(cell, t) per axis in the arithmetic `dtype`"""
    p, lo, hi = p.astype(dtype), lo.astype(dtype), hi.astype(dtype)
    inv = np.where(hi > lo, dtype(N) / np.where(hi > lo, hi - lo, dtype(1)), dtype(1))
    t = (p - lo) * inv
    return np.clip(np.floor(t), 0, N - 1).astype(np.int64), t


def _statement(tris, N, clusters, dtype):
    """runs and cell weights from the triangles, in the arithmetic `dtype` (the weights' last step always in float64)"""
    v = tris["v"].astype(np.float64)
    lit = (tris["emissive"] > 0).any(axis=1)
    lv = v[lit]
    L = len(lv)
    B = min(clusters, L)
    lo, hi = _finite_box(v)
    llo, lhi = _finite_box(lv)
    cen = ((lv[:, 0].astype(dtype) + lv[:, 1].astype(dtype)) + lv[:, 2].astype(dtype)) * (dtype(1) / dtype(3))
    q, tq = _axis_cells(cen, llo, lhi, 1024, dtype)
    code = np.zeros(L, np.int64)
    for bit in range(10):
        for a in range(3):
            code |= ((q[:, a] >> bit) & 1) << (3 * bit + a)
    perm = np.lexsort((np.arange(L), code))
    start = np.array([r * L // B for r in range(B + 1)])
    area = 0.5 * np.linalg.norm(np.cross(lv[:, 1] - lv[:, 0], lv[:, 2] - lv[:, 0]), axis=1)
    lum = tris["emissive"][lit].astype(np.float64) @ np.array([0.1762044, 0.8129847, 0.0108109])
    wl = np.where(np.isfinite(area * lum) & (area * lum > 0), area * lum, 0.0)
    size = np.where(hi > lo, (hi - lo) / N, 1.0).astype(dtype)
    h = dtype(0.5) * np.sqrt((size * size).sum(dtype=dtype))
    P, centre, rho = np.zeros(B), np.zeros((B, 3), dtype), np.zeros(B, dtype)
    for r in range(B):
        m = lv[perm[start[r]:start[r + 1]]]
        P[r] = wl[perm[start[r]:start[r + 1]]].sum()
        rlo, rhi = _finite_box(m)
        centre[r] = dtype(0.5) * (rlo.astype(dtype) + rhi.astype(dtype))
        pts = m.reshape(-1, 3)
        pts = pts[np.isfinite(pts).all(axis=1)].astype(dtype)
        rho[r] = np.sqrt(((pts - centre[r]) ** 2).sum(axis=1, dtype=dtype)).max() if len(pts) else 0
    idx = np.arange(N)
    cz, cy, cx = np.meshgrid(idx, idx, idx, indexing="ij")
    xc = lo.astype(dtype) + (np.stack([cx, cy, cz], axis=-1).reshape(-1, 3).astype(dtype) + dtype(0.5)) * size
    d2 = ((xc[:, None, :].astype(np.float64) - centre[None, :, :].astype(np.float64)) ** 2).sum(axis=2)
    floor = (float(h) + rho.astype(np.float64)) ** 2
    wcell = P[None, :] / np.maximum(d2, floor[None, :])
    return dict(perm=perm, start=start, tq=tq, w=wcell, lo=lo, hi=hi)


@pytest.mark.parametrize("name", ["L = 7, B = 3", "B = 1", "a flat scene", "lamp room at the limits", "soup"])
def test_independent_float64_statement(name):
    if name == "soup":
        rng = np.random.default_rng(15)
        tris, N, clusters = _tris(100, 50, 15), 5, 9
    else:
        tris, N, clusters = CONFIGS[name]
    if name == "lamp room at the limits":
        N = 6  # 32^3 x 82 weights say no more than 6^3 x 82
    g = lg.Grid(tris, N, clusters)
    s64, s32 = _statement(tris, N, clusters, np.float64), _statement(tris, N, clusters, np.float32)
    assert np.array_equal(g.lo, s64["lo"].astype(np.float32)) and np.array_equal(g.hi, s64["hi"].astype(np.float32))
    # cells of random points, inside the bounds and up to half an extent outside: equal except within the float32 against float64
    # spread of a cell face
    rng = np.random.default_rng(9)
    ext = np.where(s64["hi"] > s64["lo"], s64["hi"] - s64["lo"], 1.0)
    p = (s64["lo"] - 0.5 * ext + rng.random((20000, 3)) * 2.0 * ext).astype(np.float32)
    c64, t64 = _axis_cells(p, s64["lo"], s64["hi"], N, np.float64)
    c32, t32 = _axis_cells(p, s64["lo"], s64["hi"], N, np.float32)
    spread = float(np.abs(t32.astype(np.float64) - t64).max())
    assert spread < 1e-4, spread
    near = (np.abs(t64 - np.round(t64)) <= 2.0 * spread).any(axis=1)
    assert near.mean() < 0.01
    want = (c64[:, 2] * N + c64[:, 1]) * N + c64[:, 0]
    got = g.cell_of(p)
    assert np.array_equal(got[~near], want[~near]), f"{int((got[~near] != want[~near]).sum())} points in another cell, away from every face by {2 * spread:.2e} cells"
    # runs: exactly, given that no centroid lies within the spread of a face of the 1024^3 Morton lattice (a property of the scene)
    mspread = float(np.abs(s32["tq"].astype(np.float64) - s64["tq"]).max())
    inside = (s64["tq"] > 0) & (s64["tq"] < 1024)  # a coordinate at the box's own face clamps, in either arithmetic
    assert not ((np.abs(s64["tq"] - np.round(s64["tq"])) <= 2.0 * mspread) & inside & (np.round(s64["tq"]) > 0) & (np.round(s64["tq"]) < 1024)).any(), \
        "the scene has a centroid on a face of the Morton lattice: choose another"
    assert np.array_equal(g.perm, s64["perm"]) and np.array_equal(g.run_start, s64["start"])
    # weights: within 8 x the statement's own float32 against float64 spread
    live = s64["w"] > 0
    assert np.array_equal(live.ravel(), g.cell_w > 0)
    wspread = float((np.abs(s32["w"] - s64["w"])[live] / s64["w"][live]).max())
    err = float((np.abs(g.cell_w.reshape(s64["w"].shape).astype(np.float64) - s64["w"])[live] / s64["w"][live]).max())
    print(f"{name}: cell spread {spread:.2e}, Morton spread {mspread:.2e}, weight spread {wspread:.2e}, header against float64 {err:.2e}")
    assert 0 < wspread < 1e-4 and err <= 8.0 * wspread, f"cell weights {err:.3e} from the float64 statement, its own spread {wspread:.3e}"


# ---- (4) and (5)

@pytest.fixture(scope="module")
def worlds(oracle):
    from cedec_2024_rt_amd import scenes

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    out = {}
    for name, tris, eye, at in (("room", scenes.make_quad_room(), ls.LAMP_EYE, ls.LAMP_AT), ("lamp", ls.make_lamp_room(), ls.LAMP_EYE, ls.LAMP_AT),
                                ("field", lg.make_lamp_field(), lg.FIELD_EYE, lg.FIELD_AT)):
        out[name] = dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True), eye=eye, at=at)
    return out


def _view(oracle, world, W, H):
    rg = oracle.raygen_lookat(world["eye"], world["at"], (0, 1, 0), FOVY, W, H)
    vis = world["scene"].raycast(W, H, rg)
    lit = (world["tris"]["emissive"] > 0).any(axis=1)
    return vis, (vis["index"] >= 0) & ~lit[np.maximum(vis["index"], 0)]


def test_grid_off_equals_the_oracle_and_on_changes_the_records(oracle, worlds):
    """the anchor (tests/test_light_sampling_cpu.py's, once from here): with the grid off the restatement IS the oracle's
    generate_candidate, byte for byte; with it on the records differ and nothing else does"""
    world, W, H = worlds["room"], 64, 48
    vis, shaded = _view(oracle, world, W, H)
    assert shaded.sum() > W * H // 4
    opt = oracle.default_options()
    grid = lg.Grid(world["tris"], 4, 8)
    want = world["scene"].generate_candidate(W, H, 3, vis, world["eye"], opt)
    got = lg.generate_candidate(W, H, 3, world["tris"], vis, world["eye"], opt, lg.UNIFORM)
    assert np.array_equal(_bits(got), _bits(want))
    on = lg.generate_candidate(W, H, 3, world["tris"], vis, world["eye"], opt, lg.GRID, grid=grid)
    assert not np.array_equal(_bits(on[shaded]), _bits(want[shaded])), "the grid changes nothing: the GPU tests would show nothing"
    assert np.array_equal(on["M"], want["M"]) and not _bits(on[~shaded]).any()


def _moments(oracle, world, W, H, vis, shaded, runs, n_frames):
    """per run (mode, first frame, grid): per-pixel mean and variance of R + G + B over n_frames independent frames, and the image means"""
    sc, n = world["scene"], int(shaded.sum())
    opt = oracle.default_options()  # temporal and spatial reuse off, accumulate off
    eye = np.asarray(world["eye"], np.float32)
    R = len(runs)
    s1, s2, per_frame = np.zeros((R, n)), np.zeros((R, n)), np.zeros((R, n_frames))
    accum = oracle.new_state(W, H)["accum"]
    for frame in range(n_frames):
        for m, (mode, first, grid) in enumerate(runs):
            res = lg.generate_candidate(W, H, first + frame, world["tris"], vis, eye, opt, mode, grid=grid)
            sc.resolve(accum, W, H, vis, eye, opt, res)
            v = accum.reshape(W * H, 4)[shaded, :3].astype(np.float64).sum(axis=1)
            s1[m] += v
            s2[m] += v * v
            per_frame[m, frame] = v.mean()
    mean = s1 / n_frames
    return mean, (s2 - n_frames * mean * mean) / (n_frames - 1), per_frame


def _compare(mean, var, per_frame, a, b, F):
    """(z of the image means' difference, per-pixel z) of run b against run a"""
    se = np.sqrt(per_frame[a].var(ddof=1) / F + per_frame[b].var(ddof=1) / F)
    z_image = (per_frame[b].mean() - per_frame[a].mean()) / se
    pse = np.sqrt((var[a] + var[b]) / F)
    live = pse > 0
    z = np.zeros(len(pse))
    z[live] = (mean[b] - mean[a])[live] / pse[live]
    assert np.array_equal(mean[a][~live], mean[b][~live]), "pixels without variance in either run must agree exactly"
    return z_image, z


def test_the_grid_has_the_expectation_of_uniform_selection_and_less_variance(oracle, worlds):
    world, W, H, F = worlds["field"], 64, 48, N_FRAMES
    vis, shaded = _view(oracle, world, W, H)
    assert shaded.sum() > W * H // 2
    grid = lg.Grid(world["tris"], 16, 64)
    assert (grid.L, grid.B) == (512, 64)
    runs = [(lg.UNIFORM, 0, None), (lg.UNIFORM, F, None), (lg.POWER, 0, None), (lg.GRID, 0, grid)]
    mean, var, pf = _moments(oracle, world, W, H, vis, shaded, runs, F)
    se_uniform = np.sqrt(pf[0].var(ddof=1) / F) / pf[0].mean()
    z_self, zp_self = _compare(mean, var, pf, 0, 1, F)
    z_grid, zp_grid = _compare(mean, var, pf, 0, 3, F)
    ratio_u, ratio_p = var[3].sum() / var[0].sum(), var[3].sum() / var[2].sum()
    print(f"shaded {int(shaded.sum())}; uniform's standard error of the mean {100 * se_uniform:.3f} %; means uniform {pf[0].mean():.5f} "
          f"power {pf[2].mean():.5f} grid {pf[3].mean():.5f}; grid - uniform {z_grid:+.2f} SE, {int((np.abs(zp_grid) > 4).sum())} pixels beyond 4 "
          f"(largest {np.abs(zp_grid).max():.2f}); uniform against uniform {z_self:+.2f} SE, {int((np.abs(zp_self) > 4).sum())} beyond 4 "
          f"(largest {np.abs(zp_self).max():.2f}); summed variance uniform {var[0].sum():.1f} power {var[2].sum():.1f} grid {var[3].sum():.1f}: "
          f"grid / uniform {ratio_u:.4f}, grid / power {ratio_p:.4f}")
    assert se_uniform < 0.002, "too few frames: the uniform run's standard error of the mean is not below 0.2 %"
    assert abs(z_self) <= 4.0 and (np.abs(zp_self) > 4.0).sum() <= 6, "two uniform runs against each other leave the bound: the bound is wrong for this setup"
    assert abs(z_grid) <= 4.0, f"the grid's image mean is {z_grid:+.2f} standard errors from uniform selection's"
    assert (np.abs(zp_grid) > 4.0).sum() <= 6, f"{int((np.abs(zp_grid) > 4).sum())} pixels further than 4 standard errors apart, worst {np.abs(zp_grid).max():.2f}"
    r = np.sqrt(1.0 * MEASURED_VARIANCE_RATIO)
    assert ratio_u <= r, f"summed per-pixel variance {var[3].sum():.3f} against uniform's {var[0].sum():.3f}: ratio {ratio_u:.4f} > {r:.4f}"


def test_the_grid_has_the_expectation_of_power_mode_on_the_lamp_room(oracle, worlds):
    """r21's scene, one panel with nearly all the power: the variance ratio is reported (docstring: 0.998), the mean is asserted"""
    world, W, H, F = worlds["lamp"], 64, 48, 600
    vis, shaded = _view(oracle, world, W, H)
    grid = lg.Grid(world["tris"], 16, 64)
    mean, var, pf = _moments(oracle, world, W, H, vis, shaded, [(lg.POWER, 0, None), (lg.GRID, 0, grid)], F)
    z_image, z = _compare(mean, var, pf, 0, 1, F)
    print(f"lamp room: means power {pf[0].mean():.5f} grid {pf[1].mean():.5f}, {z_image:+.2f} SE; {int((np.abs(z) > 4).sum())} pixels beyond 4 "
          f"(largest {np.abs(z).max():.2f}); summed variance grid / power {var[1].sum() / var[0].sum():.4f}")
    assert abs(z_image) <= 4.0 and (np.abs(z) > 4.0).sum() <= 6
