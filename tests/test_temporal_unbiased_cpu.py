"""rt_temporal_unbiased without a GPU: the restatement of tests/temporal_unbiased_ref.py (compiled from csrc/temporal_unbiased.h and the
other headers of the kernels) (1) anchored to tests/temporal_reproject_ref.py with the switch off, (2) equal to the reprojected
reference merge where the history's pixel and the merging pixel have the same support, (3) unbiased under an orbiting camera where
the reference's merge is not, (4) chained with rt_spatial_unbiased, and (5) the gather's edge cases.

Setup of (3) and (4), as measured when the mode was specified: scenes.make_quad_room() at 64 x 48, last camera eye (0.5, 3, 6) ->
(0, 1, -1.5), fovy 0.9 (2 329 shaded pixels), default options + use_temporal_resampling (32 candidates, visibility reuse on), an
orbit of 4 steps of 0.15 rad about the target that ends at that camera, merged every frame; statistic: mean of R + G + B of the
resolved last frame over the shaded pixels; truth: plain candidates at the last camera; control: a second, independent truth."""
import numpy as np
import pytest

import restir_unbiased_ref as ru
import temporal_reproject_ref as tr
import temporal_unbiased_ref as tu

EYE, AT, FOVY = (0.5, 3.0, 6.0), (0.0, 1.0, -1.5), np.float32(0.9)
STEP, STEPS = 0.15, 4
N_TRIALS = 6000        # (3): the issue's count
N_TRIALS_CHAIN = 2000  # (4): the count of rt_spatial_unbiased's own study (tests/test_restir_unbiased_cpu.py)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _orbit(eye, at, angle):
    e, a = _f32(eye).astype(np.float64), _f32(at).astype(np.float64)
    c, s = np.cos(angle), np.sin(angle)
    d = e - a
    return _f32(a + np.array([c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]])), _f32(at)


class View:
    """a camera over a world: RayGenerator, eye, the oracle's Visibility buffer and its shaded pixels"""

    def __init__(self, oracle, world, W, H, eye, at, fovy=FOVY):
        self.W, self.H, self.eye, self.at = W, H, _f32(eye), _f32(at)
        self.rg = oracle.raygen_lookat(self.eye, self.at, (0, 1, 0), fovy, W, H)
        self.vis = world["scene"].raycast(W, H, self.rg)
        lit = (world["tris"]["emissive"] > 0).any(axis=1)
        self.shaded = (self.vis["index"] >= 0) & ~lit[np.maximum(self.vis["index"], 0)]


@pytest.fixture(scope="module")
def room(oracle):
    from cedec_2024_rt_amd import scenes

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    tris = scenes.make_quad_room()
    return dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True))


def _history(oracle, world, view, opt, frames=2, first=1):
    """a temporal history written under `view`: `frames` frames of candidates + the reference's temporal merge"""
    sc, W, H = world["scene"], view.W, view.H
    hist = np.zeros(W * H, dtype=oracle.RESERVOIR)
    for f in range(first, first + frames):
        res = sc.generate_candidate(W, H, f, view.vis, view.eye, opt)
        sc.temporal_resampling(W, H, f, view.vis, view.eye, opt, hist, res)
        hist = res
    return hist


# ------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("W,H", [(64, 48), (37, 29)])
@pytest.mark.parametrize("vis_reuse", [1, 0])
def test_switch_off_is_temporal_reproject_ref(oracle, room, W, H, vis_reuse):
    """modes REFERENCE and REPROJECT equal tests/temporal_reproject_ref.py byte for byte, under a moved and under a standing camera;
    UNBIASED under a standing camera is the reference's merge too (the host launches the same kernels)"""
    opt = oracle.default_options(use_temporal_resampling=1, use_visibility_reuse=vis_reuse)
    cur = View(oracle, room, W, H, EYE, AT)
    prev = View(oracle, room, W, H, *_orbit(EYE, AT, -STEP))
    assert cur.shaded.sum() > W * H // 3
    for pv in (prev, cur):
        hist = _history(oracle, room, pv, opt)
        cand = room["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
        for mode, tr_mode in ((tu.REFERENCE, tr.REFERENCE), (tu.REPROJECT, tr.REPROJECT)):
            want, wd = tr.temporal(W, H, 7, room["tris"], cur.vis, pv.vis, cur.eye, pv.rg, cur.rg, opt, hist, cand.copy(), mode=tr_mode)
            got, gd = tu.temporal(W, H, 7, room["tris"], cur.vis, pv.vis, cur.eye, pv.rg, cur.rg, opt, hist, cand.copy(), mode=mode)
            assert np.array_equal(_bits(got), _bits(want)), (mode, int((_bits(got) != _bits(want)).reshape(W * H, 76).any(axis=1).sum()))
            if tr_mode == tr.REPROJECT and pv is prev:
                assert np.array_equal(gd[:, 0], wd[:, 0])
            assert (got["M"][cur.shaded] > cand["M"][cur.shaded]).any(), "no history was merged: the comparison would show nothing"
        if pv is cur:
            got, _ = tu.temporal(W, H, 7, room["tris"], cur.vis, pv.vis, cur.eye, pv.rg, cur.rg, opt, hist, cand.copy(), mode=tu.UNBIASED)
            assert np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------------------------- 2
def test_equal_supports_give_the_reprojected_reference_merge(oracle):
    """a floor, one lamp above it, nothing else: the history's pixel could have produced every sample, so Z = M_sum everywhere and the
    record is the reprojected reference merge's in every field but the origin, which is the pixel's own surface"""
    t = np.zeros(4, dtype=oracle.TRIANGLE)
    floor = np.array([(-6, 0, -6), (6, 0, -6), (6, 0, 6), (-6, 0, 6)], np.float32)
    lamp = np.array([(-0.5, 4, -0.5), (0.5, 4, -0.5), (0.5, 4, 0.5), (-0.5, 4, 0.5)], np.float32)
    for i, (q, col, ke) in enumerate(((floor, 0.7, 0.0), (lamp, 0.0, 10.0))):
        t["v"][2 * i], t["v"][2 * i + 1] = q[[0, 1, 2]], q[[0, 2, 3]]
        t["color"][2 * i:2 * i + 2], t["emissive"][2 * i:2 * i + 2] = col, ke
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    world = dict(tris=t, scene=oracle.Scene(t, use_bvh=True))
    W, H, eye, at = 40, 30, (0.0, 3.0, 7.0), (0.0, 0.0, 0.0)
    cur = View(oracle, world, W, H, eye, at, np.float32(0.8))
    prev = View(oracle, world, W, H, *_orbit(eye, at, -STEP), np.float32(0.8))
    sh = cur.shaded
    assert sh.sum() > W * H // 3
    opt = oracle.default_options(use_temporal_resampling=1)
    hist = _history(oracle, world, prev, opt)
    cand = world["scene"].generate_candidate(W, H, 5, cur.vis, cur.eye, opt)
    want, _ = tr.temporal(W, H, 5, t, cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, cand.copy(), mode=tr.REPROJECT)
    got, diag = tu.temporal(W, H, 5, t, cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, cand.copy(), mode=tu.UNBIASED)
    assert (diag[sh, 0] == 1).sum() > sh.sum() // 2 and (diag[sh, 1] == 1).any() and (diag[sh, 4] > 0).any()
    assert np.array_equal(diag[sh, 5], got["M"][sh]), "Z = M_sum at every shaded pixel"
    assert np.array_equal(diag[sh, 2] == 1, diag[sh, 4] > 0)
    for f in got.dtype.names:
        if f in ("origin_position", "origin_normal", "pad"):
            continue
        assert np.array_equal(_bits(got[f]), _bits(want[f])), f
    assert np.array_equal(_bits(got["origin_position"][sh]), _bits(cand["origin_position"][sh]))
    assert np.array_equal(_bits(got["origin_normal"][sh]), _bits(cand["origin_normal"][sh]))
    pts, shaded = tr.surface_points(t, cur.vis, cur.eye)
    assert np.array_equal(shaded, sh) and np.array_equal(_bits(got["origin_position"][sh]), _bits(pts[sh]))
    assert np.array_equal(_bits(got[~sh]), _bits(cand[~sh]))


# ------------------------------------------------------------------------------------------------------------- 3 and 4
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


def _study(oracle, room, n_trials, spatial, first=0):
    """the orbit merged every frame by the reference's merge with a reprojected history (frames 100 000 + 10 f + k) and by the 1/Z
    merge (500 000 + ...), beside the truth (1 + f) and the control (900 001 + f). spatial: the last frame also runs the three spatial
    passes on the merged records (the history is what stage 0 wrote, as the reference saves it before the passes): the oracle's
    for the reference chain, rt_spatial_unbiased's restatement for the other."""
    W, H = 64, 48
    views = [View(oracle, room, W, H, *_orbit(EYE, AT, -STEP * (STEPS - k))) for k in range(STEPS + 1)]
    cur = views[-1]
    assert int(cur.shaded.sum()) == 2329
    sc, tris = room["scene"], room["tris"]
    plain = oracle.default_options()
    topt = oracle.default_options(use_temporal_resampling=1)
    sopt = oracle.default_options(use_temporal_resampling=1, use_spatial_resampling=1)
    acc = np.zeros((W * H, 4), np.float32)

    def shade(res):
        sc.resolve(acc, W, H, cur.vis, cur.eye, plain, res)
        return acc[cur.shaded, :3].sum(axis=1)

    n = int(cur.shaded.sum())
    truth, control, biased, unbiased = _Seq(n), _Seq(n), _Seq(n), _Seq(n)
    excluded = 0
    for f in range(first, first + n_trials):  # first > 0: trials that share no frame number with the committed runs (the log's reruns)
        truth.add(shade(sc.generate_candidate(W, H, 1 + f, cur.vis, cur.eye, plain)))
        control.add(shade(sc.generate_candidate(W, H, 900001 + f, cur.vis, cur.eye, plain)))
        for mode, seq, base in ((tu.REPROJECT, biased, 100000), (tu.UNBIASED, unbiased, 500000)):
            v0 = views[0]
            hist = sc.generate_candidate(W, H, base + 10 * f, v0.vis, v0.eye, topt)
            for k in range(1, STEPS + 1):
                v, frame = views[k], base + 10 * f + k
                res = sc.generate_candidate(W, H, frame, v.vis, v.eye, topt)
                res, diag = tu.temporal(W, H, frame, tris, v.vis, views[k - 1].vis, v.eye, views[k - 1].rg, v.rg, topt, hist, res, mode=mode)
                hist = res
            if mode == tu.UNBIASED:
                excluded += int(((diag[:, 4] > 0) & (diag[:, 2] == 0)).sum())
            if spatial:
                frame = base + 10 * f + STEPS
                for pas in range(3):
                    if mode == tu.REPROJECT:
                        res = sc.spatial_resampling(W, H, frame, pas, cur.vis, cur.eye, sopt, res)
                    else:
                        res, _ = ru.spatial(W, H, frame, pas, tris, cur.vis, cur.eye, sopt, res)
            seq.add(shade(res))
    for s in (truth, control, biased, unbiased):
        s.done()
    out = dict(excluded=excluded / n_trials, truth=truth.stat.mean())
    for name, s in (("control", control), ("biased", biased), ("unbiased", unbiased)):
        d, z = _compare(s, truth)
        out[name] = dict(d=d, low=int((z < -4).sum()), beyond=int((np.abs(z) > 4).sum()), zmax=float(np.abs(z).max()), mean=s.stat.mean())
        print(f"{name}: {s.stat.mean():.6f} against {truth.stat.mean():.6f} ({(s.stat.mean() / truth.stat.mean() - 1) * 100:+.2f} %), {d:+.1f} SE, "
              f"{out[name]['low']} pixels with z < -4, {out[name]['beyond']} with |z| > 4, max |z| {out[name]['zmax']:.2f}")
    print(f"history kept out of Z in the last merge: {out['excluded']:.1f} pixels per frame")
    return out


def test_unbiased_where_the_reference_merge_is_not(oracle, room):
    """Measured by this test as committed (6 000 trials; docs/MEASUREMENT_LOG_r31.md):
        control:                                 0.203224 against the truth's 0.203241, -0.3 SE, 0 pixels with |z| > 4 (max |z| 3.75)
        reference merge, reprojected history:    0.202194 = -0.52 %, -21.3 SE, 35 pixels with z < -4 (max |z| 14.11)
        1/Z merge:                               0.203232 = -0.00 %, -0.2 SE, 0 pixels with |z| > 4 (max |z| 3.88)
        history kept out of Z in the last merge: 97.8 pixels per frame"""
    m = _study(oracle, room, N_TRIALS, spatial=False)
    assert abs(m["control"]["d"]) <= 4.0, "the truth disagrees with itself: the run says nothing"
    # the test can fail: the reference's merge does
    assert m["biased"]["d"] <= -10.0 and m["biased"]["low"] >= 15
    assert abs(m["unbiased"]["d"]) <= 4.0
    assert m["unbiased"]["beyond"] <= 6
    assert m["excluded"] >= 50.0


def test_chain_with_the_unbiased_spatial_passes(oracle, room):
    """both unbiased toggles over the same orbit, the three spatial passes on the last frame. Measured by this test as committed
    (2 000 trials):
        control:                                        0.203160 against the truth's 0.203236, -0.8 SE, 0 pixels with |z| > 4
        reference merge + reference passes:             0.197294 = -2.92 %, -44.8 SE, 161 pixels with z < -4
        1/Z merge + 1/Z passes:                         0.202817 = -0.21 %, -3.2 SE, 2 pixels with |z| > 4 (max |z| 5.21)
    Inside the bound, but not centred as the merge alone is. Further runs of this function: 8 000 trials in the same numbering (its
    first 2 000 are these) -0.10 % = -3.0 SE with 0 pixels beyond 4; 6 000 trials that share no frame number (first=20000) -0.06 % =
    -1.5 SE beside a control of +0.2. Pooled over the 14 000 distinct trials about -0.08 % = -3.1 SE, every stretch below the truth,
    while the three unbiased passes alone stand at +0.3 SE over 12 000 trials: a small residual in the hand-over between the merge
    and the passes, a thirty-fifth of the reference chain's, not explained (docs/MEASUREMENT_LOG_r31.md section 2)."""
    m = _study(oracle, room, N_TRIALS_CHAIN, spatial=True)
    assert abs(m["control"]["d"]) <= 4.0, "the truth disagrees with itself: the run says nothing"
    assert m["biased"]["d"] <= -10.0
    assert abs(m["unbiased"]["d"]) <= 4.0


# ------------------------------------------------------------------------------------------------------------------- 5
def _no_history_view(oracle, room, W, H, kind):
    eye, at = _f32(EYE), _f32(AT)
    if kind == "away":  # looking the other way from the same place: behind the previous camera
        return View(oracle, room, W, H, eye, _f32(eye + (eye - at)))
    if kind == "sky":  # from far above the room, straight up: every previous pixel is sky
        return View(oracle, room, W, H, (0.0, 40.0, 0.0), (0.0, 80.0, 0.1))
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["away", "sky", "nan"])
@pytest.mark.parametrize("vis_reuse", [1, 0])
def test_no_history_leaves_the_candidates(oracle, room, kind, vis_reuse):
    """behind the previous camera, a previous image of sky only, a NaN camera: Z = r.M and the record is the candidates', ucw in bits"""
    W, H = 37, 29
    opt = oracle.default_options(use_temporal_resampling=1, use_visibility_reuse=vis_reuse)
    cur = View(oracle, room, W, H, EYE, AT)
    prev = cur if kind == "nan" else _no_history_view(oracle, room, W, H, kind)
    rg_prev = np.full(9, np.nan, np.float32) if kind == "nan" else prev.rg
    if kind == "sky":
        assert not prev.shaded.any()
    hist = _history(oracle, room, cur, opt)  # records that must not be read: whatever the previous view is, the buffer is full
    cand = room["scene"].generate_candidate(W, H, 9, cur.vis, cur.eye, opt)
    got, diag = tu.temporal(W, H, 9, room["tris"], cur.vis, prev.vis, cur.eye, rg_prev, cur.rg, opt, hist, cand.copy(), mode=tu.UNBIASED)
    sh = cur.shaded
    assert not diag[:, :5].any()
    assert np.array_equal(diag[sh, 5], cand["M"][sh])
    assert np.array_equal(_bits(got), _bits(cand))


# previous cameras that stood to one side of the current one, along its own axes (world units): the current image then reaches past
# ONE edge of the previous image, named in storage coordinates (fx = floorf(px + 0.5f), fr = floorf(pr + 0.5f) of temporal_reproject.h)
EDGE_PANS = {"fx < 0": (2.5, 0.0), "fx >= W": (-2.5, 0.0), "fr < 0": (0.0, 1.5), "fr >= H": (0.0, -1.5)}


def edge_pan_view(oracle, room, W, H, edge):
    cur = View(oracle, room, W, H, EYE, AT)
    r, u = cur.rg["right"][0].astype(np.float64), cur.rg["up"][0].astype(np.float64)
    dr, du = EDGE_PANS[edge]
    shift = dr * r / np.linalg.norm(r) + du * u / np.linalg.norm(u)
    return cur, View(oracle, room, W, H, _f32(_f32(EYE) + shift), _f32(_f32(AT) + shift))


def beyond_edge(tris, cur, prev, edge):
    """shaded pixels of `cur` whose surface point lies in front of `prev` and projects past the named edge of its image, and past
    that edge only (tr.project = tr_previous_pixel and its continuous coordinates)"""
    W, H = cur.W, cur.H
    pts, sh = tr.surface_points(tris, cur.vis, cur.eye)
    pix, cont = tr.project(pts, prev.rg, W, H)
    front = sh & ~np.isnan(cont[:, 0])
    fx, fr = np.floor(cont[:, 0] + np.float32(0.5)), np.floor(cont[:, 1] + np.float32(0.5))
    past = {"fx < 0": fx < 0, "fx >= W": fx >= W, "fr < 0": fr < 0, "fr >= H": fr >= H}
    for other, m in past.items():
        if other != edge:
            assert not (front & m).any(), f"the pan for {edge} also leaves by {other}"
    out = front & past[edge]
    assert not pix[out, 0].any(), "tr_previous_pixel calls a pixel past the edge valid"
    return out


@pytest.mark.parametrize("W,H", [(37, 29), (17, 9)])
@pytest.mark.parametrize("edge", list(EDGE_PANS))
@pytest.mark.parametrize("vis_reuse", [1, 0])
def test_no_history_off_each_edge(oracle, room, W, H, edge, vis_reuse):
    """a previous camera panned along +right, -right, +up, -up: shaded pixels project past the left, right, low-row and high-row
    edge of its image (at 37 x 29: 148, 195, 259 and 130 of 838 shaded pixels; at 17 x 9: 6, 6, 28 and 10 of 83). There nothing is
    gathered, Z = r.M and the record is the candidates' in bytes, while the rest of the image merges its history"""
    opt = oracle.default_options(use_temporal_resampling=1, use_visibility_reuse=vis_reuse)
    cur, prev = edge_pan_view(oracle, room, W, H, edge)
    out = beyond_edge(room["tris"], cur, prev, edge)
    assert out.sum() >= 6, f"{edge}: {int(out.sum())} shaded pixels past the edge, the case covers nothing"
    hist = _history(oracle, room, prev, opt)
    assert (hist["M"] > 0).sum() == prev.shaded.sum()  # a full buffer: an index formed from a pixel past the edge would read a record
    cand = room["scene"].generate_candidate(W, H, 11, cur.vis, cur.eye, opt)
    got, diag = tu.temporal(W, H, 11, room["tris"], cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, cand.copy(), mode=tu.UNBIASED)
    assert not diag[out, :5].any()
    assert np.array_equal(diag[out, 5], cand["M"][out])
    assert np.array_equal(_bits(got[out]), _bits(cand[out]))
    inside = cur.shaded & ~out
    assert (diag[inside, 0] == 1).sum() > inside.sum() // 2 and (got["M"][inside] > cand["M"][inside]).any()


@pytest.mark.parametrize("W,H", [(37, 29), (17, 9)])
def test_edges_lamps_and_the_cap(oracle, room, W, H):
    """a pan that pushes part of the image off an edge of the previous one, a previous view that shows lamps, and ris_sample_count = 4
    with a history above the cap of 80: every pixel's diag is consistent, Z lies between r.M and the sum, and a pixel without a valid
    history keeps its candidates"""
    opt = oracle.default_options(use_temporal_resampling=1, ris_sample_count=4)
    cur = View(oracle, room, W, H, EYE, AT)
    rg = cur.rg
    r = rg["right"][0].astype(np.float64)
    shift = 2.5 * r / np.linalg.norm(r)
    for prev in (View(oracle, room, W, H, _f32(_f32(EYE) + shift), _f32(_f32(AT) + shift)), View(oracle, room, W, H, (0.0, 2.0, 3.0), (0.0, 6.0, -1.5))):
        hist = _history(oracle, room, prev, opt, frames=22)
        assert hist["M"].max() == 84  # 4 candidates + a history capped at 80: above the cap, which the merge applies again
        cand = room["scene"].generate_candidate(W, H, 30, cur.vis, cur.eye, opt)
        got, diag = tu.temporal(W, H, 30, room["tris"], cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, cand.copy(), mode=tu.UNBIASED)
        sh = cur.shaded
        valid = diag[:, 0] == 1
        assert valid[sh].any() and (~valid[sh]).any(), "the case needs pixels with and without a history"
        assert not diag[~sh].any() and np.array_equal(_bits(got[~sh]), _bits(cand[~sh]))
        assert np.array_equal(_bits(got[sh & ~valid]), _bits(cand[sh & ~valid]))
        # the rejection heuristics scale the capped 80 down and the product is truncated: 78 or 79 across a pan, never the 84 held
        assert (diag[:, 4] <= 80).all() and (diag[:, 4] >= 72).any()
        assert np.array_equal(got["M"][sh], cand["M"][sh] + diag[sh, 4])
        assert np.array_equal(diag[sh, 5], cand["M"][sh] + np.where(diag[sh, 2] == 1, diag[sh, 4], 0))
        assert not (diag[:, 3] & diag[:, 1]).any(), "no ray from the history's origin where its own sample won"
        pts, _ = tr.surface_points(room["tris"], cur.vis, cur.eye)
        assert np.array_equal(_bits(got["origin_position"][sh]), _bits(pts[sh]))
