"""rt_temporal_motion without a GPU: the restatement of tests/temporal_motion_ref.py (compiled from csrc/temporal_motion.h and the other
headers of the kernels) anchored to tests/temporal_reproject_ref.py and to the oracle, its lookup checked against an independent
float64 statement, the coverage the GPU cases rely on, the edge cases of the rule, and what the toggle is for: a smaller error on a
moving object.

Scene: the lamp room of tests/light_sampling_ref.py; its box (triangles 64-75, non-emissive) is moved by scenes.move_triangles."""
import numpy as np
import pytest

import light_sampling_ref as ls
import temporal_motion_ref as tm
import temporal_reproject_ref as tr
from cedec_2024_rt_amd import scenes
from test_temporal_reproject_cpu import FOVY, View, _gathered, _history, _orbit, _project64, _res_diff

BOX_LO, BOX_HI = 64, 76
SIZES = [(64, 48), (37, 29), (8, 8)]
MOVES = [(0.0, 0.0, 1.0), (0.4, 0.0, 0.3)]
ORBIT = 0.3  # the previous camera of the cases with two cameras, as tests/test_temporal_reproject_cpu.py

# Largest difference between the binary32 continuous coordinates (px, pr) of the previous surface point (csrc/temporal_motion.h, then
# csrc/temporal_reproject.h) and the float64 statement of test_lookup_against_float64 over all of its cases (SIZES x MOVES x one and two
# cameras, pixels on the box in front of the previous camera): 4.937e-06 pixels, at 64 x 48 with the move (0.4, 0, 0.3) and two cameras
# (printed by the test; docs/MEASUREMENT_LOG_r24.md). DELTA = four times that, rounded up to two digits.
DELTA = 2.0e-5


def move(tris, offset, first=BOX_LO, count=BOX_HI - BOX_LO):
    m = np.zeros(len(tris), bool)
    m[first:first + count] = True
    return scenes.move_triangles(tris, m, offset)


class Worlds:
    """the lamp room and its variants, one oracle scene per triangle array (built on first use)"""

    def __init__(self, oracle):
        oracle.set_math_mode(oracle.MATH_PORTABLE)
        self.o = oracle
        self.base = ls.make_lamp_room()
        self._cache = {}

    def of(self, tris):
        key = tris.tobytes()
        if key not in self._cache:
            self._cache[key] = dict(tris=tris, scene=self.o.Scene(tris, use_bvh=True))
        return self._cache[key]

    def moved(self, offset, **kw):
        return self.of(move(self.base, offset, **kw))

    def view(self, world, W, H, eye=ls.LAMP_EYE, at=ls.LAMP_AT):
        return View(self.o, world, W, H, eye, at)


@pytest.fixture(scope="module")
def worlds(oracle):
    return Worlds(oracle)


def on_box(view, lo=BOX_LO, hi=BOX_HI):
    return view.shaded & (view.vis["index"] >= lo) & (view.vis["index"] < hi)


def merge(wcur, wprev, cur, prev, opt, hist, cand, lo=BOX_LO, hi=BOX_HI, frame=7):
    return tm.temporal(cur.W, cur.H, frame, wcur["tris"], wprev["tris"], cur.vis, prev.vis, cur.eye, prev.eye, prev.rg, cur.rg, lo, hi, opt, hist, cand.copy())


def other_pixel(diag, W):
    q = np.arange(len(diag))
    return (diag[:, 0] == 1) & ((diag[:, 1] != q % W) | (diag[:, 2] != q // W))


OPTION_CASES = [dict(), dict(use_visibility_reuse=0), dict(use_shadowed_target_function=1), dict(use_shadowed_target_function=1, use_visibility_reuse=0)]


# ----------------------------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize("kw", OPTION_CASES)
@pytest.mark.parametrize("two_cameras", [False, True])
def test_empty_range_is_the_reprojection_restatement(oracle, worlds, kw, two_cameras):
    W, H = 37, 29
    opt = oracle.bench_options(**kw)
    w = worlds.of(worlds.base)
    cur = worlds.view(w, W, H)
    prev = worlds.view(w, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT)) if two_cameras else cur
    hist = _history(oracle, w, prev, opt)
    cand = w["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
    want, wdiag = tr.temporal(W, H, 7, w["tris"], cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, cand.copy())
    for lo in (0, BOX_LO, len(w["tris"])):
        got, diag = merge(w, w, cur, prev, opt, hist, cand, lo, lo)
        assert not _res_diff(got, want), _res_diff(got, want)
        assert np.array_equal(diag[:, :3], wdiag[:, :3]) and not diag[:, 3].any()
    if not two_cameras:
        assert not _res_diff(want, w["scene"].temporal_resampling(W, H, 7, cur.vis, cur.eye, opt, hist, cand.copy()))


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("two_cameras", [False, True])
def test_pixels_off_the_moved_triangles_keep_their_record(oracle, worlds, W, H, two_cameras):
    opt = oracle.bench_options()
    wa, wb = worlds.of(worlds.base), worlds.moved(MOVES[0])
    cur = worlds.view(wb, W, H)
    prev = worlds.view(wa, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT)) if two_cameras else worlds.view(wa, W, H)
    hist = _history(oracle, wa, prev, opt)
    cand = wb["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
    got, diag = merge(wb, wa, cur, prev, opt, hist, cand)
    off = cur.shaded & ~on_box(cur)
    assert off.any() and on_box(cur).any() and np.array_equal(diag[:, 3] == 1, on_box(cur))
    want, wdiag = tr.temporal(W, H, 7, wb["tris"], cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, cand.copy())
    assert not _res_diff(got, want, off) and np.array_equal(diag[off, :3], wdiag[off, :3])
    if not two_cameras:
        assert not _res_diff(got, wb["scene"].temporal_resampling(W, H, 7, cur.vis, cur.eye, opt, hist, cand.copy()), off)
    # and on the box it is another merge
    assert _res_diff(got, want, on_box(cur))


def test_an_update_that_no_pixel_sees_changes_no_record(oracle, worlds):
    """lights only (triangles 76 ... are the emitters: never a shaded pixel's triangle), and the box with a range that is not its own"""
    W, H = 37, 29
    opt = oracle.bench_options()
    wa = worlds.of(worlds.base)
    wb = worlds.of(move(worlds.base, (0.1, 0.0, 0.0), first=76, count=len(worlds.base) - 76))
    cur, prev = worlds.view(wb, W, H), worlds.view(wa, W, H)
    hist = _history(oracle, wa, prev, opt)
    cand = wb["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
    got, diag = merge(wb, wa, cur, prev, opt, hist, cand, 76, len(worlds.base))
    assert not diag.any()
    assert not _res_diff(got, wb["scene"].temporal_resampling(W, H, 7, cur.vis, cur.eye, opt, hist, cand.copy()))


# ------------------------------------------------------------------------------------------------------------------ lookup
def _previous_points64(tris_prev, vis, mask):
    """numpy, float64: the pixel's barycentrics on the triangle's previous vertices"""
    v = tris_prev["v"][vis["index"][mask]].astype(np.float64)
    a, b = vis["uv"][mask][:, 0].astype(np.float64)[:, None], vis["uv"][mask][:, 1].astype(np.float64)[:, None]
    return (1.0 - a - b) * v[:, 0] + a * v[:, 1] + b * v[:, 2]


@pytest.fixture(scope="module")
def lookup_worst():
    return dict(worst=0.0, cases=0)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("offset", MOVES)
@pytest.mark.parametrize("two_cameras", [False, True])
def test_lookup_against_float64(oracle, worlds, lookup_worst, W, H, offset, two_cameras):
    opt = oracle.bench_options()
    wa, wb = worlds.of(worlds.base), worlds.moved(offset)
    cur = worlds.view(wb, W, H)
    prev = worlds.view(wa, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT)) if two_cameras else worlds.view(wa, W, H)
    hist = _history(oracle, wa, prev, opt)
    cand = wb["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
    got, diag = merge(wb, wa, cur, prev, opt, hist, cand)
    box = on_box(cur)
    assert box.any()
    pts32, _, m = tm.previous_points(wb["tris"], wa["tris"], cur.vis, prev.eye, BOX_LO, BOX_HI)
    assert np.array_equal(m, box)
    _, cont = tr.project(pts32[box], prev.rg, W, H)
    t, px, pr = _project64(_previous_points64(wa["tris"], cur.vis, box), prev.rg, W, H)
    assert (t > 0).all() and not np.isnan(cont).any()
    worst = max(float(np.abs(cont[:, 0] - px).max()), float(np.abs(cont[:, 1] - pr).max()))
    lookup_worst["worst"] = max(lookup_worst["worst"], worst)
    lookup_worst["cases"] += 1
    print(f"temporal motion {W} x {H} {offset} {'two cameras' if two_cameras else 'one camera'}: largest binary32 - float64 difference of (px, pr) = {worst:.3e} "
          f"pixels, over the cases so far {lookup_worst['worst']:.3e} (DELTA = {DELTA:.1e})")
    assert 4.0 * worst <= DELTA, "DELTA no longer covers four times the measured difference: measure again and say so in the log"
    d = diag[box]
    inside = (np.floor(px + 0.5) >= 0) & (np.floor(px + 0.5) < W) & (np.floor(pr + 0.5) >= 0) & (np.floor(pr + 0.5) < H)
    edge = np.zeros(len(px), bool)
    for c, n in ((px, W), (pr, H)):
        edge |= (np.abs(c + 0.5) <= DELTA) | (np.abs(c + 0.5 - n) <= DELTA)
    # away from the rounding point of an image edge: a point inside the previous image reports its nearest pixel, one outside none
    ins = ~edge & inside
    assert (np.abs(d[ins, 1] - px[ins]) <= 0.5 + DELTA).all() and (np.abs(d[ins, 2] - pr[ins]) <= 0.5 + DELTA).all()
    assert not d[~edge & ~inside, :3].any()
    v = d[:, 0] == 1
    assert v.any()
    assert (np.abs(d[v, 1] - px[v]) <= 0.5 + DELTA).all() and (np.abs(d[v, 2] - pr[v]) <= 0.5 + DELTA).all(), "not the nearest pixel of the float64 statement"
    # a valid history comes from a pixel that showed the box in the previous frame
    assert on_box(prev)[d[v, 2] * W + d[v, 1]].mean() > 0.8


# ---------------------------------------------------------------------------------------------------------------- coverage
def _coverage(oracle, worlds, W, H, offset):
    opt = oracle.bench_options()
    wa, wb = worlds.of(worlds.base), worlds.moved(offset)
    cur, prev = worlds.view(wb, W, H), worlds.view(wa, W, H)
    hist = _history(oracle, wa, prev, opt)
    cand = wb["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
    got, diag = merge(wb, wa, cur, prev, opt, hist, cand)
    same = wb["scene"].temporal_resampling(W, H, 7, cur.vis, cur.eye, opt, hist, cand.copy())
    box = on_box(cur)
    return dict(box=int(box.sum()), valid=int((diag[box, 0] == 1).sum()), other=int(other_pixel(diag, W)[box].sum()),
                same_keeps=int((same["M"][box] > cand["M"][box]).sum()), followed_keeps=int((got["M"][box] > cand["M"][box]).sum()))


def test_coverage_at_64_x_48(oracle, worlds):
    c = _coverage(oracle, worlds, 64, 48, MOVES[0])
    print("coverage 64 x 48:", c)
    assert c["box"] == 215
    assert 4 * c["other"] > 3 * c["box"], "more than three quarters of the box pixels gather a valid history from another pixel"
    assert 2 * c["same_keeps"] < c["box"], "the same-pixel lookup keeps an M above 0 on fewer than half of them"


def test_coverage_at_37_x_29(oracle, worlds):
    c = _coverage(oracle, worlds, 37, 29, MOVES[0])
    print("coverage 37 x 29:", c)
    assert c["box"] == 77 and c["valid"] >= 68 and 4 * c["other"] > 3 * c["box"]


@pytest.mark.parametrize("offset,box,other", [(MOVES[0], 6, 2), (MOVES[1], 4, 3)])
def test_coverage_at_8_x_8(oracle, worlds, offset, box, other):
    c = _coverage(oracle, worlds, 8, 8, offset)
    print("coverage 8 x 8:", offset, c)
    assert c["box"] == box and c["other"] == other and c["other"] >= 1


# -------------------------------------------------------------------------------------------------------------- edge cases
def oracle_merge(oracle, wcur, wprev, cur, prev, opt, hist, cand, diag, lo=BOX_LO, hi=BOX_HI, frame=7):
    """The oracle's temporal_resampling over the history numpy gathers from the restatement's diag. Its rejection heuristics read the
    current record's origin and the one eye it is given, so for the pixels of the range the candidates' origin is set to the previous
    surface point and normal (one camera, eye_prev = eye: the cases that use this) and put back where the candidate's sample stayed."""
    W = cur.W
    assert np.array_equal(cur.eye, prev.eye)
    pts, nrm, m = tm.previous_points(wcur["tris"], wprev["tris"], cur.vis, prev.eye, lo, hi)
    g = hist.copy()  # pixels off the range, one camera: the own pixel's record
    g[m] = _gathered(diag, hist, W)[m]
    c = cand.copy()
    c["origin_position"][m], c["origin_normal"][m] = pts[m], nrm[m]
    want = wcur["scene"].temporal_resampling(W, cur.H, frame, cur.vis, cur.eye, opt, g, c)
    def same(a, b, f):
        return (a[f].view(np.uint32) == b[f].view(np.uint32)).all(axis=1)

    # the candidate's sample stayed: the substituted origin came out, with the candidate's hit point and radiance
    stayed = m & same(want, c, "origin_position") & same(want, c, "origin_normal") & same(want, cand, "hit_position") & same(want, cand, "radiance")
    want["origin_position"][stayed], want["origin_normal"][stayed] = cand["origin_position"][stayed], cand["origin_normal"][stayed]
    return want


def _edge(oracle, worlds, wprev, wcur, W, H, kw=None, lo=BOX_LO, hi=BOX_HI, prev_eye_at=None):
    opt = oracle.bench_options(**(kw or {}))
    cur = worlds.view(wcur, W, H)
    prev = worlds.view(wprev, W, H, *(prev_eye_at or (ls.LAMP_EYE, ls.LAMP_AT)))
    hist = _history(oracle, wprev, prev, opt)
    cand = wcur["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
    got, diag = merge(wcur, wprev, cur, prev, opt, hist, cand, lo, hi)
    return opt, cur, prev, hist, cand, got, diag


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kw", [dict(), dict(use_shadowed_target_function=1)])
@pytest.mark.parametrize("offset", MOVES)
def test_a_moved_box_against_the_oracles_merge(oracle, worlds, W, H, kw, offset):
    wa, wb = worlds.of(worlds.base), worlds.moved(offset)
    opt, cur, prev, hist, cand, got, diag = _edge(oracle, worlds, wa, wb, W, H, kw)
    want = oracle_merge(oracle, wb, wa, cur, prev, opt, hist, cand, diag)
    assert not _res_diff(got, want), _res_diff(got, want)
    assert other_pixel(diag, W)[on_box(cur)].any()


@pytest.mark.parametrize("W,H", [(37, 29), (8, 8)])
def test_the_box_came_from_outside_the_previous_image(oracle, worlds, W, H):
    """previously 9 units to the left: its previous points project off the image, no history, the merge with Reservoir{}"""
    wa, wb = worlds.moved((-9.0, 0.0, 0.0)), worlds.of(worlds.base)
    opt, cur, prev, hist, cand, got, diag = _edge(oracle, worlds, wa, wb, W, H)
    box = on_box(cur)
    assert box.any() and not diag[box, :3].any()
    zero = wb["scene"].temporal_resampling(W, H, 7, cur.vis, cur.eye, opt, np.zeros_like(hist), cand.copy())
    assert not _res_diff(got, zero, box)
    assert not _res_diff(got, oracle_merge(oracle, wb, wa, cur, prev, opt, hist, cand, diag))


@pytest.mark.parametrize("W,H", [(37, 29), (8, 8)])
def test_the_box_came_from_behind_the_previous_camera(oracle, worlds, W, H):
    wa, wb = worlds.moved((0.0, 0.0, 9.0)), worlds.of(worlds.base)
    opt, cur, prev, hist, cand, got, diag = _edge(oracle, worlds, wa, wb, W, H)
    box = on_box(cur)
    pts, _, _ = tm.previous_points(wb["tris"], wa["tris"], cur.vis, prev.eye, BOX_LO, BOX_HI)
    assert box.any() and (pts[box, 2] > ls.LAMP_EYE[2]).all() and not diag[box, :3].any()
    zero = wb["scene"].temporal_resampling(W, H, 7, cur.vis, cur.eye, opt, np.zeros_like(hist), cand.copy())
    assert not _res_diff(got, zero, box)


def test_previous_pixels_that_were_sky_or_emissive(oracle, worlds):
    """seen from below, the box comes down from above the panel to in front of it: most pixels its previous points project to showed the
    panel (49 of 129), some the sky beside it (9), and held no history"""
    W, H = 37, 29
    eye_at = ((0.0, 0.3, 3.0), (0.0, 5.0, -1.0))
    wa, wb = worlds.moved((0.0, 5.2, 0.0)), worlds.moved((0.0, 3.0, 0.0))
    opt = oracle.bench_options()
    cur, prev = worlds.view(wb, W, H, *eye_at), worlds.view(wa, W, H, *eye_at)
    hist = _history(oracle, wa, prev, opt)
    # whatever garbage such a record holds is not read
    poisoned = hist.copy()
    bad = ~prev.shaded
    poisoned["M"][bad], poisoned["ucw"][bad], poisoned["w_sum"][bad], poisoned["visibility"][bad] = 77, np.float32(1e30), np.float32(1e30), 1
    cand = wb["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
    got, diag = merge(wb, wa, cur, prev, opt, poisoned, cand)
    box = on_box(cur)
    proj = box & ((diag[:, 1] != 0) | (diag[:, 2] != 0))
    qi = diag[:, 2] * W + diag[:, 1]
    sky, emi = proj & ~prev.hit[qi], proj & prev.emissive[qi]
    assert sky.sum() > 0 and emi.sum() > 0, f"the camera must show both kinds: {int(sky.sum())} sky, {int(emi.sum())} emissive"
    assert not diag[sky | emi, 0].any() and (diag[proj & prev.shaded[qi], 0] == 1).all()
    zero = wb["scene"].temporal_resampling(W, H, 7, cur.vis, cur.eye, opt, np.zeros_like(hist), cand.copy())
    assert not _res_diff(got, zero, sky | emi)
    assert not _res_diff(got, oracle_merge(oracle, wb, wa, cur, prev, opt, hist, cand, diag), cur.shaded & (box | prev.shaded))


@pytest.mark.parametrize("W,H", [(37, 29), (8, 8)])
def test_previous_vertices_that_were_nan_infinite_or_degenerate(oracle, worlds, W, H):
    """no index (the restatement traps on one outside its buffers), and the box's pixels hold the merge with Reservoir{}"""
    wb = worlds.of(worlds.base)
    opt = oracle.bench_options()
    cur = worlds.view(wb, W, H)
    hist = _history(oracle, wb, cur, opt)  # a full history under the same camera, which must not be merged
    cand = wb["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
    zero = wb["scene"].temporal_resampling(W, H, 7, cur.vis, cur.eye, opt, np.zeros_like(hist), cand.copy())
    same = wb["scene"].temporal_resampling(W, H, 7, cur.vis, cur.eye, opt, hist, cand.copy())
    box = on_box(cur)
    assert _res_diff(same, zero, box), "the history matters on the box"
    for what in ("nan", "inf", "-inf", "huge", "point", "line"):
        prev_tris = worlds.base.copy()
        v = prev_tris["v"]
        if what == "point":
            v[BOX_LO:BOX_HI, 1:] = v[BOX_LO:BOX_HI, :1]
        elif what == "line":
            v[BOX_LO:BOX_HI, 2] = (v[BOX_LO:BOX_HI, 0] + (v[BOX_LO:BOX_HI, 1] - v[BOX_LO:BOX_HI, 0]) * np.float32(2.0)).astype(np.float32)
        else:
            v[BOX_LO:BOX_HI, :, 1] = dict(nan=np.nan, inf=np.inf, huge=3e38)[what.lstrip("-")] * (-1 if what[0] == "-" else 1)
        got, diag = tm.temporal(W, H, 7, wb["tris"], prev_tris, cur.vis, cur.vis, cur.eye, cur.eye, cur.rg, cur.rg, BOX_LO, BOX_HI, opt, hist, cand.copy())
        if what in ("point", "line"):
            # a finite previous point, a NaN previous normal: a record may be gathered, and its M is scaled to 0
            assert (got["M"][box] == cand["M"][box]).all(), what
            for f in ("hit_position", "radiance", "w_sum", "ucw"):
                assert np.array_equal(got[f][box].view(np.uint32), zero[f][box].view(np.uint32)), (what, f)
        else:
            assert not diag[box, :3].any(), what
            assert not _res_diff(got, zero, box), what
        assert not _res_diff(got, same, cur.shaded & ~box), what


def test_two_updates_of_two_spans_between_two_frames(oracle, worlds):
    """the box's first six triangles and its last six moved by two updates, by different amounts: the covering range is the box"""
    W, H = 37, 29
    wa = worlds.of(worlds.base)
    t = move(move(worlds.base, (0.0, 0.0, 1.0), first=64, count=6), (0.0, 0.0, 1.0), first=70, count=6)
    assert np.array_equal(t.view(np.uint8), move(worlds.base, MOVES[0]).view(np.uint8))
    wb = worlds.of(t)
    opt, cur, prev, hist, cand, got, diag = _edge(oracle, worlds, wa, wb, W, H)
    assert not _res_diff(got, oracle_merge(oracle, wb, wa, cur, prev, opt, hist, cand, diag))
    # following one span only is another result: both are needed
    half, hdiag = merge(wb, wa, cur, prev, opt, hist, cand, 64, 70)
    assert _res_diff(got, half, on_box(cur))


def test_an_in_range_triangle_that_did_not_move(oracle, worlds):
    """range = the box and the floor / wall triangles before it; only the box moved. The others' previous point is their current one
    bit for bit, they project to their own pixel and merge what the same-pixel merge gives them"""
    W, H = 37, 29
    wa, wb = worlds.of(worlds.base), worlds.moved(MOVES[0])
    opt, cur, prev, hist, cand, got, diag = _edge(oracle, worlds, wa, wb, W, H, lo=0, hi=BOX_HI)
    still = cur.shaded & (cur.vis["index"] < BOX_LO)
    assert still.any() and (diag[still, 3] == 1).all()
    pts, nrm, m = tm.previous_points(wb["tris"], wa["tris"], cur.vis, prev.eye, 0, BOX_HI)
    cur_pts, _ = tr.surface_points(wb["tris"], cur.vis, cur.eye)
    assert np.array_equal(pts[still].view(np.uint32), cur_pts[still].view(np.uint32))
    assert not _res_diff(got, oracle_merge(oracle, wb, wa, cur, prev, opt, hist, cand, diag, lo=0, hi=BOX_HI))
    q = np.arange(W * H)
    own = (diag[:, 1] == q % W) & (diag[:, 2] == q // W)
    assert own[still].mean() > 0.95  # the nearest pixel of a pixel's own point is the pixel, up to rounding at a half
    # where it is the own pixel and that pixel was shaded, the record is the same-pixel merge's unless the candidate was empty
    # (the reference's heuristics then read a zero origin, these the surface point)
    same = wb["scene"].temporal_resampling(W, H, 7, cur.vis, cur.eye, opt, hist, cand.copy())
    full = still & own & (diag[:, 0] == 1) & (cand["w_sum"] > 0)
    assert full.any() and not _res_diff(got, same, full)


def test_a_history_one_update_too_old_gets_the_cameras_only(oracle, worlds):
    """what the host does with a history whose generation is not the one the kept vertices describe: the r23 launch, which is this
    restatement with an empty range (test_empty_range_is_the_reprojection_restatement); stated here on the moved scene"""
    W, H = 37, 29
    wa, wc = worlds.of(worlds.base), worlds.moved((0.0, 0.0, 2.0))
    opt = oracle.bench_options()
    cur, prev = worlds.view(wc, W, H), worlds.view(wa, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT))
    hist = _history(oracle, wa, prev, opt)
    cand = wc["scene"].generate_candidate(W, H, 7, cur.vis, cur.eye, opt)
    got, diag = merge(wc, worlds.moved(MOVES[0]), cur, prev, opt, hist, cand, 0, 0)
    want, _ = tr.temporal(W, H, 7, wc["tris"], cur.vis, prev.vis, cur.eye, prev.rg, cur.rg, opt, hist, cand.copy())
    assert not _res_diff(got, want) and not diag[:, 3].any()


# ------------------------------------------------------------------------------------------------------------ what it buys
# The box starts 2 units back and comes forward by 0.8 units per frame: from the second move on the same-pixel lookup keeps an M above
# 0 on 33, 42 and 18 of 177, 235 and 311 box pixels (the depth heuristic leaves exp(-32 * 0.64 / 7)), the followed one on 134, 206, 276.
STUDY_START, STUDY_STEP, STUDY_FRAMES, STUDY_ORBIT, OFFSETS, CONVERGED_FRAMES = (0.0, 0.0, -2.0), (0.0, 0.0, 0.8), 6, 0.1, 128, 2048

# measured by test_followed_history_lowers_the_error_on_the_moving_box (docs/MEASUREMENT_LOG_r24.md): RMSE(followed) / RMSE(r23) over the
# box's pixels of the last frame, means over OFFSETS frame-number offsets; the paired difference is 5.3 (still) and 4.5 (orbit)
# standard errors. A gain of 6 %: with 8 offsets it does not stand out of the noise (1.2 standard errors), hence the 128.
MEASURED_RHO = dict(still=0.9389, orbit=0.9370)


def _study_worlds(worlds):
    t = move(worlds.base, STUDY_START)
    out = [worlds.of(t)]
    for _ in range(1, STUDY_FRAMES):
        t = move(t, STUDY_STEP)
        out.append(worlds.of(t))
    return out


def _study_run(oracle, ws, views, first_frame, variant, orbit):
    """STUDY_FRAMES frames of 10_restir_di.cpp:257-379 with the benchmark options, one scene update (and camera step) per frame; the
    last frame's resolved image. variant: 'off' (no temporal reuse), 'r23' (the toggle off: cameras only), 'followed'"""
    W, H = views[0].W, views[0].H
    opt = oracle.bench_options(use_temporal_resampling=0 if variant == "off" else 1)
    hist = np.zeros(W * H, dtype=oracle.RESERVOIR)
    accum = np.zeros((W * H, 4), np.float32)
    for k, (w, v) in enumerate(zip(ws, views)):
        sc, f = w["scene"], first_frame + k
        r0 = sc.generate_candidate(W, H, f, v.vis, v.eye, opt)
        p, wp = (views[k - 1], ws[k - 1]) if k else (v, w)
        if variant == "followed" and k:
            tm.temporal(W, H, f, w["tris"], wp["tris"], v.vis, p.vis, v.eye, p.eye, p.rg, v.rg, BOX_LO, BOX_HI, opt, hist, r0)
        elif orbit and k:
            tr.temporal(W, H, f, w["tris"], v.vis, p.vis, v.eye, p.rg, v.rg, opt, hist, r0)
        else:
            sc.temporal_resampling(W, H, f, v.vis, v.eye, opt, hist, r0)
        hist = r0.copy()
        src = r0
        for q in range(int(opt["spatial_resampling_passes"][0])):
            src = sc.spatial_resampling(W, H, f, q, v.vis, v.eye, opt, src)
        accum[:] = 0
        sc.resolve(accum, W, H, v.vis, v.eye, opt, src)
    return accum[:, :3].copy()


@pytest.fixture(scope="module")
def motion_study(oracle, worlds):
    """computed once per camera mode: the converged image of the last scene at the last camera (plain candidates, CONVERGED_FRAMES
    frames accumulated, no reuse) and the RMSE over the box's pixels of the three variants over OFFSETS frame-number offsets"""
    W, H = 64, 48
    ws = _study_worlds(worlds)
    out = {}
    for mode, step in (("still", 0.0), ("orbit", STUDY_ORBIT)):
        views = [worlds.view(w, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, step * k)) for k, w in enumerate(ws)]
        last, sc = views[-1], ws[-1]["scene"]
        box = on_box(last)
        assert box.sum() > 200
        opt = oracle.default_options(accumulate=1)  # temporal and spatial reuse off
        accum = np.zeros((W * H, 4), np.float32)
        for f in range(1, CONVERGED_FRAMES + 1):
            res = sc.generate_candidate(W, H, 100000 + f, last.vis, last.eye, opt)
            sc.resolve(accum, W, H, last.vis, last.eye, opt, res)
        ref = (accum[:, :3] / np.maximum(accum[:, 3:4], 1.0))[box]
        out[mode] = {v: np.array([np.sqrt(np.mean((_study_run(oracle, ws, views, 1 + 1000 * j, v, step != 0.0)[box].astype(np.float64) - ref) ** 2))
                                  for j in range(OFFSETS)]) for v in ("off", "r23", "followed")}
    return out


@pytest.mark.parametrize("mode", ["still", "orbit"])
def test_followed_history_lowers_the_error_on_the_moving_box(motion_study, mode):
    """Measured (docs/MEASUREMENT_LOG_r24.md); the means, the ratio and the paired difference are printed. The
    assertion: the ratio of the mean RMSEs is at most the square root of the measured one, half the gain on a log scale."""
    r = motion_study[mode]
    for k in ("off", "r23", "followed"):
        print(f"motion study ({mode}), {k:8s}: mean RMSE {r[k].mean():.5f}, standard deviation {r[k].std(ddof=1):.5f} over {len(r[k])} offsets")
    d = r["r23"] - r["followed"]
    se = d.std(ddof=1) / np.sqrt(len(d))
    rho = r["followed"].mean() / r["r23"].mean()
    print(f"motion study ({mode}): rho = RMSE(followed) / RMSE(r23) = {rho:.4f}; paired difference r23 - followed: mean {d.mean():.5f}, "
          f"standard error {se:.5f} ({d.mean() / se:.1f} standard errors)")
    assert MEASURED_RHO[mode] is not None and MEASURED_RHO[mode] < 1.0
    assert rho <= np.sqrt(MEASURED_RHO[mode]), f"rho = {rho:.4f} above sqrt({MEASURED_RHO[mode]}) = {np.sqrt(MEASURED_RHO[mode]):.4f}"


# -------------------------------------------------------------------------------------------------------------- restir_app
def test_restir_app_follow_motion_needs_reproject():
    """argument checks come before any GPU call: --follow-motion implies nothing and errors without --reproject"""
    import os
    import subprocess

    app = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "app", "restir_app")
    p = subprocess.run([app, "--follow-motion"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--follow-motion needs --reproject" in p.stderr, p.stdout + p.stderr
    p = subprocess.run([app, "--move-tris", "0", "1", "0", "0", "0", "--move-lights", "0", "0", "0"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "exclude each other" in p.stderr, p.stdout + p.stderr
