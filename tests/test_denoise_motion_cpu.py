"""rt_denoise_temporal_motion without a GPU: the restatement of tests/denoise_motion_ref.py (compiled from csrc/denoise_motion.h and
the other headers of the kernels) anchored to tests/denoise_temporal_ref.py, the coverage the GPU cases rely on, the edge cases of
the rule and the host's bookkeeping. The float64 statement is tested in tests/test_denoise_motion_spec_cpu.py.

Scene: the lamp room of tests/light_sampling_ref.py; its box (triangles 64-75) is moved by scenes.move_triangles.

One correction to what the issue expected of the toggle off: the box is 1.5 deep and MOVES[0] brings it forward by 1, so a strip of
its top face lies where the top face lay one call earlier, on the same plane with the same normal. Those pixels (12 of 215 at
64 x 48, 4 of 77 at 37 x 29) legitimately find a valid tap without the toggle and reach h = 2; every other box pixel has h = 1."""
import numpy as np
import pytest

import denoise_motion_ref as dm
import denoise_temporal_ref as dtr
import light_sampling_ref as ls
from test_temporal_motion_cpu import BOX_HI, BOX_LO, MOVES, Worlds, move, on_box
from test_temporal_reproject_cpu import _orbit

ORBIT = 0.1  # rad per call, the cases with a moving camera
K = 4


@pytest.fixture(scope="module")
def worlds(oracle):
    oracle.set_threads(oracle.effective_cpus())
    return Worlds(oracle)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, mask=None):
    a, b = _bits(a), _bits(b)
    return np.array_equal(a, b) if mask is None else np.array_equal(a[mask], b[mask])


def _flat(n):
    """an accumulation every surface pixel participates with (the coverage and edge cases look at h only)"""
    acc = np.ones((n, 4), np.float32)
    acc[:, :3] = 0.25
    return acc


class Frames:
    """oracle ReSTIR frames at accumulate = 0, one state per sequence"""

    def __init__(self, oracle, W, H):
        self.o, self.W, self.H, self.st, self.f = oracle, W, H, oracle.new_state(W, H), 0
        self.opt = oracle.bench_options(accumulate=0)

    def __call__(self, world, view):
        self.f += 1
        world["scene"].frame(self.W, self.H, self.f, view.rg, view.eye, self.opt, self.st, tone_map=False)
        return self.st["accum"].reshape(-1, 4).copy()


def _view(worlds, world, W, H, angle=0.0):
    return worlds.view(world, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, angle))


def _participating(M, acc):
    return ((M.words >> 30) == 0) & (acc[:, 3] != 0)


# ----------------------------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize("two_cameras", [False, True])
@pytest.mark.parametrize("mode", ["off", "empty"])
def test_toggle_off_or_empty_range_is_the_temporal_restatement(oracle, worlds, two_cameras, mode):
    """moments, colour history and image, bit for bit; `empty`: the toggle on and no update, and a followed call whose range is empty"""
    W, H = 37, 29
    w = worlds.of(worlds.base)
    M, T = dm.MotionRef(W, H, w["tris"], on=mode == "empty"), dtr.TemporalRef(W, H, w["tris"])
    fr = Frames(oracle, W, H)
    for j in range(3):
        v = _view(worlds, w, W, H, ORBIT * j if two_cameras else 0.0)
        acc = fr(w, v)
        if mode == "empty" and j == 2:
            M.update(w["tris"][0:0], 0)  # an update of no triangle: a new generation, an empty range, a followed call
        got, want = M(v.vis, v.eye, v.rg, acc), T(v.vis, v.eye, v.rg, acc)
        assert M.followed == (mode == "empty" and j == 2) and not M.diag[:, 0].any()
        assert _same(got[0], want[0]) and _same(got[1], want[1]) and _same(M.hcol, T.hcol), (mode, j)


@pytest.mark.parametrize("W,H", [(37, 29), (64, 48)])
@pytest.mark.parametrize("two_cameras", [False, True])
def test_pixels_off_the_range_keep_the_parents_integration(oracle, worlds, W, H, two_cameras):
    wa, wb = worlds.of(worlds.base), worlds.moved(MOVES[0])
    M, T = dm.MotionRef(W, H, wa["tris"], on=True, iterations=0), dtr.TemporalRef(W, H, wa["tris"], iterations=0)
    fr = Frames(oracle, W, H)
    va = _view(worlds, wa, W, H)
    acc = fr(wa, va)
    M(va.vis, va.eye, va.rg, acc), T(va.vis, va.eye, va.rg, acc)
    M.update(wb["tris"][BOX_LO:BOX_HI], BOX_LO)
    T.tris = dm._bytes(wb["tris"])
    vb = _view(worlds, wb, W, H, ORBIT if two_cameras else 0.0)
    acc = fr(wb, vb)
    (_, gm), (_, wm) = M(vb.vis, vb.eye, vb.rg, acc), T(vb.vis, vb.eye, vb.rg, acc)
    assert M.followed
    box, part = on_box(vb), _participating(M, acc)
    assert np.array_equal(M.diag[:, 0] == 1, box & part) and box.any()
    off = part & ~box
    assert off.any() and _same(gm, wm, off) and _same(M.hcol[:, :3], T.hcol[:, :3], off)
    assert not _same(gm, wm, box), "and on the box it is another history"


def test_an_update_that_no_pixel_shows_changes_nothing(oracle, worlds):
    """the emitters (triangles 76 ...: never a participating pixel's triangle), and a followed call all the same"""
    W, H = 37, 29
    wa = worlds.of(worlds.base)
    tb = move(worlds.base, (0.1, 0.0, 0.0), first=76, count=len(worlds.base) - 76)
    wb = worlds.of(tb)
    M, T = dm.MotionRef(W, H, wa["tris"], on=True), dtr.TemporalRef(W, H, wa["tris"])
    fr = Frames(oracle, W, H)
    va = _view(worlds, wa, W, H)
    acc = fr(wa, va)
    M(va.vis, va.eye, va.rg, acc), T(va.vis, va.eye, va.rg, acc)
    M.update(tb[76:], 76)
    T.tris = dm._bytes(tb)
    vb = _view(worlds, wb, W, H)
    acc = fr(wb, vb)
    got, want = M(vb.vis, vb.eye, vb.rg, acc), T(vb.vis, vb.eye, vb.rg, acc)
    assert M.followed and M.range() == dict(lo=76, hi=len(tb), generation=0) and not M.diag[:, 0].any()
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and _same(M.hcol, T.hcol)


# ---------------------------------------------------------------------------------------------------------------- coverage
def _moving_box(worlds, W, H, on, offset, k=K):
    """the box moved by `offset` before each of k calls, ending one `offset` in front of the lamp room's own box; per call the
    moments, the view and the restatement's diag. `chain`: the pixels of the last call whose previous point was visible all the way
    back, i.e. whose valid tap of largest weight lay on such a pixel of the call before (call 1: every participating pixel)."""
    off = np.asarray(offset, np.float32)
    t = move(worlds.base, tuple(off * np.float32(1 - k)))
    M = dm.MotionRef(W, H, t, on=on, iterations=0)
    acc = _flat(W * H)
    calls, chain = [], None
    for j in range(1, k + 1):
        t = move(t, offset)
        M.update(t[BOX_LO:BOX_HI], BOX_LO)
        v = worlds.view(worlds.of(t), W, H)
        _, mom = M(v.vis, v.eye, v.rg, acc)
        assert M.followed == (on and j > 1)
        part = _participating(M, acc)
        if j == 1:
            chain = part.copy()
        else:
            q = M.diag[:, 3] * W + M.diag[:, 2]
            chain = part & (M.diag[:, 1] > 0) & chain[np.maximum(q, 0)]
        calls.append(dict(mom=mom, view=v, diag=M.diag.copy(), box=on_box(v)))
    return calls, chain


def _same_plane_as_before(calls, tris, offset):
    """box pixels of the last call whose own pixel showed, one call earlier, the same face of the box, and that face's normal is
    perpendicular to the move: what a lookup that does not follow the box can still find (the top face and the sides, which a forward
    move slides along their own planes)"""
    cur, prev = calls[-1]["view"], calls[-2]["view"]
    ci, pi = cur.vis["index"], prev.vis["index"]
    v = tris["v"].astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    along = np.abs(n @ np.asarray(offset, np.float64)) <= 1e-9 * np.linalg.norm(n, axis=1)
    return calls[-1]["box"] & calls[-2]["box"] & ((ci - BOX_LO) // 2 == (pi - BOX_LO) // 2) & along[np.maximum(ci, 0)]


@pytest.mark.parametrize("W,H,count", [(64, 48, 215), (37, 29, 77)])
def test_followed_box_pixels_keep_their_history(worlds, W, H, count):
    """This test fails without the feature: with the toggle off (what the parent computes) the moving box starts again every call."""
    on, chain = _moving_box(worlds, W, H, True, MOVES[0])
    box = on[-1]["box"]
    kind = box & chain
    print(f"denoise motion coverage {W} x {H}: {int(box.sum())} box pixels, {int(kind.sum())} with a visible previous point in every call, "
          f"h with the toggle on: {np.unique(on[-1]['mom'][box, 2], return_counts=True)}")
    assert box.sum() == count
    assert 4 * kind.sum() >= 3 * box.sum(), "at least three quarters of the box pixels have a previous point that was visible"
    assert (on[-1]["mom"][kind, 2] == K).all()
    off, _ = _moving_box(worlds, W, H, False, MOVES[0])
    assert np.array_equal(off[-1]["box"], box)
    slid = _same_plane_as_before(off, worlds.base, MOVES[0])
    h_off = off[-1]["mom"][:, 2]
    print(f"denoise motion coverage {W} x {H}: toggle off h: {np.unique(h_off[box], return_counts=True)}; {int(slid.sum())} pixels see a face that slid along its own plane")
    assert (h_off[kind & ~slid] == 1.0).all() and (h_off[box] <= 2.0).all()
    assert 4 * (kind & ~slid).sum() >= 3 * box.sum()


def test_coverage_at_8_x_8(worlds):
    """6 box pixels; the move (0.4, 0, 0.3) one call earlier: the restatement's counts, printed and pinned"""
    W = H = 8
    t0 = worlds.base
    M = dm.MotionRef(W, H, t0, on=True, iterations=0)
    acc = _flat(W * H)
    v = worlds.view(worlds.of(t0), W, H)
    M(v.vis, v.eye, v.rg, acc)
    t1 = move(t0, MOVES[1])
    M.update(t1[BOX_LO:BOX_HI], BOX_LO)
    v = worlds.view(worlds.of(t1), W, H)
    _, mom = M(v.vis, v.eye, v.rg, acc)
    box = on_box(v)
    q = np.arange(W * H)
    other = box & (M.diag[:, 1] > 0) & ((M.diag[:, 2] != q % W) | (M.diag[:, 3] != q // W))
    counts = dict(box=int(box.sum()), valid=int((M.diag[box, 1] > 0).sum()), other=int(other.sum()), h2=int((mom[box, 2] == 2).sum()))
    print("denoise motion coverage 8 x 8:", MOVES[1], counts)
    assert M.followed and counts["other"] >= 1
    assert counts == COUNTS_8_X_8


COUNTS_8_X_8 = dict(box=4, valid=4, other=3, h2=4)


# -------------------------------------------------------------------------------------------------------------- edge cases
def _two_calls(worlds, wprev, wcur, W, H, lo=BOX_LO, hi=BOX_HI, eye_at=None, poke=None):
    """one call on wprev, one update of [lo, hi) to wcur, one followed call; and the camera-only restatement on the same input"""
    view = (lambda w: worlds.view(w, W, H, *eye_at)) if eye_at else (lambda w: worlds.view(w, W, H))
    M, T = dm.MotionRef(W, H, wprev["tris"], on=True, iterations=0), dtr.TemporalRef(W, H, wprev["tris"], iterations=0)
    acc = _flat(W * H)
    va = view(wprev)
    M(va.vis, va.eye, va.rg, acc), T(va.vis, va.eye, va.rg, acc)
    M.update(wcur["tris"][lo:hi], lo)
    T.tris = dm._bytes(wcur["tris"])
    if poke is not None:
        poke(M.tv_prev.view(np.float32).reshape(-1, 15)[:, :9].reshape(-1, 3, 3))
    vb = view(wcur)
    _, gm = M(vb.vis, vb.eye, vb.rg, acc)
    _, wm = T(vb.vis, vb.eye, vb.rg, acc)
    assert M.followed
    return M, T, va, vb, gm, wm


@pytest.mark.parametrize("W,H", [(37, 29), (8, 8)])
@pytest.mark.parametrize("offset", [(-9.0, 0.0, 0.0), (0.0, 0.0, 9.0)])
def test_the_box_came_from_outside_the_image_or_behind_the_camera(worlds, W, H, offset):
    M, T, va, vb, gm, wm = _two_calls(worlds, worlds.moved(offset), worlds.of(worlds.base), W, H)
    box = on_box(vb)
    assert box.any() and (M.diag[box, 0] == 1).all()
    assert np.isnan(M.coords[box]).all() or not (M.diag[box, 1] > 0).any()
    assert (gm[box, 2] == 1.0).all()
    assert _same(gm, wm, ~box)


def test_the_box_came_from_in_front_of_the_sky(worlds):
    """r24's view from below: the box comes down from above the panel; previous points that project onto sky or the panel find no tap"""
    W, H = 37, 29
    eye_at = ((0.0, 0.3, 3.0), (0.0, 5.0, -1.0))
    M, T, va, vb, gm, wm = _two_calls(worlds, worlds.moved((0.0, 5.2, 0.0)), worlds.moved((0.0, 3.0, 0.0)), W, H, eye_at=eye_at)
    box = on_box(vb) & (M.diag[:, 0] == 1)
    c = M.coords
    x0, r0 = np.floor(c[:, 0]), np.floor(c[:, 1])
    none = box & ~np.isnan(c[:, 0])
    for dx in (0, 1):
        for dy in (0, 1):
            qx, qr = x0 + dx, r0 + dy
            inside = none & (qx >= 0) & (qx < W) & (qr >= 0) & (qr < H)
            q = (np.where(inside, qr, 0) * W + np.where(inside, qx, 0)).astype(int)
            none &= ~inside | ~va.shaded[q]
    assert none.sum() > 0, "the camera must show box pixels whose previous taps were all sky or emissive"
    assert (gm[none, 2] == 1.0).all() and not (M.diag[none, 1] > 0).any()
    assert (gm[box, 2] == 2.0).any()


@pytest.mark.parametrize("what", ["nan", "inf", "-inf", "huge", "point", "line"])
def test_previous_vertices_that_were_nan_infinite_or_degenerate(worlds, what):
    W, H = 37, 29

    def poke(v):
        b = v[BOX_LO:BOX_HI]
        if what == "point":
            b[:, 1:] = b[:, :1]
        elif what == "line":
            b[:, 2] = (b[:, 0] + (b[:, 1] - b[:, 0]) * np.float32(2.0)).astype(np.float32)
        else:
            b[:, :, 1] = dict(nan=np.nan, inf=np.inf, huge=3e38)[what.lstrip("-")] * (-1 if what[0] == "-" else 1)

    w = worlds.of(worlds.base)
    M, T, va, vb, gm, wm = _two_calls(worlds, w, w, W, H, poke=poke)
    box = on_box(vb)
    assert box.any() and (wm[box, 2] == 2.0).all(), "the history matters on the box"
    assert (gm[box, 2] == 1.0).all() and not (M.diag[box, 1] > 0).any(), what
    if what in ("nan", "inf", "-inf", "huge"):
        assert np.isnan(M.coords[box]).all(), what  # dn_reproject refused the point
    assert _same(gm, wm, ~box) and _same(M.hcol[:, :3], T.hcol[:, :3], ~box)


def test_an_unmoved_triangle_inside_the_range(worlds):
    """range = floor, wall and box; only the box moved: the others' lookup point is their current one bit for bit, and they get the
    parent's result"""
    W, H = 37, 29
    M, T, va, vb, gm, wm = _two_calls(worlds, worlds.of(worlds.base), worlds.moved(MOVES[0]), W, H, lo=0, hi=BOX_HI)
    part = _participating(M, _flat(W * H))
    still = part & (vb.vis["index"] < BOX_LO)
    assert still.any() and (M.diag[still, 0] == 1).all() and M.range()["lo"] == 0
    assert _same(M.lookup[:, :3], M.gx[:, :3], still) and _same(M.lookup[:, 3:], M.gn[:, :3], still)
    assert _same(gm, wm, still) and _same(M.hcol[:, :3], T.hcol[:, :3], still)


def test_two_updates_of_two_spans_between_two_calls(worlds):
    W, H = 37, 29
    wa, wb = worlds.of(worlds.base), worlds.moved(MOVES[0])
    one, _, _, vb, gm1, _ = _two_calls(worlds, wa, wb, W, H)
    M = dm.MotionRef(W, H, wa["tris"], on=True, iterations=0)
    acc = _flat(W * H)
    va = worlds.view(wa, W, H)
    M(va.vis, va.eye, va.rg, acc)
    half = move(worlds.base, MOVES[0], first=64, count=6)
    M.update(half[64:70], 64)
    M.frame()  # a frame rendered in between re-bases nothing while only this toggle is on
    M.update(wb["tris"][70:76], 70)
    assert M.range() == dict(lo=64, hi=76, generation=0)
    _, gm2 = M(vb.vis, vb.eye, vb.rg, acc)
    assert M.followed and _same(gm1, gm2) and _same(one.hcol, M.hcol)
    assert (gm2[on_box(vb), 2] == 2.0).all()


def test_a_history_one_generation_too_old_gets_the_camera_only(worlds):
    """both toggles, in the order frame / update / denoise / update / frame / update / denoise: the last update re-bases for the ReSTIR
    history, the denoiser's is then one generation older than the kept vertices and the call equals denoise_temporal_ref"""
    W, H = 37, 29
    ts = [worlds.base]
    for _ in range(3):
        ts.append(move(ts[-1], (0.0, 0.0, 0.5)))
    M, T = dm.MotionRef(W, H, ts[0], on=True, motion=True, iterations=0), dtr.TemporalRef(W, H, ts[0], iterations=0)
    acc = _flat(W * H)

    def call(t):
        v = worlds.view(worlds.of(t), W, H)
        T.tris = dm._bytes(t)
        T.gx, T.gn, T.hcol, T.hmom, T.rg, T.has = M.gx, M.gn, M.hcol, M.hmom, M.rg, M.has  # the same previous state
        return M(v.vis, v.eye, v.rg, acc), T(v.vis, v.eye, v.rg, acc), v

    call(ts[0])
    M.frame()
    M.update(ts[1][BOX_LO:BOX_HI], BOX_LO)
    (_, gm), (_, wm), v = call(ts[1])
    assert M.followed and not _same(gm, wm, on_box(v))
    M.update(ts[2][BOX_LO:BOX_HI], BOX_LO)
    assert M.range()["generation"] == 1
    M.frame()
    M.update(ts[3][BOX_LO:BOX_HI], BOX_LO)
    assert M.range()["generation"] == 2 and M.dt_gen == 1
    (_, gm), (_, wm), v = call(ts[3])
    assert not M.followed and _same(gm, wm) and _same(M.hcol, T.hcol)


# ------------------------------------------------------------------------------------------------------------ what it buys
# r24's sequence (tests/test_temporal_motion_cpu.py): the box starts 2 units back and comes forward by 0.8 per frame for 6 frames, under
# a still camera and under an orbit of 0.1 rad per frame; oracle ReSTIR frames at accumulate = 0, one rt_denoise_temporal call per
# frame. Relative MSE (the metric of tests/test_denoise_temporal_cpu.py) over the box's participating pixels of the last denoised frame
# against 2 048 accumulated frames of the last scene.
#
# Measured (printed by the test; docs/MEASUREMENT_LOG_r25.md), means over STUDY_OFFSETS frame-number offsets:
#   still camera: raw 0.0859, rt_denoise 0.0069, toggle off 0.0058, toggle on 0.1443; on / off = 25.1 (paired difference 15.5 standard errors)
#   orbit:        raw 0.1044, rt_denoise 0.0086, toggle off 0.0069, toggle on 0.0901; on / off = 13.0 (13.3 standard errors)
#   box pixels with h >= 4: toggle on 100 %, toggle off 0 %.
# The toggle keeps the history and the history is out of date: the box's converged lighting changes along this path (top face 0.59 ...
# 0.44, front face 0.12 -> 0.0001), so the blended frames lag. With a step of 0.05 (lighting nearly constant) on / off is 0.95 / 0.89.
# Nothing is promised about the error; the test asserts that the run completes and that h >= 4 is more common with the toggle on.
STUDY_START, STUDY_STEP, STUDY_FRAMES, STUDY_ORBIT, STUDY_OFFSETS, CONVERGED_FRAMES = (0.0, 0.0, -2.0), (0.0, 0.0, 0.8), 6, 0.1, 24, 2048


def _rel_mse(out, ref, mask):
    x, g = (out[mask, :3] / out[mask, 3:4]).astype(np.float64), ref[mask]
    return float(np.mean((x - g) ** 2 / (g ** 2 + 1e-2)))


@pytest.mark.parametrize("mode", ["still", "orbit"])
def test_what_following_buys_on_the_moving_box(oracle, worlds, mode):
    import denoise_ref

    W, H = 64, 48
    ts = [move(worlds.base, STUDY_START)]
    for _ in range(1, STUDY_FRAMES):
        ts.append(move(ts[-1], STUDY_STEP))
    ws = [worlds.of(t) for t in ts]
    views = [_view(worlds, w, W, H, (STUDY_ORBIT if mode == "orbit" else 0.0) * k) for k, w in enumerate(ws)]
    last, sc = views[-1], ws[-1]["scene"]
    opt = oracle.default_options(accumulate=1)  # plain candidates: no reuse, no bias
    accum = np.zeros((W * H, 4), np.float32)
    for f in range(1, CONVERGED_FRAMES + 1):
        sc.resolve(accum, W, H, last.vis, last.eye, opt, sc.generate_candidate(W, H, 100000 + f, last.vis, last.eye, opt))
    ref = (accum[:, :3] / np.maximum(accum[:, 3:4], 1.0)).astype(np.float64)
    res = dict(on=[], off=[], spatial=[], raw=[])
    long_history = dict(on=[], off=[])
    fopt = oracle.bench_options(accumulate=0)
    for j in range(STUDY_OFFSETS):
        st = oracle.new_state(W, H)
        refs = dict(on=dm.MotionRef(W, H, ts[0], on=True), off=dm.MotionRef(W, H, ts[0], on=False))
        for k, (w, v) in enumerate(zip(ws, views)):
            w["scene"].frame(W, H, 1 + 1000 * j + k, v.rg, v.eye, fopt, st, tone_map=False)
            acc = st["accum"].reshape(-1, 4).copy()
            outs = {}
            for name, M in refs.items():
                if k:
                    M.update(ts[k][BOX_LO:BOX_HI], BOX_LO)
                outs[name], mom = M(v.vis, v.eye, v.rg, acc)
                assert M.followed == (name == "on" and k > 0)
        box = on_box(last) & _participating(refs["on"], acc)
        assert box.sum() > 200
        for name in ("on", "off"):
            res[name].append(_rel_mse(outs[name], ref, box))
            long_history[name].append(float((refs[name].hmom[box, 2] >= 4).mean()))
        res["spatial"].append(_rel_mse(denoise_ref.denoise(W, H, ts[-1], last.vis, last.eye, last.rg["up"][0], acc), ref, box))
        res["raw"].append(_rel_mse(acc, ref, box))
    r = {k: np.array(v) for k, v in res.items()}
    for k in ("raw", "spatial", "off", "on"):
        print(f"denoise motion study ({mode}) {k:8s}: relative MSE over the box {r[k].mean():.5f} (standard deviation {r[k].std(ddof=1):.5f}, {len(r[k])} offsets)")
    d = r["off"] - r["on"]
    se = d.std(ddof=1) / np.sqrt(len(d))
    print(f"denoise motion study ({mode}): on / off = {r['on'].mean() / r['off'].mean():.4f}; paired difference off - on {d.mean():.5f}, standard error {se:.5f} "
          f"({d.mean() / se:.1f} standard errors); box pixels with h >= 4: on {np.mean(long_history['on']):.4f}, off {np.mean(long_history['off']):.4f}")
    assert np.mean(long_history["on"]) > np.mean(long_history["off"])
