"""rt_denoise_temporal_antilag without a GPU: the restatement of tests/denoise_antilag_ref.py (compiled from csrc/denoise_antilag.h and
the other headers of the kernels) anchored to tests/denoise_motion_ref.py, the rule on inputs whose answer is known, the window's
membership, images smaller than the window, and what the rule buys and costs: the moving box of tests/test_denoise_motion_cpu.py
(box and rest separately) and the static scene of tests/test_denoise_temporal_cpu.py. The float64 statement is tested in
tests/test_denoise_antilag_spec_cpu.py.

Scene: the lamp room of tests/light_sampling_ref.py; its box (triangles 64-75) is moved by scenes.move_triangles."""
import numpy as np
import pytest

import denoise_antilag_ref as da
import denoise_motion_ref as dm
from test_denoise_motion_cpu import (CONVERGED_FRAMES, ORBIT, STUDY_FRAMES, STUDY_OFFSETS, STUDY_ORBIT, STUDY_START, STUDY_STEP, Frames, _flat,
                                     _participating, _same, _view)
from test_denoise_motion_cpu import _rel_mse as _rel_mse_box
from test_temporal_motion_cpu import BOX_HI, BOX_LO, MOVES, Worlds, move, on_box


@pytest.fixture(scope="module")
def worlds(oracle):
    oracle.set_threads(oracle.effective_cpus())
    return Worlds(oracle)


def _window_count(W, H, R, gn, member, normals=True):
    """members of every pixel's window, counted in numpy: inside the image, `member`, n_p . n_q >= 0.9 (normals=False: any normal)"""
    n3 = gn[:, :3].astype(np.float64).reshape(H, W, 3)
    m = member.reshape(H, W)
    cnt = np.zeros((H, W), int)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            ys, xs = np.arange(H) + dy, np.arange(W) + dx
            oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            yy, xx = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
            q = n3[yy][:, xx]
            d = (n3 * q).sum(axis=2)
            assert not (np.abs(d - 0.9) < 1e-4).any(), "a normal pair on the threshold: choose another scene"
            cnt += (oky[:, None] & okx[None, :]) & m[yy][:, xx] & ((d >= 0.9) | (not normals))
    return cnt.reshape(-1)


# ----------------------------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize("two_cameras", [False, True])
@pytest.mark.parametrize("follow", [False, True])
@pytest.mark.parametrize("mode", ["off", "floor"])
def test_toggle_off_or_a_huge_floor_is_the_motion_restatement(oracle, worlds, two_cameras, follow, mode):
    """image, colour history and moments (.w = 0 included), bit for bit, over a moving box; `floor`: the toggle on with floor = 1e30,
    so that lambda' = 0 everywhere and the adapted path gives the bytes of the parent's"""
    W, H = 37, 29
    t = worlds.base
    al = dict(floor=1e30) if mode == "floor" else {}
    A, M = da.AntilagRef(W, H, t, on=follow, antilag=mode == "floor", al=al), dm.MotionRef(W, H, t, on=follow)
    fr = Frames(oracle, W, H)
    for j in range(4):
        if j:
            t = move(t, (0.0, 0.0, 0.25))
            A.update(t[BOX_LO:BOX_HI], BOX_LO), M.update(t[BOX_LO:BOX_HI], BOX_LO)
        w = worlds.of(t)
        v = _view(worlds, w, W, H, ORBIT * j if two_cameras else 0.0)
        acc = fr(w, v)
        got, want = A(v.vis, v.eye, v.rg, acc), M(v.vis, v.eye, v.rg, acc)
        assert A.followed == M.followed == (follow and j > 0) and A.adapted == (mode == "floor" and j > 0)
        assert _same(got[0], want[0]) and _same(got[1], want[1]) and _same(A.hcol, M.hcol), (mode, j)
        assert (got[1][:, 3] == 0.0).all()
        if A.adapted:
            assert np.isfinite(A.grad[:, 3]).any() and (A.grad[np.isfinite(A.grad[:, 3]), 3] < 1e-25).all()


def test_the_same_accumulation_twice_has_no_gradient(oracle, worlds):
    """0 iterations, still camera, floor = 0: the history of the second call is the first call's e, so lambda' = 0 and every byte is
    the toggle-off run's.

    One correction to what the issue expected: l_h == l_e holds to rounding, not bit for bit. dn_reproject returns a still camera's
    pixel to itself within about 1e-5 pixels, not exactly (tests/test_denoise_temporal_cpu.py allows 1e-3), so the bilinear taps give the
    neighbours a weight of that order. The test asserts what follows from that: the reprojection error it measures, times the largest
    ratio between a pixel's window sums, bounds lambda, and lambda stays far below gradient_lo."""
    W, H = 37, 29
    w = worlds.of(worlds.base)
    A = da.AntilagRef(W, H, w["tris"], antilag=True, al=dict(floor=0.0), iterations=0)
    M = dm.MotionRef(W, H, w["tris"], iterations=0)
    v = _view(worlds, w, W, H)
    acc = Frames(oracle, W, H)(w, v)
    for j in range(2):
        got, want = A(v.vis, v.eye, v.rg, acc), M(v.vis, v.eye, v.rg, acc)
    part = _participating(A, acc)
    assert A.adapted and part.sum() > W * H // 2 and (got[1][part, 2] == 2.0).all()
    xs, rs = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    off = max(float(np.abs(A.coords[part, 0] - xs[part]).max()), float(np.abs(A.coords[part, 1] - rs[part]).max()))
    lam = A.grad[part, 3]
    e = A.hcol[part, :3].max()
    print(f"same accumulation twice: reprojection off by at most {off:.3e} pixels, largest lambda {lam.max():.3e}")
    assert off <= 1e-3 and np.isfinite(lam).all()
    # a tap's weight is at most 2 * off; the largest e of the image over the smallest window mean bounds the relative change
    assert lam.max() <= 2.0 * off * e / float((A.grad[part, 0] / A.grad[part, 2]).min()) + 1e-6
    assert lam.max() < 0.01
    assert (got[1][:, 3] == 0.0).all()
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and _same(A.hcol, M.hcol)


def test_the_steepest_response_takes_the_frame(oracle, worlds):
    """lo = 0, hi = 1e-30, floor = 0: wherever mc != mh the integrated colour is e and the moments are (l, l^2), bit for bit"""
    W, H = 37, 29
    w = worlds.of(worlds.base)
    A = da.AntilagRef(W, H, w["tris"], antilag=True, al=dict(floor=0.0, gradient_lo=0.0, gradient_hi=1e-30), iterations=0)
    F = dm.MotionRef(W, H, w["tris"], iterations=0)  # a context that sees the last frame only: its e, l and l^2
    fr = Frames(oracle, W, H)
    v = _view(worlds, w, W, H)
    for j in range(3):
        acc = fr(w, v)
        _, mom = A(v.vis, v.eye, v.rg, acc)
    _, first = F(v.vis, v.eye, v.rg, acc)
    part = _participating(A, acc)
    differ = part & (A.grad[:, 0] != A.grad[:, 1])
    assert differ.sum() > part.sum() // 2
    assert (mom[differ, 3] == 1.0).all() and (mom[differ, 2] == 3.0).all()
    assert _same(A.hcol[:, :3], F.hcol[:, :3], differ) and _same(mom[:, :2], first[:, :2], differ)


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_noise_free_step(worlds):
    """a constant accumulation for 8 calls, then a rectangle of it scaled by 4: lambda = 3 / 4 where the window's members lie inside
    the rectangle, the blend follows the formula; a window that misses the rectangle changes nothing; without the toggle the step
    lags at 0.8 old + 0.2 new"""
    W, H, R = 64, 48, 3
    w = worlds.of(worlds.base)
    v = worlds.view(w, W, H)
    al = dict(radius=R, floor=0.0)
    A = da.AntilagRef(W, H, w["tris"], antilag=True, al=al, iterations=0)
    M = dm.MotionRef(W, H, w["tris"], iterations=0)
    acc = _flat(W * H)
    for _ in range(8):
        A(v.vis, v.eye, v.rg, acc), M(v.vis, v.eye, v.rg, acc)
    assert _same(A.hcol, M.hcol) and (A.hmom[:, 3] == 0.0).all(), "a constant input has no gradient"
    old = A.hcol[:, :3].astype(np.float64)
    x0, x1, y0, y1 = 12, 52, 8, 40
    rect = np.zeros((H, W), bool)
    rect[y0:y1, x0:x1] = True
    step = acc.copy()
    step[rect.reshape(-1), :3] *= np.float32(4.0)
    (_, gm), (_, wm) = A(v.vis, v.eye, v.rg, step), M(v.vis, v.eye, v.rg, step)
    part = _participating(A, step)
    assert (gm[part, 2] == 9.0).all()
    ys, xs = np.mgrid[0:H, 0:W]
    inside = ((xs >= x0 + R) & (xs < x1 - R) & (ys >= y0 + R) & (ys < y1 - R)).reshape(-1) & part
    outside = ((xs < x0 - R) | (xs >= x1 + R) | (ys < y0 - R) | (ys >= y1 + R)).reshape(-1) & part
    assert inside.sum() > 300 and outside.sum() > 300
    new = 4.0 * old
    lam = A.grad[:, 3].astype(np.float64)
    assert np.abs(lam[inside] - 0.75).max() <= 1e-6, np.abs(lam[inside] - 0.75).max()
    lr = np.clip((lam - al.get("gradient_lo", 0.2)) / (0.8 - 0.2), 0.0, 1.0)
    lr32 = np.clip((lam.astype(np.float32) - np.float32(0.2)) / (np.float32(0.8) - np.float32(0.2)), 0, 1)
    assert np.abs(gm[inside, 3] - lr32[inside]).max() <= 2e-7
    alpha = 0.2 + 0.8 * lr[inside, None]
    want = (1.0 - alpha) * old[inside] + alpha * new[inside]
    err = np.abs(A.hcol[inside, :3] - want) / np.maximum(want, 1e-30)
    print(f"noise-free step: lambda' {lr[inside].mean():.6f}, alpha' {alpha.mean():.6f}, worst relative difference to float64 {err.max():.3e}")
    assert err.max() <= 1e-5  # float32 rounding of e (the history was blended 8 times), of lambda' and of the blend
    assert (gm[outside, 3] == 0.0).all() and _same(gm, wm, outside) and _same(A.hcol[:, :3], M.hcol[:, :3], outside)
    lag = 0.8 * old[inside] + 0.2 * new[inside]
    assert (np.abs(M.hcol[inside, :3] - lag) / np.maximum(lag, 1e-30)).max() <= 1e-5 and (wm[:, 3] == 0.0).all()


def test_members(oracle, worlds):
    """the window leaves out the other plane across the wall / floor crease, pixels without a history of their own (the moved box
    without follow-motion: h = 1, .w = 0), and what does not participate"""
    W, H, R = 64, 48, 3
    t0, t1 = worlds.base, move(worlds.base, MOVES[0])
    A = da.AntilagRef(W, H, t0, antilag=True, al=dict(radius=R), iterations=0)
    fr = Frames(oracle, W, H)
    w0, w1 = worlds.of(t0), worlds.of(t1)
    v0 = _view(worlds, w0, W, H)
    A(v0.vis, v0.eye, v0.rg, fr(w0, v0))
    A.update(t1[BOX_LO:BOX_HI], BOX_LO)
    v1 = _view(worlds, w1, W, H)
    acc = fr(w1, v1)
    _, mom = A(v1.vis, v1.eye, v1.rg, acc)
    part = _participating(A, acc)
    has = part & (mom[:, 2] >= 2.0)
    fresh = part & (mom[:, 2] == 1.0)
    assert A.adapted and fresh.sum() > 100 and (on_box(v1) & fresh).sum() > 100
    assert (mom[fresh, 3] == 0.0).all() and np.isnan(A.grad[fresh]).all() and (mom[~part] == 0.0).all()
    want = _window_count(W, H, R, A.gn, has)
    assert np.array_equal(A.grad[has, 2].astype(int), want[has])
    full = np.minimum(np.arange(W) + R, W - 1) - np.maximum(np.arange(W) - R, 0) + 1
    full = (full[None, :] * (np.minimum(np.arange(H) + R, H - 1) - np.maximum(np.arange(H) - R, 0) + 1)[:, None]).reshape(-1)
    # the crease: pixels whose window holds participating pixels with a history on another plane
    every = _window_count(W, H, R, A.gn, has, normals=False)
    crease = has & (want < every)
    near_fresh = has & (every < _window_count(W, H, R, A.gn, part, normals=False))
    print(f"members: {int(crease.sum())} pixels leave out another plane, {int(near_fresh.sum())} a pixel without history; window sizes {np.unique(want[has])[[0, -1]]}")
    assert crease.sum() > 100 and near_fresh.sum() > 50 and (want[has] >= 1).all() and (want <= full).all()


@pytest.mark.parametrize("W,H", [(1, 1), (3, 70), (70, 3)])
def test_images_smaller_than_the_window(worlds, W, H):
    w = worlds.of(worlds.base)
    v = worlds.view(w, W, H)
    acc = _flat(W * H)
    rng = np.random.default_rng(5)
    for R in (1, 2, 3, 4):
        A = da.AntilagRef(W, H, w["tris"], antilag=True, al=dict(radius=R), iterations=1)
        Z = da.AntilagRef(W, H, w["tris"], antilag=True, al=dict(radius=R, floor=1e30), iterations=1)
        M = dm.MotionRef(W, H, w["tris"], iterations=1)
        for j in range(3):
            a = acc.copy()
            a[:, :3] *= rng.uniform(0.2, 4.0, (W * H, 1)).astype(np.float32)
            got, zero, want = A(v.vis, v.eye, v.rg, a), Z(v.vis, v.eye, v.rg, a), M(v.vis, v.eye, v.rg, a)
            assert _same(zero[0], want[0]) and _same(zero[1], want[1]) and _same(Z.hcol, M.hcol)
        part = _participating(A, a)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        if part.any():
            assert np.array_equal(A.grad[part, 2].astype(int), _window_count(W, H, R, A.gn, part)[part])
            assert (got[1][part, 2] == 3.0).all() and (got[1][part, 3] > 0.0).any() and (got[1][:, 3] <= 1.0).all()


# ------------------------------------------------------------------------------------------------------------ what it buys
# The sequence of tests/test_denoise_motion_cpu.py (the box comes forward 0.8 per frame for 6 frames; still camera and an orbit of 0.1
# rad per frame; oracle ReSTIR frames at accumulate = 0; relative MSE of the last denoised frame against 2 048 accumulated frames of the
# last scene), over the box and over `rest`: every participating pixel not on the box, i.e. the walls and the floor that do not move
# and whose shadows and bounce light the box changes.
#
# Measured (printed by the test; docs/MEASUREMENT_LOG_r30.md), means over STUDY_OFFSETS = 24 offsets, at the
# defaults (radius 4, lo 0.2, hi 0.8, floor 0.05), rest / box:
#   still: raw 0.1141 / 0.0859, rt_denoise 0.0184 / 0.0069, temporal 0.3206 / 0.0058, + anti-lag 0.0346 / 0.0057,
#          follow-motion 0.3242 / 0.1443, + anti-lag 0.0359 / 0.0274
#   orbit: raw 0.1956 / 0.1044, rt_denoise 0.0250 / 0.0086, temporal 0.3263 / 0.0069, + anti-lag 0.0313 / 0.0069,
#          follow-motion 0.3379 / 0.0901, + anti-lag 0.0335 / 0.0177
# Static scene (ratio to raw): orbit 0.0754 (without 0.0606, spatial-only 0.0914), still camera 0.1476 (0.1042, 0.1802).
def moving_box_study(oracle, worlds, mode, configs, offsets=STUDY_OFFSETS, converged=CONVERGED_FRAMES):
    """configs: name -> dict(on=follow-motion, antilag=, al=) ; returns name -> dict(box=[...], rest=[...]) plus `raw` and `spatial`"""
    import denoise_ref

    W, H = 64, 48
    ts = [move(worlds.base, STUDY_START)]
    for _ in range(1, STUDY_FRAMES):
        ts.append(move(ts[-1], STUDY_STEP))
    ws = [worlds.of(t) for t in ts]
    views = [_view(worlds, w, W, H, (STUDY_ORBIT if mode == "orbit" else 0.0) * k) for k, w in enumerate(ws)]
    last, sc = views[-1], ws[-1]["scene"]
    opt = oracle.default_options(accumulate=1)
    accum = np.zeros((W * H, 4), np.float32)
    for f in range(1, converged + 1):
        sc.resolve(accum, W, H, last.vis, last.eye, opt, sc.generate_candidate(W, H, 100000 + f, last.vis, last.eye, opt))
    ref = (accum[:, :3] / np.maximum(accum[:, 3:4], 1.0)).astype(np.float64)
    res = {k: dict(box=[], rest=[], fired=[]) for k in list(configs) + ["raw", "spatial"]}
    fopt = oracle.bench_options(accumulate=0)
    for j in range(offsets):
        st = oracle.new_state(W, H)
        refs = {k: da.AntilagRef(W, H, ts[0], **c) for k, c in configs.items()}
        for k, (w, v) in enumerate(zip(ws, views)):
            w["scene"].frame(W, H, 1 + 1000 * j + k, v.rg, v.eye, fopt, st, tone_map=False)
            acc = st["accum"].reshape(-1, 4).copy()
            outs = {}
            for name, A in refs.items():
                if k:
                    A.update(ts[k][BOX_LO:BOX_HI], BOX_LO)
                outs[name], _ = A(v.vis, v.eye, v.rg, acc)
        part = _participating(next(iter(refs.values())), acc)
        box, rest = on_box(last) & part, ~on_box(last) & part
        assert box.sum() > 200 and rest.sum() > 1500
        outs["raw"] = acc
        outs["spatial"] = denoise_ref.denoise(W, H, ts[-1], last.vis, last.eye, last.rg["up"][0], acc)
        for name, o in outs.items():
            res[name]["box"].append(_rel_mse_box(o, ref, box))
            res[name]["rest"].append(_rel_mse_box(o, ref, rest))
            if name in refs:
                res[name]["fired"].append(float((refs[name].hmom[part, 3] > 0).mean()))
    return {k: {m: np.array(x) for m, x in r.items()} for k, r in res.items()}


STUDY_CONFIGS = dict(off=dict(), on=dict(antilag=True), follow_off=dict(on=True), follow_on=dict(on=True, antilag=True))


@pytest.mark.parametrize("mode", ["still", "orbit"])
def test_what_anti_lag_buys_on_the_moving_box(oracle, worlds, mode):
    """Fails without the feature (there is no toggle to turn on). follow-motion off / on x anti-lag off / on, box and rest."""
    r = moving_box_study(oracle, worlds, mode, STUDY_CONFIGS)
    m = {k: {a: float(x.mean()) if len(x) else 0.0 for a, x in v.items()} for k, v in r.items()}
    for k in ("raw", "spatial", "off", "on", "follow_off", "follow_on"):
        print(f"denoise antilag study ({mode}) {k:10s}: relative MSE rest {m[k]['rest']:.5f} box {m[k]['box']:.5f}"
              + (f"  pixels with lambda' > 0: {m[k]['fired']:.4f}" if len(r[k]["fired"]) else ""))
    for a, b in (("off", "on"), ("follow_off", "follow_on")):
        d = r[a]["rest"] - r[b]["rest"]
        print(f"denoise antilag study ({mode}) rest {a} - {b}: {d.mean():.5f}, standard error {d.std(ddof=1) / np.sqrt(len(d)):.5f}")
    for on, off in (("on", "off"), ("follow_on", "follow_off")):
        assert m[on]["rest"] < m["raw"]["rest"], (mode, on)
        assert m[on]["rest"] < 0.25 * m[off]["rest"], (mode, on)
    assert m["follow_on"]["box"] < m["follow_off"]["box"], mode
    assert abs(m["on"]["box"] - m["off"]["box"]) <= 0.05 * m["off"]["box"], mode


# ------------------------------------------------------------------------------------------------------------ what it costs
def static_study(oracle, still, configs=None, frames=12):
    """tests/test_denoise_temporal_cpu.py's ReSTIR orbit (or the same frames under a still camera) on the 240 x 135 stand-in: the ratio
    denoised / raw of the relative MSE against the converged image of the last pose, for anti-lag off, spatial-only, and every entry
    of configs (name -> parameters; default: `on` = the defaults), with the share of pixels that responded and the mean lambda'"""
    import denoise_ref
    import test_denoise_temporal_cpu as tt
    from cedec_2024_rt_amd import scenes

    W, H = tt.W, tt.H
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    tris = scenes.make_blocks_restir()
    sc = oracle.Scene(tris, use_bvh=True)
    eye0, at0 = scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT
    poses = tt._orbit(oracle, eye0, at0, frames)
    if still:
        poses = [poses[0]] * frames
    configs = dict(on=None) if configs is None else configs
    refs = dict(off=da.AntilagRef(W, H, tris))
    refs.update({k: da.AntilagRef(W, H, tris, antilag=True, al=al) for k, al in configs.items()})
    seq = oracle.new_state(W, H)
    outs = {}
    for f, (eye, at) in enumerate(poses, start=1):
        rg = tt._camera(oracle, eye, at)
        vis = sc.raycast(W, H, rg)
        sc.frame(W, H, f, rg, np.asarray(eye, np.float32), oracle.bench_options(accumulate=0), seq, tone_map=False)
        raw = seq["accum"].reshape(-1, 4).copy()
        for k, A in refs.items():
            outs[k], _ = A(vis, eye, rg, raw)
    outs["spatial"] = denoise_ref.denoise(W, H, tris, vis, eye, rg["up"][0], raw)
    st = oracle.new_state(W, H)
    for k in range(1, tt.CONVERGED_FRAMES + 1):
        sc.frame(W, H, k, rg, np.asarray(eye, np.float32), oracle.bench_options(accumulate=1), st, tone_map=False)
    ref = st["accum"].reshape(-1, 4).copy()
    part = tt._participating(refs["off"].words, raw)
    assert part.sum() > W * H // 2
    ratios = {k: tt._rel_mse(raw, o, ref, part)[0] for k, o in outs.items()}
    for k in configs:
        ratios[k + ".fired"] = float((refs[k].hmom[part, 3] > 0).mean())
        ratios[k + ".mean_response"] = float(refs[k].hmom[part, 3].mean())
    return ratios


@pytest.mark.parametrize("still", [False, True])
def test_static_cost_stays_below_spatial_only(oracle, still):
    r = static_study(oracle, still)
    print(f"denoise antilag static ({'still' if still else 'orbit'}): off {r['off']:.4f} on {r['on']:.4f} spatial {r['spatial']:.4f}; "
          f"pixels with lambda' > 0: {r['on.fired']:.4f}, mean lambda' {r['on.mean_response']:.4f}")
    assert r["on"] < r["spatial"], r
