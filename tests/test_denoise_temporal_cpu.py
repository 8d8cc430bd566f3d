"""CPU. rt_denoise_temporal (csrc/denoise_math.h + the loops of csrc/denoise_kernels.h) restated on the host
(tests/denoise_temporal_ref.py, g++ -ffp-contract=off): the first call equals rt_denoise, a static camera reprojects every pixel
onto itself and grows the history by one per call up to 32, a sideways step behind a box starts the disoccluded wall afresh, and
under an orbit the temporal result beats the spatial-only one.

Measured with the defaults on the bench stand-in at 240 x 135: oracle frames at accumulate = 0 under an
orbit of 12 px left-button drags, against 256 accumulated frames at the final pose, relative MSE denoised / raw (the metric of
test_denoise_cpu.py) on the last frame:
  ReSTIR, 12 frames:      temporal 0.061, spatial-only 0.091 (0.66x the spatial ratio; the 0.5x stretch target is not reached);
                          mean luminance -6.5 % against -11.9 %
  07_pt 1 spp, 16 frames: temporal 0.110, spatial-only 0.091 (1.21x: worse, cause not investigated);
                          mean luminance -35 % against -51 %"""
import numpy as np
import pytest

import denoise_ref
import denoise_temporal_ref as dtr

W, H = 240, 135
CONVERGED_FRAMES = 256
ORBIT_DX = 12.0


def _lum(c):
    return 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]


@pytest.fixture(scope="module")
def stand_in(oracle):
    from cedec_2024_rt_amd import scenes

    oracle.set_math_mode(oracle.MATH_PORTABLE)
    oracle.set_threads(oracle.effective_cpus())
    tris = scenes.make_blocks_restir()
    return dict(ob=oracle, tris=tris, sc=oracle.Scene(tris, use_bvh=True), eye=scenes.BLOCKS_RESTIR_EYE, at=scenes.BLOCKS_RESTIR_LOOKAT)


def _camera(ob, eye, at, w=W, h=H):
    return ob.raygen_lookat(eye, at, (0, 1, 0), np.float32(np.pi) / np.float32(4), w, h)


def _orbit(ob, eye, at, frames):
    """the poses of `frames` frames: the first at (eye, at), each later one a left-button drag of ORBIT_DX pixels (rt_camera_orbit)"""
    poses = [(np.asarray(eye, np.float32), np.asarray(at, np.float32))]
    for _ in range(frames - 1):
        e, a, _ = ob.camera_control(poses[-1][0], poses[-1][1], 0, ORBIT_DX, 0.0)
        poses.append((e, a))
    return poses


def _participating(words, acc):
    return ((words >> 30) == 0) & (acc[:, 3] != 0)


def test_first_call_equals_rt_denoise(stand_in):
    s = stand_in
    ob = s["ob"]
    rg = _camera(ob, s["eye"], s["at"])
    vis = s["sc"].raycast(W, H, rg)
    st = ob.new_state(W, H)
    s["sc"].frame(W, H, 1, rg, np.asarray(s["eye"], np.float32), ob.bench_options(accumulate=0), st, tone_map=False)
    acc = st["accum"].reshape(-1, 4).copy()
    T = dtr.TemporalRef(W, H, s["tris"])
    for it in (0, 1, 5):
        T.reset()
        out, mom = T(vis, s["eye"], rg, acc, iterations=it)
        want = denoise_ref.denoise(W, H, s["tris"], vis, s["eye"], rg["up"][0], acc, iterations=it)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), it
        part = _participating(T.words, acc)
        assert (mom[part, 2] == 1.0).all() and (mom[~part] == 0.0).all()


def test_static_camera_reprojects_onto_itself(stand_in):
    s = stand_in
    ob = s["ob"]
    rg = _camera(ob, s["eye"], s["at"])
    vis = s["sc"].raycast(W, H, rg)
    st = ob.new_state(W, H)
    T = dtr.TemporalRef(W, H, s["tris"])
    opt = ob.bench_options(accumulate=0)
    xs, rs = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    for k in range(1, 35):
        s["sc"].frame(W, H, k, rg, np.asarray(s["eye"], np.float32), opt, st, tone_map=False)
        acc = st["accum"].reshape(-1, 4).copy()
        out, mom = T(vis, s["eye"], rg, acc)
        part = _participating(T.words, acc)
        assert part.sum() > W * H // 2
        if k > 1:
            c = T.coords[part]
            assert np.isfinite(c).all()
            assert float(np.abs(c[:, 0] - xs[part]).max()) <= 1e-3 and float(np.abs(c[:, 1] - rs[part]).max()) <= 1e-3
        assert (mom[part, 2] == min(k, 32)).all(), (k, np.unique(mom[part, 2]))
        assert (mom[~part] == 0.0).all()
        assert np.isfinite(out).all()


def _wall_and_box():
    """a wall at z = -6 facing +z (40 x 40) and a box [-0.6, 0.6]^2 x [-3.2, -2.0] in front of it, grey albedo"""
    q = []

    def quad(a, b, c, d):
        q.append((a, b, c))
        q.append((a, c, d))

    quad((-20, -20, -6), (20, -20, -6), (20, 20, -6), (-20, 20, -6))
    x0, x1, y0, y1, z0, z1 = -0.6, 0.6, -0.6, 0.6, -3.2, -2.0
    quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1))  # front
    quad((x1, y0, z1), (x1, y0, z0), (x1, y1, z0), (x1, y1, z1))  # right
    quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0))  # left
    quad((x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0))  # top
    quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1))  # bottom
    tris = np.zeros(len(q), dtype=[("v", "<f4", (3, 3)), ("color", "<f4", 3), ("emissive", "<f4", 3)])
    tris["v"] = np.asarray(q, np.float32)
    tris["color"] = 0.5
    return tris


def _project(rg, p):
    """continuous storage coordinates of world points p under a RayGenerator (numpy, float64)"""
    o, r, u = (np.asarray(rg[k], np.float64).reshape(3) for k in ("origin", "right", "up"))
    f = np.cross(u, r)
    f /= np.linalg.norm(f)
    d = p - o
    t = d @ f
    a, b = (d @ r) / (t * (r @ r)), (d @ u) / (t * (u @ u))
    return (a + 1) * 0.5 * W, (H - 1) - (1 - b) * 0.5 * H


def test_disocclusion_behind_a_sideways_step(oracle):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    tris = _wall_and_box()
    sc = oracle.Scene(tris, use_bvh=True)
    poses = [((0.0, 0.0, 2.0), (0.0, 0.0, -6.0)), ((0.5, 0.0, 2.0), (0.5, 0.0, -6.0))]
    T = dtr.TemporalRef(W, H, tris)
    acc = np.ones((W * H, 4), np.float32)
    acc[:, :3] = 0.25
    tri = []
    for eye, at in poses:
        rg = _camera(oracle, eye, at)
        vis = sc.raycast(W, H, rg)
        out, mom = T(vis, eye, rg, acc)
        tri.append(vis.view(np.int32).reshape(-1, 4)[:, 2].reshape(H, W).copy())
    assert (tri[0] >= 0).all() and (tri[1] >= 0).all()
    wall0, wall1 = tri[0] < 2, tri[1] < 2
    h = mom[:, 2].reshape(H, W)
    # where each wall pixel of the second frame was in the first one
    gx = T.gx[:, :3].astype(np.float64)
    px, pr = _project(_camera(oracle, *poses[0]), gx)
    px, pr = px.reshape(H, W), pr.reshape(H, W)

    def all_in(mask, x, r, rad):
        xi, ri = np.floor(x).astype(int), np.floor(r).astype(int)
        ok = np.ones(x.shape, bool)
        for dy in range(-rad, rad + 2):
            for dx in range(-rad, rad + 2):
                qx, qr = xi + dx, ri + dy
                inside = (qx >= 0) & (qx < W) & (qr >= 0) & (qr < H)
                ok &= inside & mask[np.clip(qr, 0, H - 1), np.clip(qx, 0, W - 1)]
        return ok

    rows, cols = np.mgrid[0:H, 0:W]
    away1 = all_in(wall1, cols.astype(float), rows.astype(float), 2)  # >= 2 px from an edge in the second frame
    covered = wall1 & away1 & all_in(~wall0, px, pr, 2)
    seen = wall1 & away1 & all_in(wall0, px, pr, 2)
    assert covered.sum() >= 200 and seen.sum() >= W * H // 2, (int(covered.sum()), int(seen.sum()))
    assert (h[covered] == 1).all(), np.unique(h[covered], return_counts=True)
    assert (h[seen] == 2).all(), np.unique(h[seen], return_counts=True)
    # the box itself is seen in both frames too
    box = ~wall1 & all_in(~wall1, cols.astype(float), rows.astype(float), 2) & all_in(~wall0, px, pr, 2)
    front = box & (np.abs(T.gn[:, 2].reshape(H, W) - 1.0) < 1e-6)
    assert front.sum() > 100 and (h[front] == 2).all()


def _rel_mse(raw, out, ref, part):
    col = lambda a: a[:, :3] / a[:, 3:4]  # noqa: E731
    r, d, g = col(raw)[part], col(out)[part], col(ref)[part]
    rel = lambda x: float(np.mean((x - g) ** 2 / (g ** 2 + 1e-2)))  # noqa: E731
    drift = float((_lum(d).mean() - _lum(r).mean()) / _lum(r).mean())
    return rel(d) / rel(r), drift


def _sequence(s, frames, render):
    """the temporal calls over an orbit of `frames` frames (render(f, rg, eye) -> accumulation) and the spatial-only call on
    the last frame: (temporal ratio, spatial ratio, temporal drift, spatial drift) against the converged image of the last pose"""
    ob = s["ob"]
    T = dtr.TemporalRef(W, H, s["tris"])
    for f, (eye, at) in enumerate(_orbit(ob, s["eye"], s["at"], frames), start=1):
        rg = _camera(ob, eye, at)
        vis = s["sc"].raycast(W, H, rg)
        raw = render(f, rg, eye, 0)
        out, _ = T(vis, eye, rg, raw)
    spatial = denoise_ref.denoise(W, H, s["tris"], vis, eye, rg["up"][0], raw)
    ref = render(0, rg, eye, CONVERGED_FRAMES)
    part = _participating(T.words, raw)
    assert part.sum() > W * H // 2
    assert np.array_equal(out[~part].view(np.uint32), raw[~part].view(np.uint32))
    rt, dt = _rel_mse(raw, out, ref, part)
    rs, ds = _rel_mse(raw, spatial, ref, part)
    return rt, rs, dt, ds


def test_restir_orbit_quality(stand_in):
    s = stand_in
    ob = s["ob"]

    seq = ob.new_state(W, H)  # one frame sequence: the reservoirs carry over from pose to pose, as in the frame loop

    def render(f, rg, eye, converge):
        if converge:
            st = ob.new_state(W, H)
            for k in range(1, converge + 1):
                s["sc"].frame(W, H, k, rg, np.asarray(eye, np.float32), ob.bench_options(accumulate=1), st, tone_map=False)
            return st["accum"].reshape(-1, 4).copy()
        s["sc"].frame(W, H, f, rg, np.asarray(eye, np.float32), ob.bench_options(accumulate=0), seq, tone_map=False)
        return seq["accum"].reshape(-1, 4).copy()

    rt, rs, dt, ds = _sequence(s, 12, render)
    print(f"ReSTIR orbit: temporal {rt:.4f} spatial {rs:.4f} ({rt / rs:.3f}x), drift {dt:+.4f} / {ds:+.4f}")
    assert rt < rs, (rt, rs)
    assert rt <= 0.075, rt  # measured 0.061 (spatial-only 0.091)


def test_path_trace_orbit_quality(stand_in):
    s = stand_in
    ob = s["ob"]

    def render(f, rg, eye, converge):
        acc = np.zeros((W * H, 4), np.float32)
        if converge:
            for k in range(1, converge + 1):
                s["sc"].path_trace(7, W, H, k, rg, ob.default_options(accumulate=1), acc)
        else:
            s["sc"].path_trace(7, W, H, f, rg, ob.default_options(accumulate=0), acc)
        return acc

    rt, rs, dt, ds = _sequence(s, 16, render)
    print(f"07_pt orbit: temporal {rt:.4f} spatial {rs:.4f} ({rt / rs:.3f}x), drift {dt:+.4f} / {ds:+.4f}")
    assert rt <= 0.13, rt  # measured 0.110 (spatial-only 0.091): recorded, not a goal met
    assert ds < dt <= 0.0, (dt, ds)  # measured -0.35 against -0.51: less energy lost than spatial-only
