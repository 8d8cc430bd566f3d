"""The inputs and comparisons that tests/test_denoise_spec_cpu.py and tests/test_gpu_denoise_small.py share: a small scene on which
every term of the denoisers carries weight, camera sequences, noisy accumulation buffers, and the error measures between a result
and the float64 reference of tests/denoise_spec.py.

The scene (world units; the cameras sit near the origin with the default 45 degree field of view):
* a ring of 90 flat facets, 4 degrees apart, radius 6 around a tilted axis: neighbouring facets' normals differ by 4 degrees, so
  (n.n')^128 is 0.73 one facet over and 0.29 two over, and a tap on another facet is off the tangent plane by a fraction of a pixel;
* a terraced panel in front of it (a depth step against the ring): six strips with the same normal, each 0.15 behind the last, so
  the plane term alone separates them; its albedo has a zero channel;
* a folded screen of three quads that share their edges, with creases of 30 and 15 degrees (n.n' = 0.866 and 0.966): across a
  crease a reprojected tap lies within a fraction of a pixel of the tangent plane, so rt_denoise_temporal's normal test alone
  decides it, and the two creases sit on either side of its threshold of 0.9;
* an emissive triangle; sky above the ring.
The accumulation has gamma noise of relative sigma 0.14 per channel on every pixel (so no variance cancels to rounding noise),
sample counts 1..3 and a share of w == 0 records."""
import numpy as np

import denoise_spec as spec

TRIANGLE = np.dtype([("v", "<f4", (3, 3)), ("color", "<f4", 3), ("emissive", "<f4", 3)])
FOVY = np.float32(np.pi) / np.float32(4)
EYE, AT = (0.8, 0.3, 1.0), (0.3, 0.0, -6.0)
OTHER = dict(sigma_luminance=2.5, sigma_plane=0.5, normal_power_log2=3, variance_radius=1)  # tests/test_gpu_denoise.py's
PARITY_BAR = 1e-4  # the project's parity bar: a case whose tolerance needs more is ill-conditioned
SPREAD_FACTOR = 8.0
MARGIN_MIN = 1e-4
LEFT_OUT_MAX = 0.02


def scene():
    q = []

    def quad(a, b, c, d, color, emissive=(0, 0, 0)):
        q.append(((a, b, c), color, emissive))
        q.append(((a, c, d), color, emissive))

    tilt = np.deg2rad(20.0)
    rot = np.array([[np.cos(tilt), -np.sin(tilt), 0], [np.sin(tilt), np.cos(tilt), 0], [0, 0, 1]])
    for i in range(90):
        a0, a1 = np.deg2rad(4.0 * i + 1.0), np.deg2rad(4.0 * (i + 1) + 1.0)
        p0, p1 = np.array([6 * np.sin(a0), 0, -6 * np.cos(a0)]), np.array([6 * np.sin(a1), 0, -6 * np.cos(a1)])
        lo, hi = np.array([0, -4.0, 0]), np.array([0, 2.0, 0])
        quad(*(tuple(rot @ v) for v in (p0 + lo, p1 + lo, p1 + hi, p0 + hi)), (0.7, 0.5, 0.3))
    for i in range(6):
        x0, z = -2.2 + 0.35 * i, -3.6 - 0.15 * i
        x1 = x0 + (0.5 if i < 5 else 0.35)  # each strip reaches behind the next nearer one: no gap from any pose used here
        quad((x0, -2.5, z), (x1, -2.5, z), (x1, -0.3, z), (x0, -0.3, z), (0.2, 0.9, 0.0))
    px, pz, heading = 0.3, -4.4, 0.0  # the screen in plan view: 0.8 wide quads, turning by 30 and then by 15 degrees
    for turn in (0.0, 30.0, 15.0):
        heading += np.deg2rad(turn)
        nx, nz = px + 0.8 * np.cos(heading), pz + 0.8 * np.sin(heading)
        quad((px, -2.5, pz), (nx, -2.5, nz), (nx, -0.4, nz), (px, -0.4, pz), (0.6, 0.6, 0.4))
        px, pz = nx, nz
    q.append((((0.9, 0.5, -3.0), (1.9, 0.5, -3.0), (1.3, 1.4, -3.0)), (0.5, 0.5, 0.5), (5.0, 5.0, 5.0)))
    tris = np.zeros(len(q), TRIANGLE)
    for t, (v, c, e) in zip(tris, q):
        t["v"], t["color"], t["emissive"] = np.asarray(v, np.float32), c, e
    return tris


def raygen(ob, pose, W, H):
    return ob.raygen_lookat(pose[0], pose[1], (0, 1, 0), FOVY, W, H)


def pixel_world(H, dist=6.5):
    """world size of one pixel at `dist`"""
    return dist * 2.0 * np.tan(np.pi / 8) / H


def _yaw(eye, at, deg):
    e, a = np.asarray(eye, np.float64), np.asarray(at, np.float64)
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    d = a - e
    return tuple(e), tuple(e + np.array([c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]]))


def sequence(name, W, H):
    """the (eye, at) poses of one camera sequence"""
    e, a = np.asarray(EYE, np.float64), np.asarray(AT, np.float64)
    if name == "sideways":  # steps of 2.3 pixels at the ring's distance: fractional offsets around 0.3
        d = 2.3 * pixel_world(H)
        return [(tuple(e + (k * d, 0, 0)), tuple(a + (k * d, 0, 0))) for k in range(5)]
    if name == "dolly":
        fwd = (a - e) / np.linalg.norm(a - e)
        return [(tuple(e + fwd * z), tuple(a + fwd * z)) for z in (0.0, 0.4, 0.8, 0.4, 0.0)]
    if name == "turn":  # each step turns by a third of the horizontal field of view
        third = np.rad2deg(2 * np.arctan(np.tan(np.pi / 8) * W / H)) / 3
        return [_yaw(e, a, k * third) for k in (0, 1, 2, 1)]
    if name == "half_turn":
        return [_yaw(e, a, 0.0), _yaw(e, a, 180.0), _yaw(e, a, 0.0)]
    if name == "static":
        return [(EYE, AT)] * 36
    raise KeyError(name)


SEQUENCES = ("sideways", "dolly", "turn", "half_turn", "static")


def accumulation(W, H, seed, empty_seed=None, empty_share=0.1, blocks=False):
    """(W * H, 4) float32 {rgb sum, w}: a smooth pattern times gamma(50, 1/50) noise per channel (relative sigma 0.14, 0.105 in
    luminance), w in 1..3, and records that are all zero, chosen by empty_seed (so a sequence can keep them in place while the
    noise changes): `empty_share` of the pixels one by one, or with blocks=True four rectangles of W/6 x H/5 pixels"""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    base = (1.0 + 0.3 * np.sin(xs / 5.0) + 0.3 * (ys > H // 2)).ravel()
    w = rng.integers(1, 4, W * H).astype(np.float32)
    acc = np.zeros((W * H, 4), np.float32)
    acc[:, :3] = (base[:, None] * rng.gamma(50.0, 0.02, size=(W * H, 3)) * w[:, None]).astype(np.float32)
    acc[:, 3] = w
    erng = np.random.default_rng(seed if empty_seed is None else empty_seed)
    if blocks:
        empty = np.zeros((H, W), bool)
        bw, bh = max(1, W // 6), max(1, H // 5)
        for _ in range(4):
            x0, y0 = int(erng.integers(0, W - bw + 1)), int(erng.integers(0, H - bh + 1))
            empty[y0:y0 + bh, x0:x0 + bw] = True
        acc[empty.ravel()] = 0
    else:
        acc[erng.permutation(W * H)[:max(1, int(round(empty_share * W * H)))]] = 0
    return acc


def colour_error(a, ref):
    """per pixel: the largest channel difference over the largest reference channel (columns 0..2)"""
    a, ref = np.asarray(a, np.float64)[:, :3], np.asarray(ref, np.float64)[:, :3]
    return np.abs(a - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-30)


def scalar_error(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.abs(a - ref) / np.maximum(np.abs(ref), 1e-30)


def worst(err, mask):
    assert mask.any(), "nothing to compare"
    return float(err[mask].max())


def check(name, err, spread):
    """err (the result under test against the float64 reference) and spread (the float32 reference against it), both the worst
    over the compared pixels: the tolerance is SPREAD_FACTOR * spread and may not exceed the parity bar"""
    tol = SPREAD_FACTOR * spread
    msg = f"{name}: error {err:.3g}, spread {spread:.3g}, tol {tol:.3g}"
    assert tol <= PARITY_BAR, msg + " (ill-conditioned input)"
    assert err < tol, msg
    return dict(name=name, err=err, spread=spread, tol=tol)


class SpatialCase:
    """one guide and accumulation; the float64 reference, its float32 spread and the tolerance per parameter set, computed once"""

    def __init__(self, W, H, tris, vis, eye, rg, acc):
        self.W, self.H, self.tris, self.vis, self.eye, self.rg, self.acc = W, H, tris, vis, eye, rg, acc
        self._ref = {}

    def reference(self, **params):
        key = tuple(sorted(params.items()))
        if key not in self._ref:
            r64, part, cov = spec.denoise(self.W, self.H, self.tris, self.vis, self.eye, self.rg, self.acc, coverage=True, **params)
            r32, part32 = spec.denoise(self.W, self.H, self.tris, self.vis, self.eye, self.rg, self.acc, dtype=np.float32, **params)
            assert np.array_equal(part, part32)
            self._ref[key] = dict(hdr=r64, part=part, coverage=cov, spread=worst(colour_error(r32, r64), part))
        return self._ref[key]

    def compare(self, name, hdr, **params):
        """hdr (W * H, 4) float32 against the reference: every participating pixel within tol, every other one the accumulation's bits"""
        r = self.reference(**params)
        part = r["part"]
        hdr = np.ascontiguousarray(hdr, np.float32).reshape(-1, 4)
        assert np.array_equal(hdr[~part].view(np.uint32), self.acc[~part].view(np.uint32)), f"{name}: a pixel that does not participate changed"
        assert np.array_equal(r["hdr"][~part].astype(np.float32).view(np.uint32), self.acc[~part].view(np.uint32))
        assert (hdr[part, 3] == 1.0).all(), name
        return check(name, worst(colour_error(hdr, r["hdr"]), part), r["spread"])


def prev_state(T):
    """the state of a TemporalRef as denoise_spec.denoise_temporal takes it (None before the first call)"""
    return dict(gx=T.gx.copy(), gn=T.gn.copy(), hcol=T.hcol.copy(), hmom=T.hmom.copy(), rg=T.rg.copy()) if T.has else None


def _dilate(mask, W, H, reach):
    m = mask.reshape(H, W)
    if reach <= 0 or not m.any():
        return mask.copy()
    out = np.zeros_like(m)
    for r, c in zip(*np.nonzero(m)):
        out[max(0, r - reach):r + reach + 1, max(0, c - reach):c + reach + 1] = True
    return out.reshape(-1)


class TemporalCall:
    """the float64 reference of one call from the restatement's previous state (teacher forcing), its float32 spread, and the
    pixels left out because the float64 values sit within MARGIN_MIN of a discrete decision"""

    def __init__(self, W, H, tris, vis, eye, rg, acc, prev, **params):
        self.W, self.H, self.params = W, H, params
        self.r64 = spec.denoise_temporal(W, H, tris, vis, eye, rg, acc, prev, **params)
        self.r32 = spec.denoise_temporal(W, H, tris, vis, eye, rg, acc, prev, dtype=np.float32, **params)
        self.acc = acc
        self.part = self.r64["part"]
        self.left_out = self.part & (self.r64["margin"] < MARGIN_MIN)
        self.share = float(self.left_out.sum()) / max(1, int(self.part.sum()))
        p = dict(spec.SPATIAL_DEFAULTS)
        p.update(params)
        it = p["iterations"]
        # a level reads colour and variance 2 * step away, and the first variance reads colour variance_radius away
        self.reach_history = 0 if it == 0 else 2 + p["variance_radius"]
        self.reach_hdr = 0 if it == 0 else 2 * sum(1 << i for i in range(it)) + p["variance_radius"]

    def keep(self, reach):
        return self.part & ~_dilate(self.left_out, self.W, self.H, reach)

    def compare(self, name, hdr, mom, hcol=None):
        """one call's HDR image and moments (and colour history, where the caller has it) against the reference"""
        assert self.share <= LEFT_OUT_MAX, f"{name}: {self.share:.3%} of the participating pixels sit on a decision"
        r64, r32, part = self.r64, self.r32, self.part
        hdr, mom = (np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in (hdr, mom))
        assert np.array_equal(hdr[~part].view(np.uint32), self.acc[~part].view(np.uint32)), f"{name}: a pixel that does not participate changed"
        assert (mom[~part] == 0).all() and (mom[:, 3] == 0).all(), name
        k0 = self.keep(0)
        assert k0.any(), name
        bad = k0 & (mom[:, 2] != r64["moments"][:, 2])
        assert not bad.any(), f"{name}: h differs on {int(bad.sum())} pixels, e.g. pixel {int(np.flatnonzero(bad)[0])}: " \
                              f"{mom[bad, 2][0]} against {r64['moments'][bad, 2][0]}"
        out = []  # a figure whose comparison set is empty (everything within the filter's reach of a left-out pixel) is not made
        for j, what in ((0, "mu1"), (1, "mu2")):
            out.append(check(f"{name} {what}", worst(scalar_error(mom[:, j], r64["moments"][:, j]), k0),
                             worst(scalar_error(r32["moments"][:, j], r64["moments"][:, j]), k0)))
        if hcol is not None:
            kh = self.keep(self.reach_history)
            hcol = np.ascontiguousarray(hcol, np.float32).reshape(-1, 4)
            assert (hcol[~part, 3] == -1).all(), name
            if kh.any():
                out.append(check(f"{name} history", worst(colour_error(hcol, r64["history"]), kh), worst(colour_error(r32["history"], r64["history"]), kh)))
        ko = self.keep(self.reach_hdr)
        if ko.any():
            out.append(check(f"{name} hdr", worst(colour_error(hdr, r64["hdr"]), ko), worst(colour_error(r32["hdr"], r64["hdr"]), ko)))
        return out
